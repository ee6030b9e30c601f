"""The count + checksum GRAM kernels on every compiled instance, against the CPU oracle, exactly (tests/gram_exact.py has the dictionaries,
the texts and the oracle's answers; tests/test_gram_exact_host.py checks those on the CPU) —

  gram_kernels.hip    gram_count_kernel<K, HAS_SHORT, TPB, DENSE, RANK_LDS, P>: 2 x 2 x {1024, 768, 512} x 2 x 2 at 16 positions per lane, and
                      eight more at 32 (only without short patterns, only 1024 threads): 56 instances      gram_version = 1, engine = Gram
  gram2_kernels.hip   gram2_kernel<K, S16 = true, DENSE, TPB>: 2 x 2 x {1024, 512} = 8 instances            gram_version = 2, engine = Gram
  gram2w_kernels.hip  gram2w_kernel<EXACT>: count + checksum and `.count()` alone                          a 40-class dictionary

Every comparison is for equality: the count of `.count()`, the count and the 64-bit checksum of `scan_count`.  After every call the whole of
daac_last_kernel() is compared with the line worked out here from the options, the buffer's alignment and the range — a shape chooser that
falls back in silence fails the test —, and the instance the line names goes into a ledger which the file's last test compares with the 56 +
8 + 2 expected.  (A call over an empty range launches nothing: its line is the family's name alone.)

Sizes.  The texts have 3 * 2048 + 5 bytes; lengths 0 .. 5, 15 .. 17, 1023 .. 1025, 2047 .. 2049 and the whole, each from buffer addresses 0, 5,
13 and 15 mod 16, with 2 KiB regions: load_chunk's first and last chunk, the carry over a region's start, the `after2` loads of a region's last
step and the step prefetch have their edges there.  `deep` (words end to end) hits and goes on at every position, `uniform` almost never."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import daachorse_amd as da
from daachorse_amd import Engine, ScanMode

import gram_exact as ge

OV = ScanMode.FindOverlapping
N = ge.TEXT_BYTES
V1_BASE = {"gram_version": 1, "threads": 1024, "gram_dense": 0, "gram_ppl": 16, "gram_region": 2048, "gram_slab": 4096, "blocks_per_cu": 0}
V2_BASE = {"gram_version": 2, "threads": 1024, "gram_dense": 0, "gram_region": 2048, "gram_slab": 4096, "blocks_per_cu": 0}
V1_DEFAULT_REGION, V2_DEFAULT_REGION, WIDE_DEFAULT_REGION = 16384, 65536, 16384   # api_scan.hip: CountPlan::region, resolve_count
# gram2's tables get gram_lds_budget less 16 KiB of hit rings (upload_layout.hpp:365); gram2.cpp takes K = 3 where M (4 C^3 bytes), its
# directory and CID (2 C^3) fit: with C = 9 more than 4 374 bytes, K = 2 less than 1 000
V2_K2_BUDGET = 16384 + 3072

# the instances that ran, as the labels named them
LEDGER_V1, LEDGER_V2, LEDGER_WIDE = set(), set(), set()
# (K, short, TPB, dense, rank in LDS, positions per lane)
EXPECTED_V1 = {(K, s, tpb, dense, rank, 16) for K in (3, 2) for s in (0, 1) for tpb in (1024, 768, 512) for dense in (0, 1) for rank in (0, 1)} | \
              {(K, 0, 1024, dense, rank, 32) for K in (3, 2) for dense in (0, 1) for rank in (0, 1)}
# (K, dir, dense, TPB)
EXPECTED_V2 = {(K, 1, dense, tpb) for K in (3, 2) for dense in (0, 1) for tpb in (1024, 512)}
EXPECTED_WIDE = {0, 1}
# compiled instances this file cannot reach; the list is fixed, each with its reason
UNREACHABLE_V2 = {
    (3, 2, 0, 1024): "32-bit directory entries need 65 536 depth-4 states: tests/test_gpu_gram_u32dir.py runs them",
    (3, 2, 0, 512): "32-bit directory entries need 65 536 depth-4 states: tests/test_gpu_gram_u32dir.py runs them",
    (3, 2, 1, 1024): "32-bit directory entries need 65 536 depth-4 states: tests/test_gpu_gram_u32dir.py runs them",
    (3, 2, 1, 512): "32-bit directory entries need 65 536 depth-4 states: tests/test_gpu_gram_u32dir.py runs them",
    (2, 2, 0, 1024): "no dictionary: at most 30 classes, 29^3 < 65 536 depth-3 states",
    (2, 2, 0, 512): "no dictionary: at most 30 classes, 29^3 < 65 536 depth-3 states",
    (2, 2, 1, 1024): "no dictionary: at most 30 classes, 29^3 < 65 536 depth-3 states",
    (2, 2, 1, 512): "no dictionary: at most 30 classes, 29^3 < 65 536 depth-3 states",
}
assert len(EXPECTED_V1) == 56 and len(EXPECTED_V2) == 8 and len(EXPECTED_V2 | set(UNREACHABLE_V2)) == 16


def _fields(lk):
    return dict(kv.split("=") for kv in lk.split()[1:])


def _pow2_region(opt, default):
    region = 2048
    while region * 2 <= max(2048, opt if opt > 0 else default):
        region *= 2
    return region


class World:
    """one dictionary on the device: its handles (v1 with the rank directory in the L2 and in the LDS, gram2, wide) and its texts at four
    buffer alignments"""

    def __init__(self, name):
        import torch
        self.name = name
        self.d = ge.dictionary(name)
        self.ncu = torch.cuda.get_device_properties(0).multi_processor_count
        self.handles, self.dev = {}, {}
        self.halo = max(len(w) for w in self.d.words) - 1

    def handle(self, family, rank=0):
        key = (family, rank)
        if key not in self.handles:
            p, rest = da.DoubleArrayAhoCorasick.deserialize(self.d.blob())
            assert rest == b""
            if family == "gram":
                p.set_option("gram_rank_in_lds", rank)   # (read when the tables are laid out, as gram_lds_budget is)
                if self.d.budget:
                    p.set_option("gram_lds_budget", self.d.budget)
                info = p.upload().info()
                assert info.gram_available and not info.gram_wide and info.gram_k == ge.EXPECT[self.name][0], (self.name, info.gram_k, p.explain())
            elif family == "gram2":
                if self.d.budget:
                    p.set_option("gram_lds_budget", V2_K2_BUDGET)
                info = p.upload().info()
                assert info.gram2_available and info.gram2_exact and info.gram2_k == ge.EXPECT[self.name][0], (self.name, info.gram2_k, p.explain())
            else:
                info = p.upload().info()
                assert info.gram_available and info.gram_wide and info.num_classes == 40, (self.name, info.num_classes, p.explain())
            assert info.max_pattern_len == self.halo + 1
            self.handles[key] = p
        return self.handles[key]

    def put(self, key, host, shift):
        import torch
        if (key, shift) not in self.dev:
            buf = torch.zeros(16 + len(host) + 32, dtype=torch.uint8, device="cuda")
            assert buf.data_ptr() % 16 == 0
            buf[shift:shift + len(host)].copy_(torch.from_numpy(host))
            self.dev[(key, shift)] = buf[shift:shift + len(host)]
        return self.dev[(key, shift)]

    def text(self, kind, shift=0, n=None):
        """the text (its first n bytes) in device memory, its first byte at an address `shift` mod 16"""
        t = self.put(kind, self.d.text(kind), shift)
        return t if n is None else t[:n]

    # ---- one call, its label and the ledger ----
    def _regions(self, region, shift, n, begin):
        frm = begin - min(begin, self.halo)          # a shard is scanned from max_pattern_len - 1 bytes in front of it
        lead = (shift + frm) % 16
        return -(-(lead + n - frm) // region)

    def v1(self, call, hay, shift, rank, opts=None, begin=0):
        """`count` or `scan_count` on gram_count_kernel -> the result; the label is asserted whole"""
        o = {**V1_BASE, **(opts or {})}
        p = self.handle("gram", rank)
        for k, v in o.items():
            p.set_option(k, v)
        got = getattr(p, call)(OV, hay, engine=Engine.Gram, **({"begin": begin} if begin else {}))
        lk = da.last_kernel()
        assert da.last_engine() == int(Engine.Gram), lk
        n = int(hay.numel())
        if n == begin:
            assert lk == "gram", lk
            return got
        K, short = ge.EXPECT[self.name]
        threads = min(1024, max(64, o["threads"] & ~63))
        plan_ppl = 32 if not short and o["gram_ppl"] != 16 else 16          # resolve_count; the slab is sized by it
        ppl = 32 if plan_ppl == 32 and threads > 768 else 16                 # launch_rl: 32 only in the 1024-thread instance
        region = _pow2_region(o["gram_region"], V1_DEFAULT_REGION)
        want = (f"gram K={K} short={short} waves={threads // 64} dense={o['gram_dense']} rank={'lds' if rank else 'l2'} ppl={ppl} region={region} "
                f"regions={self._regions(region, shift, n, begin)} slab={max(64 * plan_ppl + 192, o['gram_slab'])}")
        assert lk == want, (self.name, call, lk, want)
        LEDGER_V1.add((K, short, 1024 if threads > 768 else 768 if threads > 512 else 512, o["gram_dense"], rank, ppl))
        return got

    def v2(self, call, hay, shift, opts=None, begin=0):
        o = {**V2_BASE, **(opts or {})}
        p = self.handle("gram2")
        for k, v in o.items():
            p.set_option(k, v)
        got = getattr(p, call)(OV, hay, engine=Engine.Gram, **({"begin": begin} if begin else {}))
        lk = da.last_kernel()
        assert da.last_engine() == int(Engine.Gram), lk
        n = int(hay.numel())
        if n == begin:
            assert lk == "gram2", lk
            return got
        K = ge.EXPECT[self.name][0]
        threads = min(1024, max(64, o["threads"] & ~63))
        region = _pow2_region(o["gram_region"], V2_DEFAULT_REGION)
        want = f"gram2 K={K} dir=1 dense={o['gram_dense']} waves={threads // 64} region={region} regions={self._regions(region, shift, n, begin)}"
        assert lk == want, (self.name, call, lk, want)
        LEDGER_V2.add((K, 1, o["gram_dense"], 1024 if threads > 512 else 512))
        return got

    def wide(self, call, hay, shift, region_opt=2048, begin=0):
        p = self.handle("wide")
        p.set_option("gram_region", region_opt)
        got = getattr(p, call)(OV, hay, engine=Engine.Gram, **({"begin": begin} if begin else {}))
        lk = da.last_kernel()
        assert da.last_engine() == int(Engine.Gram), lk
        n = int(hay.numel())
        if n == begin:
            assert lk == "gram2w", lk
            return got
        exact = 1 if call == "scan_count" else 0
        region = _pow2_region(region_opt, WIDE_DEFAULT_REGION)
        want = f"gram2w exact={exact} region={region} regions={self._regions(region, shift, n, begin)}"
        assert lk == want, (self.name, call, lk, want)
        LEDGER_WIDE.add(exact)
        return got

    def both(self, run, kind, shift, n, begin=0, **kw):
        """`.count()` and count + checksum of the text's first n bytes from `begin` on, against the oracle's subset"""
        want = self.d.answer(kind, n, begin)
        hay = self.text(kind, shift, n)
        got = run("scan_count", hay, shift, begin=begin, **kw)
        assert got == want, (self.name, "scan_count", kind, shift, n, begin, kw, da.last_kernel(), got, want)
        got = run("count", hay, shift, begin=begin, **kw)
        assert got == want[0], (self.name, "count", kind, shift, n, begin, kw, da.last_kernel(), got, want[0])


_worlds = {}


def world(name):
    if name not in _worlds:
        _worlds[name] = World(name)
    return _worlds[name]


def _lengths(name):
    return ge.LENGTHS + (ge.C32_LENGTHS if name in ("c32", "c32n") else [])


# one instance per (K, HAS_SHORT, P) body of gram_count_kernel: (dictionary, positions per lane)
BODIES = [("k3s", 16), ("k3n", 16), ("k3n", 32), ("k2s", 16), ("k2n", 16), ("k2n", 32)]
BODY_IDS = [f"{n}-p{p}" for n, p in BODIES]


# ------------------------------------------------------------------------------------------------------------ gram_count_kernel
def _matrix(name, threads):
    w = world(name)
    short = ge.EXPECT[name][1]
    for rank in (0, 1):
        for dense in (0, 1):   # (a speed switch: both values on sparse and on dense text)
            for ppl in (16, 32) if not short and threads == 1024 else (16,):
                opts = {"threads": threads, "gram_dense": dense, "gram_ppl": ppl}
                for kind in ge.KINDS:
                    for n in _lengths(name):
                        for shift in ge.SHIFTS:
                            w.both(w.v1, kind, shift, n, rank=rank, opts=opts)


@pytest.mark.parametrize("threads", [1024, 768, 512])
@pytest.mark.parametrize("name", ["k3s", "k3n", "k2s", "k2n"])
def test_every_instance_of_gram_count_kernel(name, threads):
    """{dense 0, 1} x {rank directory in the L2, in the LDS} x {16, 32 positions per lane where the instance exists} of one (K, HAS_SHORT, TPB):
    every length from every buffer alignment on the three texts, 2 KiB regions"""
    _matrix(name, threads)


@pytest.mark.parametrize("name", ["c32", "c32n"])
def test_32_classes_fill_the_5_bit_fields(name):
    """31 distinct pattern bytes: classes 0 .. 31.  The class-31 byte stands first and second behind a depth-3 hit that ends on the last position
    lane 63 owns in a step and as the text's last byte (gram_exact.C32_PLANTS): the classes of the two bytes behind a hit travel in 5 bits each
    through the neighbour exchange, the hit ring and the walker slab.  c32 has short patterns and runs 16 positions per lane in all three
    thread-count instances (lane 63's last position: 1023 mod 1024); c32n has none and runs the 1024-thread instances at 16 and at 32
    positions per lane (2047 mod 2048), the only 32-class dictionary those eight instances see.  The label, asserted whole after every
    call, says short=0 and ppl=32 there."""
    w = world(name)
    info = w.handle("gram").info()
    assert info.num_classes == 32 and info.gram_k == 2
    # the planted continuations are what the oracle counts there: with them cut to four bits (class 15) the stem's walk finds no child
    text = w.d.text("uniform").tobytes()
    for last, behind in ge.C32_PLANTS:
        assert text[last - 2:last + 1 + len(behind)] == (ge.STEM + behind)[:N - (last - 2)]
    for threads in (1024, 768, 512) if name == "c32" else (1024,):
        _matrix(name, threads)
    if name == "c32n":   # the last call of the matrix: rank in the LDS, dense, 32 positions per lane
        f = _fields(da.last_kernel())
        assert (f["K"], f["short"], f["ppl"], f["waves"], f["rank"], f["dense"]) == ("2", "0", "32", "16", "lds", "1"), da.last_kernel()
        assert {(2, 0, 1024, dense, rank, 32) for dense in (0, 1) for rank in (0, 1)} <= LEDGER_V1


@pytest.mark.parametrize("name,ppl", BODIES, ids=BODY_IDS)
def test_other_launch_shapes(name, ppl):
    """one wave under the 512-thread instance and 15 waves under the 1024-thread one, one and two workgroups per CU, regions of 2 KiB, 4 KiB and the
    default, and the walker slab at its minimum on `deep` and `soup`: drain() then runs inside the step loop and the hit ring takes a batch on
    every group"""
    w = world(name)
    for threads in (64, 960):
        for bpc in (1, 2):
            for region in (2048, 4096, 0):
                opts = {"threads": threads, "blocks_per_cu": bpc, "gram_region": region, "gram_ppl": ppl}
                for kind in ge.KINDS:
                    for n, shift in ((N, 0), (N, 13), (4097, 5), (2049, 15)):
                        w.both(w.v1, kind, shift, n, rank=1, opts=opts)
                for kind in ("deep", "soup"):
                    for rank in (0, 1):
                        w.both(w.v1, kind, 5, N, rank=rank, opts={**opts, "gram_slab": 0, "gram_dense": 1})
                        w.both(w.v1, kind, 0, N, rank=rank, opts={**opts, "gram_slab": 0})


def _long_soup(w, n, seed):
    """n bytes of word soup on the device and the oracle's (count, checksum) of it (its own multi-threaded count: the tuple list of 16 MiB of
    word soup would be a few hundred MB)"""
    key = ("long", n, seed)
    if key not in w.dev:
        host = w.d.text_of(w.d.words, n, seed)
        w.dev[key] = (w.put(key, host, 0), w.d.oracle.overlapping_count(host, threads=8))
    return w.dev[key]


@pytest.mark.parametrize("name,ppl", BODIES, ids=BODY_IDS)
def test_several_regions_per_wave(name, ppl):
    """one 64-thread workgroup per CU over num_cu * 3 regions of 2 KiB and 5 bytes more: three regions per wave, then one wave with a fourth, a
    short one; and under the 1024- and 768-thread instances one soup of num_cu * 16 * 2 regions + 5 bytes (768 threads: 12 waves a workgroup,
    two rounds and two thirds of a third)"""
    w = world(name)
    n = w.ncu * 2048 * 3 + 5
    hay, want = _long_soup(w, n, 21)
    opts = {"threads": 64, "blocks_per_cu": 1, "gram_ppl": ppl}
    assert w.v1("scan_count", hay, 0, 1, opts) == want and w.v1("count", hay, 0, 0, opts) == want[0]
    assert int(_fields(da.last_kernel())["regions"]) == 3 * w.ncu + 1
    n = w.ncu * 16 * 2048 * 2 + 5
    hay, want = _long_soup(w, n, 22)
    for threads in (1024, 768):
        opts = {"threads": threads, "blocks_per_cu": 1, "gram_ppl": ppl}
        assert w.v1("scan_count", hay, 0, 0, opts) == want and w.v1("count", hay, 0, 1, opts) == want[0], (name, threads)
        assert int(_fields(da.last_kernel())["regions"]) == 32 * w.ncu + 1


def _shard_begins(w):
    K = ge.EXPECT.get(w.name, (2, 1))[0]
    return [1, K, K + 1, w.halo - 1, w.halo, w.halo + 1, 1024, 2048, 2049, N - 1]


@pytest.mark.parametrize("name,ppl", BODIES, ids=BODY_IDS)
def test_shards(name, ppl):
    """count and count + checksum from `begin` on: the scan of [begin - halo, n), the halo's own launch, shard_subtract_kernel — and
    shard_fixup_kernel where begin is within the halo of the start —, against the oracle's matches with begin < end <= n directly"""
    w = world(name)
    for kind in ("soup", "deep"):
        for begin in _shard_begins(w):
            for shift in (0, 13):
                w.both(w.v1, kind, shift, N, begin=begin, rank=1, opts={"gram_ppl": ppl})
            w.both(w.v1, kind, 5, N - 7, begin=min(begin, N - 8), rank=0, opts={"gram_ppl": ppl, "threads": 512, "gram_dense": 1})


@pytest.mark.parametrize("name,ppl", BODIES, ids=BODY_IDS)
def test_text_ends_inside_a_tail_record(name, ppl):
    """`soup` ends with the word of the 16-edge path; cut 1 .. 9 bytes short, the text ends inside the tail record's eight path bytes or inside a
    walker's look-ahead dword, and the bytes behind the end must read as bytes of no pattern (the buffer holds the rest of the word there)"""
    w = world(name)
    word = w.d.long_word
    assert len(word) == 6 + 16 and w.d.text("soup").tobytes().endswith(word)
    for cut in range(0, 10):
        for shift in (0, 5):
            for rank in (0, 1):
                w.both(w.v1, "soup", shift, N - cut, rank=rank, opts={"gram_ppl": ppl})
    # the whole word is found at full length and at no shorter one
    full, short = w.d.answer("soup", N), w.d.answer("soup", N - 1)
    assert full[0] > short[0]


# ------------------------------------------------------------------------------------------------------------ gram2_kernel, gram2w_kernel
@pytest.mark.parametrize("threads", [1024, 512])
@pytest.mark.parametrize("name", ["k3s", "k2s"])
def test_every_u16_instance_of_gram2_kernel(name, threads):
    """gram2_kernel<K, S16 = true, DENSE, TPB>: lengths, alignments, regions and shards as for the first table set"""
    w = world(name)
    for dense in (0, 1):
        opts = {"threads": threads, "gram_dense": dense}
        for kind in ge.KINDS:
            for n in ge.LENGTHS:
                for shift in ge.SHIFTS:
                    w.both(w.v2, kind, shift, n, opts=opts)
        for region in (4096, 0):
            for kind in ge.KINDS:
                w.both(w.v2, kind, 13, N, opts={**opts, "gram_region": region, "gram_slab": 0})
        for kind in ("soup", "deep"):
            for begin in _shard_begins(w):
                w.both(w.v2, kind, 5, N, begin=begin, opts=opts)
        for cut in range(1, 10):
            w.both(w.v2, "soup", 5, N - cut, opts=opts)


def test_gram2w_kernel_both_bodies():
    """gram2w_kernel<true> (count + checksum) and <false> (`.count()`) on the 40-class variant of k3s"""
    w = world("w40")
    for kind in ge.KINDS:
        for n in ge.LENGTHS:
            for shift in ge.SHIFTS:
                w.both(w.wide, kind, shift, n)
        w.both(w.wide, kind, 13, N, region_opt=0)
    for kind in ("soup", "deep"):
        for begin in _shard_begins(w):
            w.both(w.wide, kind, 5, N, begin=begin)


# ------------------------------------------------------------------------------------------------------------ the ledger
def test_ledger_every_reachable_instance_ran():
    """56 gram_count_kernel instances, the 8 gram2_kernel instances with 16-bit directory entries and both gram2w_kernel bodies must have run in
    the tests above: an instance that is missing fails this test.  Only where nothing at all ran before it — the test selected on its own, or in
    a process of its own — does it run the matrices itself first."""
    if not (LEDGER_V1 or LEDGER_V2 or LEDGER_WIDE):
        for name in ("k3s", "k3n", "k2s", "k2n"):
            for threads in (1024, 768, 512):
                _matrix(name, threads)
        for name in ("k3s", "k2s"):
            for threads in (1024, 512):
                test_every_u16_instance_of_gram2_kernel(name, threads)
        test_gram2w_kernel_both_bodies()
    print(f"instances run: gram {len(LEDGER_V1 & EXPECTED_V1)} of 56, gram2 {len(LEDGER_V2 & EXPECTED_V2)} of 8, gram2w {len(LEDGER_WIDE)} of 2")
    assert not sorted(EXPECTED_V1 - LEDGER_V1), sorted(EXPECTED_V1 - LEDGER_V1)
    assert LEDGER_V1 <= EXPECTED_V1, sorted(LEDGER_V1 - EXPECTED_V1)
    assert not sorted(EXPECTED_V2 - LEDGER_V2), sorted(EXPECTED_V2 - LEDGER_V2)
    assert LEDGER_V2 <= EXPECTED_V2 and not (LEDGER_V2 & set(UNREACHABLE_V2)), sorted(LEDGER_V2 - EXPECTED_V2)
    assert LEDGER_WIDE == EXPECTED_WIDE, LEDGER_WIDE
    assert len(UNREACHABLE_V2) == 8 and sum(k[0] == 3 for k in UNREACHABLE_V2) == 4
