"""The GRAM kernels on dictionaries with 65 536 and more depth-(K+1) states (tests/gram_u32dir.py): there the rank directory has 32-bit entries,
no per-word directory exists, and every consumer runs another compiled kernel than on any other dictionary of the suite —

  gram4_kernels.hip   gram4_kernel<3, Q, ARITH, DIR = 2, TPB, FILT, MPH>: 2 x 2 x 2 x {plain, FILT + rank, FILT + hash} = 24 instances, each with
                      the TAIL body the workgroup may take instead, and the density probe's 32-bit directory read
  gram2_kernels.hip   gram2_kernel<3, S16 = false, DENSE, TPB>: four instances (count + checksum; `.count()` with gram_version = 2)
  emit3_kernels.hip   emit3_detect_kernel<3, false>: every materialising overlapping scan, the lazy iterator, the steppers

(K = 2 never gets there: at most 30 byte classes give at most 29^3 depth-3 states.)  Every result is compared for equality with the CPU
oracle's find_overlapping_iter of the same bytes.  `high` is word soup of the words whose state has rank 65 536 and more: the hits a directory
read as 16 bits sends to the wrong record.  daac_last_kernel() is parsed after every gram4 call and every field of it asserted — the shape
chooser falls back in silence (16 -> 8 waves, no filter, the per-word directory asked for but absent) —, and the instances that ran are kept
in a ledger which the file's last test compares with the 24 x {tail 0, 1, auto} expected.  With gram_tail = -1 the label says `auto`: every
workgroup decides by its own probe, and only on haystacks of 1 MiB and more, so that setting runs on the whole of `holes` (uniform text: the
probe says no) and on 1 MiB of word soup (the probe says yes); either way the count must be the oracle's.

The three device table sets take their directory width from one host value (Gram2Tables::s16, copied to Gram2Dev, Gram4Dev and Gram2EmitDev
by the upload), so the handle whose gram4 launches report dir=2 runs the S16 = false instances of the other two kernels as well."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import daachorse_amd as da
from daachorse_amd import Engine, ScanMode

import gram_u32dir as gu

OV = ScanMode.FindOverlapping
LENGTHS = [1, 31, 32, 33, 2047, 2048, 2049, 3 * 2048 + 5]
SHIFTS = [0, 5, 13]
LONG_TAIL = (1 << 20) + 2048 + 5   # word soup long enough for the density probe
G4_BASE = {"gram_version": 4, "gram_ppl": 32, "gram_tail": 0, "gram2_rfull": 1, "threads": 1024, "gram4_arith": 1, "gram4_filter": 1, "gram_region": 2048,
           "gram_region_small": 0, "gram_taper_split": -1, "blocks_per_cu": 0, "gram_slab": 4096, "gram_dense": -1}
TAILS = {0: "0", 1: "1", -1: "auto"}

# (positions per lane, waves, arith, filter, mph, tail) of every gram4 launch that reported dir=2
LEDGER = set()
EXPECTED = {(ppl, waves, arith, f, m, tail) for ppl in (16, 32) for waves in (8, 16) for arith in (0, 1) for f, m in ((0, 0), (1, 0), (1, 1))
            for tail in TAILS.values()}


def _same(got, want):
    return len(got) == len(want) and np.array_equal(got["start"], want["start"]) and np.array_equal(got["end"], want["end"]) and \
        np.array_equal(got["value"], want["value"])


def _same16(got16, want):
    return len(got16) == len(want) and np.array_equal(got16["end"], want["end"]) and np.array_equal(got16["value"], want["value"]) and \
        np.array_equal(got16["length"].astype(np.uint64), want["end"] - want["start"])


class World:
    """one dictionary on the device: handles (`hash`: as uploaded by default, `rank`: gram4_mph = 0), its texts at three buffer alignments"""

    def __init__(self, name, rank_handle=False):
        import torch
        self.name = name
        self.d = gu.dictionary(name)
        self.ncu = torch.cuda.get_device_properties(0).multi_processor_count
        self.handles = {}
        for how, mph in (("hash", 8), ("rank", 0))[:2 if rank_handle else 1]:
            p, rest = da.DoubleArrayAhoCorasick.deserialize(self.d.blob())
            assert rest == b""
            p.set_option("gram4_mph", mph)   # (read when the tables are laid out)
            info = p.upload().info()
            assert info.gram2_available and info.gram2_k == 3 and info.gram2_exact, (name, info.gram2_k, info.gram2_exact)
            self.handles[how] = p
        self.dev = {}

    def text(self, kind, shift=0, n=None):
        """the text (its first n bytes) in device memory, its first byte at an address `shift` mod 16"""
        import torch
        key = (kind, shift) if kind != "long" else (kind, shift, n)
        if key not in self.dev:
            host = self.d.text(kind, n if kind == "long" else None)
            buf = torch.zeros(16 + len(host) + 32, dtype=torch.uint8, device="cuda")
            assert buf.data_ptr() % 16 == 0
            buf[shift:shift + len(host)].copy_(torch.from_numpy(host))
            self.dev[key] = buf[shift:shift + len(host)]
        t = self.dev[key]
        return t if n is None else t[:n]

    def count4(self, how, hay, opts=None, **kw):
        """`.count()` on the gram4 kernel -> (count, the fields of daac_last_kernel())"""
        p = self.handles[how]
        for k, v in {**G4_BASE, **(opts or {})}.items():
            p.set_option(k, v)
        got = p.count(OV, hay, engine=Engine.Gram, **kw)
        lk = da.last_kernel()
        assert da.last_engine() == int(Engine.Gram) and lk.startswith("gram4 "), lk
        f = dict(kv.split("=") for kv in lk.split()[1:])
        if f["dir"] == "2":
            LEDGER.add((int(f["ppl"]), int(f["waves"]), int(f["arith"]), int(f["filter"]), int(f["mph"]), f["tail"]))
        return got, f

    def lds_sum(self, how, ppl, waves, arith, filt):
        """gram4_plan's LDS sum for a shape, written out from the table sizes: hit lists (256 u16 a wave) + a text slot a wave (64 * ppl + 32) +
        the class table (unless arithmetic) + the directory's place (with the filter: the larger of it and [front table | Bloom array]) + M"""
        c = self.d.letters + 1
        m_bytes = (c ** 3 + 3) // 4 * 16
        s_bytes = (m_bytes // 16 * (4 if self.d.n_deep >= gu.THRESHOLD else 2) + 15) // 16 * 16
        return waves * 256 * 2 + waves * (64 * ppl + 32) + (0 if arith else 256) + s_bytes + m_bytes, s_bytes, m_bytes


_worlds = {}


def world(name):
    if name not in _worlds:
        _worlds[name] = World(name, rank_handle=name in ("big20", "big20s"))
    return _worlds[name]


# body -> [(dictionary, handle, gram4_arith option, arith that must run)], and the filter / mph fields the label must carry
TARGETS = {
    "plain": ([("big20", "hash", 1, 1), ("big20", "hash", 0, 0), ("big20s", "hash", 1, 0)], {"gram4_filter": 0}, ("0", "0")),
    "filt+rank": ([("big20", "rank", 1, 1), ("big20", "rank", 0, 0), ("big20s", "rank", 1, 0), ("big18", "hash", 1, 1), ("big18", "hash", 0, 0)], {}, ("1", "0")),
    "filt+hash": ([("big20", "hash", 1, 1), ("big20", "hash", 0, 0), ("big20s", "hash", 1, 0)], {}, ("1", "1")),
}
CASES = [(body, i) for body, (targets, _, _) in TARGETS.items() for i in range(len(targets))]


@pytest.mark.parametrize("body,which", CASES, ids=[f"{b}-{TARGETS[b][0][i][0]}-{TARGETS[b][0][i][1]}-arith{TARGETS[b][0][i][2]}" for b, i in CASES])
def test_every_dir2_instance_of_gram4(body, which):
    """16 / 32 positions per lane x 512 / 1024 threads x tail 0 / 1 / auto of one (dictionary, body): lengths around a lane's share, a step and a
    region of `holes` from three buffer alignments, `holes` whole, `soup` and `high` whole with the walker slab at its minimum (with and without
    the per-word directory asked for: there is none, the launch must say dir=2 either way), and 1 MiB of word soup"""
    targets, body_opts, (filt, mph) = TARGETS[body]
    name, how, arith_opt, arith = targets[which]
    w = world(name)
    d = w.d
    for ppl in (16, 32):
        for threads in (512, 1024):
            for tail in (0, 1, -1):
                opts = {"gram_ppl": ppl, "threads": threads, "gram_tail": tail, "gram4_arith": arith_opt, **body_opts}
                label = {"ppl": str(ppl), "dir": "2", "waves": str(threads // 64), "arith": str(arith), "filter": filt, "mph": mph, "tail": TAILS[tail]}

                def check(got, lk, want, what):
                    assert {k: lk.get(k) for k in label} == label, (name, body, what, lk, label, w.lds_sum(how, ppl, threads // 64, arith, filt == "1"))
                    assert got == want, (name, body, what, opts, lk, got, want)
                for n in LENGTHS:
                    for shift in SHIFTS:
                        got, lk = w.count4(how, w.text("holes", shift, n), opts)
                        check(got, lk, d.count("holes", n)[0], ("holes", n, shift))
                got, lk = w.count4(how, w.text("holes", 13), opts)
                check(got, lk, d.count("holes")[0], "holes")
                for kind, shift, rfull in (("soup", 0, 1), ("soup", 5, 0), ("high", 5, 1), ("high", 0, 0)):
                    got, lk = w.count4(how, w.text(kind, shift), {**opts, "gram_slab": 0, "gram2_rfull": rfull})
                    check(got, lk, d.count(kind)[0], (kind, shift, rfull))
                got, lk = w.count4(how, w.text("long", 5, LONG_TAIL), {**opts, "gram_region": 0})
                check(got, lk, d.count("long", LONG_TAIL)[0], "long")


@pytest.mark.parametrize("body", ["plain", "filt", "tail"])
def test_claimed_regions_on_a_32_bit_directory(body):
    """every region behind a wave's first claimed from the counter (tests/test_gpu_gram4_claims.py): 2 KiB regions, the split at 0, one 512-thread
    workgroup per CU, one and a half times as many regions as the launch has waves"""
    w = world("big20")
    nw = w.ncu * 8
    n = (3 * nw // 2) * 2048
    opts = {"threads": 512, "blocks_per_cu": 1, "gram_taper_split": 0, **{"plain": {"gram4_filter": 0}, "filt": {}, "tail": {"gram_tail": 1}}[body]}
    got, lk = w.count4("hash", w.text("long", 0, n), opts)
    assert got == w.d.count("long", n)[0], (body, lk, got)
    assert lk["dir"] == "2" and lk["waves"] == "8" and lk["filter"] == ("0" if body == "plain" else "1") and lk["tail"] == ("1" if body == "tail" else "0"), lk
    assert int(lk["regions"]) == 3 * nw // 2 and int(lk["claims"]) == nw // 2 > 0, lk


@pytest.mark.parametrize("body", ["plain", "filt", "tail"])
def test_big26_at_the_default_options(body):
    """M words and directory of the benchmark dictionary's size (78 736 + 19 684 bytes) with 32-bit entries: the shape the defaults give it — 32
    positions per lane, 16 waves, arithmetic classes, and beside the perfect hash's displacement table a Bloom array of 25 KiB"""
    w = world("big26")
    p = w.handles["hash"]
    for k in G4_BASE:
        p.set_option(k)   # (no override: the process-wide defaults)
    p.set_option("gram4_filter", 0 if body == "plain" else 1).set_option("gram_tail", 1 if body == "tail" else 0)
    want = {"ppl": "32", "dir": "2", "waves": "16", "arith": "1", "filter": "0" if body == "plain" else "1", "mph": "0" if body == "plain" else "1",
            "tail": "1" if body == "tail" else "0"}
    for kind in ("soup", "high", "holes"):
        got = p.count(OV, w.text(kind, 5), engine=Engine.Gram)
        lk = dict(kv.split("=") for kv in da.last_kernel().split()[1:])
        assert da.last_kernel().startswith("gram4 ") and {k: lk[k] for k in want} == want, (lk, w.lds_sum("hash", 32, 16, 1, body != "plain"))
        assert got == w.d.count(kind)[0], (body, kind, lk, got)
    p.set_option("gram_tail", -1)   # the probe on 1 MiB of uniform text
    assert p.count(OV, w.text("holes", 0), engine=Engine.Gram) == w.d.count("holes")[0] and " dir=2 " in da.last_kernel()


def _count2(w, hay, dense, threads, checksum, **kw):
    p = w.handles["hash"]
    p.set_option("gram_version", 2).set_option("gram_dense", dense).set_option("threads", threads).set_option("gram_region", 2048)
    got = p.scan_count(OV, hay, engine=Engine.Gram, **kw) if checksum else p.count(OV, hay, engine=Engine.Gram, **kw)
    # the instance that ran: 32-bit directory entries from 65 536 depth-4 states on (dir=2 is S16 = false)
    want = ["gram2", "K=3", "dir=2" if w.d.n_deep >= gu.THRESHOLD else "dir=1", f"dense={dense}", f"waves={threads // 64}", "region=2048"]
    assert da.last_engine() == int(Engine.Gram) and da.last_kernel().split()[:6] == want, (da.last_kernel(), want)
    return got


@pytest.mark.parametrize("dense", [0, 1])
@pytest.mark.parametrize("threads", [512, 1024])
def test_gram2_kernel_without_u16_entries(dense, threads):
    """gram2_kernel<3, S16 = false, DENSE, TPB>: `.count()` with gram_version = 2 and count + checksum on soup, high and holes, and a shard.  The
    handle is the one whose gram4 launches report dir=2: its three device table sets take s16 from the same host tables."""
    w = world("big20")
    got, lk = w.count4("hash", w.text("high", 0))
    assert lk["dir"] == "2" and got == w.d.count("high")[0]
    assert w.handles["hash"].info().gram2_exact
    for kind, shift in (("soup", 5), ("high", 0), ("holes", 13)):
        hay = w.text(kind, shift)
        assert _count2(w, hay, dense, threads, False) == w.d.count(kind)[0], (kind, "count")
        assert _count2(w, hay, dense, threads, True) == w.d.count(kind), (kind, "count + checksum")
    cut = 100_003
    assert _count2(w, w.text("high", 0), dense, threads, True, begin=cut) == w.d.count("high", None, cut)
    assert _count2(w, w.text("high", 0), dense, threads, False, begin=cut) == w.d.count("high", None, cut)[0]


def _emitter_lists(p, d, kind, n, dev):
    """every way to the tuple list of one text, all through the GRAM emitter (Engine.Gram: nothing else may serve)"""
    want = d.tuples(kind, n)
    assert len(want) > 10000
    got = p.scan(OV, dev, engine=Engine.Gram)
    assert da.last_engine() == int(Engine.Gram) and _same(got, want), (kind, "scan")
    dm = p.scan_device(OV, dev, engine=Engine.Gram)
    assert da.last_engine() == int(Engine.Gram) and dm.count == len(want) and _same(dm.to_numpy(), want), (kind, "scan_device")
    dm.free()
    d16 = p.scan_device(OV, dev, engine=Engine.Gram, fmt16=True)
    assert da.last_engine() == int(Engine.Gram) and _same16(d16.to_numpy(), want), (kind, "scan_device16")
    d16.free()
    return want


@pytest.mark.parametrize("kind", ["soup", "high", "holes"])
def test_tuple_emitter_without_u16_entries(kind):
    """emit3_detect_kernel<3, false>: the eager list, the list left on the device in both record formats, the lazy iterator over three windows
    and the stepper fed in chunks of 65 536, 3 and 4 096 bytes — the oracle's tuples, order included"""
    w = world("big20")
    p, d = w.handles["hash"], w.d
    n = gu.SOUP_BYTES
    dev = w.text(kind, 5, n)
    host = d.text(kind, n)
    p.set_option("gram_region", 0).set_option("threads", 1024)
    want = _emitter_lists(p, d, kind, n, dev)
    p.set_option("iter_window", 100_000)
    it = p.find_overlapping_iter(host, engine=Engine.Gram)
    runs = []
    while True:
        run = it.next_batch()
        if run is None:
            break
        runs.append(run.copy())
    it.close()
    p.set_option("iter_window")
    assert len(runs) >= 3 and _same16(np.concatenate(runs), want), (kind, "iterator", len(runs))
    assert da.last_engine() == int(Engine.Gram)
    st = p.find_overlapping_stepper()   # (a stepper is opened with Engine.Auto; every feed must still come back from the emitter)
    parts, at, k = [], 0, 0
    while at < n:
        size = (65536, 3, 4096)[k % 3]
        parts.append(st.feed(dev[at:at + size] if k % 2 else host[at:at + size]))
        assert da.last_engine() == int(Engine.Gram), (kind, "stepper", at, size, da.last_engine())
        at += size
        k += 1
    assert _same(np.concatenate([x for x in parts if len(x)]), want), (kind, "stepper")
    if kind == "high":   # the control path: the emitter switched off, the segment scanners write the same list
        p.set_option("emit", 0)
        got = p.scan(OV, dev)
        assert da.last_engine() != int(Engine.Gram) and _same(got, want)
        p.set_option("emit")
        p.scan(OV, dev[:4096])
        assert da.last_engine() == int(Engine.Gram)


@pytest.mark.parametrize("name", ["edge_lo", "edge_hi"])
def test_one_state_either_side_of_the_threshold(name):
    """65 535 states: u16 entries, the per-word directory (dir=0) or the coarse one (dir=1), the last entries just below 65 535; one word more:
    32-bit entries (dir=2) whatever is asked for.  One shape of each consumer, on the words of the last 1 000 prefixes and on holes."""
    w = world(name)
    d, p = w.d, w.handles["hash"]
    for rfull in (1, 0):
        for body_opts in ({}, {"gram4_filter": 0}, {"gram_tail": 1}):
            for kind, n in (("high", None), ("soup", None), ("holes", None), ("holes", 2049), ("holes", 33)):
                got, lk = w.count4("hash", w.text(kind, 5, n), {"gram2_rfull": rfull, **body_opts})
                assert lk["dir"] == ("2" if name == "edge_hi" else "0" if rfull else "1"), (name, rfull, lk)
                assert lk["ppl"] == "32" and lk["waves"] == "16" and lk["arith"] == "1" and lk["filter"] == str(body_opts.get("gram4_filter", 1)), lk
                assert got == d.count(kind, n)[0], (name, rfull, body_opts, kind, n, lk, got)
    for kind in ("high", "holes"):
        hay = w.text(kind, 5)
        assert _count2(w, hay, 0, 1024, True) == d.count(kind), (name, kind)
        assert _count2(w, hay, 1, 1024, False) == d.count(kind)[0], (name, kind)
    p.set_option("gram_region", 0)
    for kind in ("high", "holes"):
        _emitter_lists(p, d, kind, gu.SOUP_BYTES, w.text(kind, 5, gu.SOUP_BYTES))


def test_ledger_every_reachable_dir2_instance_ran():
    """the 24 gram4_kernel<3, .., DIR = 2, ..> instances x {tail 0, 1, auto}: all of them fit the LDS on big20 / big20s / big18 (the largest, 16
    waves at 32 positions per lane with a class table, sums to 41 472 + 256 + [9 264 | Bloom array] + 37 056 bytes with the Bloom array sized to
    what is left of 160 KiB), so all of them must have run — in the tests above (selected on its own, or in a process of its own, this test runs
    them itself first)"""
    if EXPECTED - LEDGER:
        for body, which in CASES:
            test_every_dir2_instance_of_gram4(body, which)
    missing = sorted(EXPECTED - LEDGER)
    print(f"gram4 DIR = 2 instances x bodies run: {len(LEDGER & EXPECTED)} of {len(EXPECTED)}")
    assert not missing, missing
    assert LEDGER <= EXPECTED, sorted(LEDGER - EXPECTED)
