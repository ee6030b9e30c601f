"""Region claims of the gram4 `.count()` kernel (gram4_kernels.hip, round 14): a wave's first regions are its number in the launch plus whole
rounds of the launch's waves, every further one comes from a counter in the call's own scratch; the haystack's end is cut into small regions
(gram4_claims.hpp); the TAIL body asks for a region's first text where the region before it ends; the launch's last workgroup stores the result.
A launch has at most 16 (8 at 512 threads) waves per CU and never more waves than regions, and nothing is claimed where the haystack has no
tail, so a case reaches the counter only with a split (option gram_taper_split) and more regions than the launch has waves: 2 KiB regions
over 9 to 16 MiB, mostly at 512 threads.  daac_last_kernel() says how many regions a launch had and how many of them were claimed; every
case below asserts that number (CLAIMED cases: thousands).  Every expected count is the CPU oracle's; the region arithmetic alone is walked
on the CPU by tests/native/gram4_claims_check.cpp.

Not here: a scan that crosses a 2 GiB epoch (more than 2 GiB of text is no few-seconds test).  The suite's large scans (the 4 GiB haystacks of
test_gpu_configs.py, the walkers across 2 GiB / 4 GiB of test_gpu_gram4.py) and bench.py's own count check cover it, and the CPU check
shows that no region straddles an epoch."""
import re

import numpy as np
import pytest

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

import daachorse_amd as da
from daachorse_amd import Engine, ScanMode, synth

OV = ScanMode.FindOverlapping
TEXT = 16 * (1 << 20) + 8192
BASE = {"gram_version": 4, "gram_ppl": 32, "gram3_tail": -1, "gram4_filter": 1, "gram_region": 2048, "gram_region_small": 0, "gram_taper_split": -1,
        "threads": 1024, "blocks_per_cu": 1, "gram_slab": 4096}


class World:
    def __init__(self):
        import torch
        self.pats = synth.patterns_cfg3(5000)
        self.o = orc.OraclePma.build(self.pats)
        self.p, rest = da.DoubleArrayAhoCorasick.deserialize(self.o.serialize())
        assert rest == b""
        self.p.upload()
        self.ncu = torch.cuda.get_device_properties(0).multi_processor_count
        self.host = {"uniform": synth.uniform_haystack(TEXT, synth.SEEDS["cfg3_hay"], synth.ALPHA_LOWER_SPACE),
                     "soup": synth.wordsoup_haystack(TEXT, synth.SEEDS["cfg3_dense"], self.pats, 20)}
        # 16 spare bytes in front: a haystack may begin at any address mod 16
        self.dev = {}
        for k, h in self.host.items():
            buf = torch.zeros(TEXT + 32, dtype=torch.uint8, device="cuda")
            assert buf.data_ptr() % 16 == 0
            buf[16:16 + TEXT].copy_(torch.from_numpy(h))
            self.dev[k] = buf
        self.cache = {}

    def want(self, kind, lo, hi):
        """matches of text[lo:hi] as a haystack of its own (computed once per slice)"""
        key = (kind, lo, hi)
        if key not in self.cache:
            self.cache[key] = self.o.overlapping_count(self.host[kind][lo:hi], threads=4)[0] if hi > lo else 0
        return self.cache[key]

    def text(self, kind, lo, hi):
        return self.dev[kind][16 + lo:16 + hi]

    def count(self, hay, opts=None, **kw):
        for k, v in {**BASE, **(opts or {})}.items():
            self.p.set_option(k, v)
        got = self.p.count(OV, hay, engine=Engine.Gram, **kw)
        assert da.last_engine() == int(Engine.Gram) and da.last_kernel().startswith("gram4 "), da.last_kernel()
        self.regions, self.claims = self.launch()
        return got

    @staticmethod
    def launch():
        """(regions, regions claimed from the counter) of the calling thread's last gram4 launch; (0, 0): the call launched nothing"""
        m = re.search(r" regions=(\d+) claims=(\d+) ", da.last_kernel())
        return (int(m.group(1)), int(m.group(2))) if m else (0, 0)


@pytest.fixture(scope="module")
def w():
    return World()


# every region behind a wave's first is claimed: 2 KiB regions, the split at 0 (static_rounds = 1)
ALL_CLAIMED = {"gram_taper_split": 0}
T512 = {"threads": 512}


def test_region_counts_around_the_wave_count(w):
    """nregions = 1, nwaves - 1, nwaves, nwaves + 1 and 1.5 nwaves (one workgroup per CU, 16 waves each, 2 KiB regions), whole and ragged, every
    region behind a wave's first claimed — and the same lengths with no tail (nothing claimed: the ownership of before round 14).  Word soup
    at 32 positions per lane runs the TAIL body, whose text of a claimed region is asked for ahead."""
    nw = w.ncu * 16
    assert (3 * nw // 2) * 2048 <= TEXT
    for kind in ("uniform", "soup"):
        for nreg in (1, nw - 1, nw, nw + 1, 3 * nw // 2):
            for ragged in (0, 2048 - 5):
                n = nreg * 2048 - ragged
                assert w.count(w.text(kind, 0, n), ALL_CLAIMED) == w.want(kind, 0, n), (kind, nreg, ragged)
                assert (w.regions, w.claims) == (nreg, max(0, nreg - nw)), (nreg, w.regions, w.claims)
                assert w.count(w.text(kind, 0, n)) == w.want(kind, 0, n), (kind, nreg, ragged)
                assert (w.regions, w.claims) == (nreg, 0)
    # the TAIL body by option as well (the probe decides it on word soup of 1 MiB and more)
    n = (3 * nw // 2) * 2048 - 5
    assert w.count(w.text("soup", 0, n), {**ALL_CLAIMED, "gram3_tail": 1}) == w.want("soup", 0, n) and w.claims == nw // 2


def test_many_claims_and_a_ragged_last_region(w):
    """one static round, two claimed regions per wave and a claimed last region of 1 byte, 15 bytes, one step + 1 (16 positions per lane: a
    2 KiB region is two steps; 8 waves a workgroup)"""
    nw = w.ncu * 8
    for ppl, step in ((16, 1024), (32, 2048)):
        for kind in ("uniform", "soup"):
            for last in (1, 15, step + 1):
                region = 2 * step
                n = 3 * nw * region + last
                if n > TEXT:   # (32 positions per lane: 4 KiB regions, two rounds in all)
                    n = 2 * nw * region + last
                opts = {"gram_ppl": ppl, "gram_region": region, "gram_region_small": region, "gram_taper_split": nw * region, **T512}
                assert w.count(w.text(kind, 0, n), opts) == w.want(kind, 0, n), (ppl, kind, last)
                assert da.last_kernel().startswith(f"gram4 ppl={ppl} ") and "waves=8" in da.last_kernel(), da.last_kernel()
                assert w.regions == n // region + 1 and w.claims == w.regions - nw and w.claims > nw, (w.regions, w.claims)


def test_taper_split_points(w):
    """4 KiB regions with 2 KiB ones behind the split, 3 072 large regions' worth of text on 8 waves a workgroup: the split at 0 (all small),
    past the end and at the end (all large: nothing to claim), one large region before the end, in the first round, and behind one whole round"""
    large, nw = 4096, w.ncu * 8
    for kind in ("uniform", "soup"):
        for n in (3072 * large, 3072 * large - 2048 - 77):
            nl = (n + large - 1) // large
            assert nl > nw
            for split, claimed in ((0, True), (n + 5 * large, False), (nl * large, False), ((nl - 1) * large, True), (7 * large + 100, True), ((nw + 3) * large, True)):
                opts = {"gram_region": large, "gram_region_small": 2048, "gram_taper_split": split, **T512}
                assert w.count(w.text(kind, 0, n), opts) == w.want(kind, 0, n), (kind, n, split)
                assert (w.claims >= nl - nw) if claimed else (w.claims == 0 and w.regions == nl), (split, w.regions, w.claims)
    # the default tail (32 KiB behind 256 KiB and 64 KiB regions) is what the large scans of the suite and bench.py run


def test_range_scans_and_the_halo(w):
    """`begin` != 0 (13 bytes in: the halo reaches the haystack's start; 1 MiB + 13 in: a halo of its own), first byte at address 13 mod 16"""
    import torch
    n = 9 * (1 << 20) + 1000
    for kind in ("uniform", "soup"):
        buf = torch.zeros(n + 48, dtype=torch.uint8, device="cuda")
        hay = buf[13:13 + n]
        hay.copy_(w.text(kind, 0, n))
        assert hay.data_ptr() % 16 == 13
        for opts in ({**ALL_CLAIMED, **T512}, {"gram_region": 8192, "gram_region_small": 2048, "gram_taper_split": 100 * 8192, **T512}):
            assert w.count(hay, opts) == w.want(kind, 0, n) and w.claims > 1000, w.claims
            for begin in (13, (1 << 20) + 13):
                assert w.count(hay, opts, begin=begin) == w.want(kind, 0, n) - w.want(kind, 0, begin), (kind, begin, opts)
                assert w.claims > 1000, (begin, w.regions, w.claims)
            assert w.count(hay, opts, begin=n) == 0


def test_repeated_and_interleaved_calls(w):
    """one scan 20 times on a stream, then two scans interleaved on two streams with one handle, thousands of claims in each: a counter that is
    not cleared skips the regions behind a wave's first, one that two calls share loses regions of both"""
    import torch
    na, nb = 9 * (1 << 20) + 333, 8 * (1 << 20) + 2048 * 3 + 1
    a, b = w.text("uniform", 0, na), w.text("soup", 4096, 4096 + nb)
    wa, wb = w.want("uniform", 0, na), w.want("soup", 4096, 4096 + nb)
    for opts in ({**ALL_CLAIMED, **T512}, {"gram_region": 8192, "gram_region_small": 2048, "gram_taper_split": 200 * 8192, **T512}):
        assert w.count(a, opts) == wa and w.claims > 1000
        assert w.count(b, opts) == wb and w.claims > 1000
        res = torch.full((40, 3), -1, dtype=torch.int64, device="cuda")
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        for i in range(20):
            assert w.p.count(OV, a, engine=Engine.Gram, stream=s.cuda_stream, result_dev=res[i].data_ptr()) is None
        assert w.launch()[1] > 1000
        s.synchronize()
        assert res[:20].tolist() == [[wa, 0, 0]] * 20
        s2 = torch.cuda.Stream()
        res.fill_(-1)
        torch.cuda.synchronize()
        for i in range(20):
            w.p.count(OV, a, engine=Engine.Gram, stream=s.cuda_stream, result_dev=res[i].data_ptr())
            w.p.count(OV, b, engine=Engine.Gram, stream=s2.cuda_stream, result_dev=res[20 + i].data_ptr())
        s.synchronize()
        s2.synchronize()
        assert res.tolist() == [[wa, 0, 0]] * 20 + [[wb, 0, 0]] * 20


def test_hits_only_at_one_end(w):
    """text without a hit but for its first region (a wave's own) / its last, ragged, claimed region (the drain at the end of a wave's claims)"""
    import torch
    large, n = 8192, 700 * 8192 + 2048 + 700
    soup = torch.from_numpy(w.host["soup"][:2048].copy()).cuda()
    piece = w.want("soup", 0, 2048)
    assert piece > 100
    for where in ("first", "last"):
        hay = torch.full((n,), ord(" "), dtype=torch.uint8, device="cuda")
        at = 0 if where == "first" else n - 2048
        hay[at:at + 2048] = soup
        for opts in ({**ALL_CLAIMED, **T512}, {"gram_region": large, "gram_region_small": 2048, "gram_taper_split": 100 * large, **T512}):
            assert w.count(hay, opts) == piece, (where, opts)
            assert w.claims > 400 and w.regions - w.claims == w.ncu * 8, (w.regions, w.claims)   # (the last region's index is beyond the waves)


def test_empty_and_tiny_haystacks(w):
    import torch
    res = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    for opts in (ALL_CLAIMED, {"gram_region": 8192, "gram_region_small": 2048, "gram_taper_split": 0}):
        assert w.count(w.text("soup", 0, 0), opts) == 0
        res.fill_(-1)
        w.p.count(OV, w.text("soup", 0, 0), engine=Engine.Gram, result_dev=res.data_ptr())
        torch.cuda.synchronize()
        assert res.tolist() == [0, 0, 0]
        for n in (1, 5, 100, 1000, 2047):
            assert w.count(w.text("soup", 0, n), opts) == w.want("soup", 0, n), n
            assert (w.regions, w.claims) == (1, 0)
            res.fill_(-1)
            w.p.count(OV, w.text("soup", 0, n), engine=Engine.Gram, result_dev=res.data_ptr())
            torch.cuda.synchronize()
            assert res.tolist() == [w.want("soup", 0, n), 0, 0], n
