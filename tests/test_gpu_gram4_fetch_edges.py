"""The seam between the two text fetches of the gram4 `.count()` kernel (gram4_kernels.hip, round 9): an interior step loads its chunks from a
scalar base with no per-lane bounds work, the first step of a scan, the last one or two and a step that reaches past its region's end go
through the patching loader.  Haystacks of k steps + d bytes around every such border, every alignment class of the first byte (`lead` != 0),
shards (`begin` > 0), regions of one and two steps and the default, a pattern that ends with the haystack's last byte and one that starts in
the last whole step and ends in the ragged one — counted by all three bodies, the oracle alone decides what is expected."""
import numpy as np
import pytest

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

import daachorse_amd as da
from daachorse_amd import Engine, ScanMode, synth

# (tail records, filter): the body with the LDS filter (what AUTO runs on uniform text), the TAIL body (word soup), the plain one
BODIES = [(0, 1), (1, 1), (0, 0)]
REGIONS = [2048, 4096, 0]   # the smallest two the launcher accepts (one / two steps of 32 positions per lane) and the default
ALIGN = [0, 1, 7, 15]       # address of the first byte mod 16


def _count4(p, hay, ppl, tail, filt, region, **kw):
    for k, v in (("gram_version", 4), ("gram_ppl", ppl), ("gram3_tail", tail), ("gram4_filter", filt), ("gram_region", region)):
        p.set_option(k, v)
    got = p.count(ScanMode.FindOverlapping, hay, engine=Engine.Gram, **kw)
    assert da.last_engine() == int(Engine.Gram)
    lk = da.last_kernel()
    assert lk.startswith(f"gram4 ppl={ppl} "), lk
    return got


def _lengths(step):
    return [k * step + d for k in (0, 1, 2, 3, 64) for d in (0, 1, 15, 16, 17, step - 17, step - 16, step - 1)]


@pytest.mark.parametrize("ppl", [16, 32])
def test_gram4_fetch_edges(ppl):
    import torch
    step = 64 * ppl
    pats = synth.patterns_cfg3(5000)
    longest = np.frombuffer(max(pats, key=len), dtype=np.uint8)
    assert 12 <= len(longest) < step - 17
    o = orc.OraclePma.build(pats)
    p, rest = da.DoubleArrayAhoCorasick.deserialize(o.serialize())
    assert rest == b""
    p.upload()
    soup = synth.wordsoup_haystack(66 * 2048, 23, pats, 20)
    rng = np.random.default_rng(909 + ppl)
    checked = 0
    for n in _lengths(step):
        for al in ALIGN:
            # the haystack: word soup from a random offset; its last bytes are a pattern that ends with the haystack; the longest
            # pattern lies across the last step border of the virtual positions (index + al), three bytes before it and the rest behind
            start = int(rng.integers(0, 2048))
            h = soup[start:start + n].copy()
            w = np.frombuffer(pats[int(rng.integers(0, len(pats)))], dtype=np.uint8)
            if n >= len(w):
                h[n - len(w):] = w
            border = ((n + al) // step) * step - al
            if border - 3 >= 0 and border - 3 + len(longest) <= n:
                h[border - 3:border - 3 + len(longest)] = longest
            buf = torch.zeros(n + 32, dtype=torch.uint8, device="cuda")
            assert buf.data_ptr() % 16 == 0
            dev = buf[al:al + n]
            dev.copy_(torch.from_numpy(h))
            want = o.overlapping_count(h, threads=1)[0] if n else 0
            begins = [0] + [b for b in (37, step + 5) if b < n]
            wants = {b: want - (o.overlapping_count(h[:b], threads=1)[0] if b else 0) for b in begins}
            if n >= len(w):
                assert want >= 1
            for region in REGIONS:
                for tail, filt in BODIES:
                    for b in begins:
                        got = _count4(p, dev, ppl, tail, filt, region, begin=b) if b else _count4(p, dev, ppl, tail, filt, region)
                        assert got == wants[b], (n, al, region, tail, filt, b, got, wants[b])
                        checked += 1
    assert checked >= len(_lengths(step)) * len(ALIGN) * len(REGIONS) * len(BODIES)
