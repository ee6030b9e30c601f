"""The gram4 `.count()` kernel's hit queue (a wave prefix sum places every lane's hits in the wave's list; a step with more hits than
the list holds runs the scan again on the rest) against the oracle: uniform text and word soup across region boundaries, text in
which every position hits (several passes per step), haystack lengths that are not a multiple of a step."""
import numpy as np
import pytest

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

import daachorse_amd as da
from daachorse_amd import Engine, ScanMode, synth

# (positions per lane, tail records (-1: the workgroups' own probe), filter, threads per workgroup)
SHAPES = [(32, -1, 1, 1024), (32, 0, 1, 1024), (32, 1, 1, 1024), (32, 0, 0, 1024), (16, 0, 1, 1024), (16, 1, 0, 512)]


def _pma(patterns):
    o = orc.OraclePma.build(patterns)
    p, rest = da.DoubleArrayAhoCorasick.deserialize(o.serialize())
    assert rest == b""
    p.upload()
    return o, p


def _count(p, dev, ppl, tail, filt, threads, region=0):
    for k, v in (("gram_version", 4), ("gram_ppl", ppl), ("gram3_tail", tail), ("gram4_filter", filt), ("threads", threads),
                 ("gram_region", region)):
        p.set_option(k, v)
    got = p.count(ScanMode.FindOverlapping, dev, engine=Engine.Gram)
    assert da.last_engine() == int(Engine.Gram)
    assert da.last_kernel().startswith(f"gram4 ppl={ppl} "), da.last_kernel()
    return got


@pytest.fixture(scope="module")
def cfg3():
    pats = synth.patterns_cfg3(30000)
    return (pats,) + _pma(pats)


def test_producer_uniform_and_word_soup_across_regions(cfg3):
    import torch
    pats, o, p = cfg3
    for hay in (synth.uniform_haystack((3 << 20) + 4099, synth.SEEDS["cfg3_hay"], synth.ALPHA_LOWER_SPACE),
                synth.wordsoup_haystack((3 << 20) + 4099, synth.SEEDS["cfg3_dense"], pats, 20)):
        want = o.overlapping_count(hay, threads=8)[0]
        dev = torch.from_numpy(hay).cuda()
        for shape in SHAPES:
            for region in (0, 8192):   # the automatic region (64 / 256 KiB) and many small ones: the queue is flushed at every boundary
                assert _count(p, dev, *shape, region=region) == want, (shape, region)


def test_producer_every_position_hits():
    """every 4-gram of the text starts a pattern of 8+ bytes: 2 048 hits per step and lane group, several list passes per step"""
    import torch
    rng = np.random.default_rng(505)
    base = synth.patterns_cfg3(5000)
    rot = [b"abcd"[i:] + b"abcd"[:i] for i in range(4)]
    pats = base + [r * 2 for r in rot] + [r * 3 + r[:1] for r in rot] + [r[:3] for r in rot]
    o, p = _pma(pats)
    rep = np.frombuffer(b"abcd" * ((1 << 20) // 4), dtype=np.uint8)
    mixed = rep.copy()
    for at in rng.integers(0, len(mixed) - 64, size=200).tolist():   # a few stretches of word soup between the dense text
        mixed[at:at + 40] = np.frombuffer(b"".join(base[int(i)] + b" " for i in rng.integers(0, len(base), size=8))[:40], dtype=np.uint8)
    for hay in (rep, mixed, rep[: (1 << 19) + 1234]):
        want = o.overlapping_count(hay, threads=8)[0]
        dev = torch.from_numpy(np.ascontiguousarray(hay)).cuda()
        for shape in SHAPES:
            assert _count(p, dev, *shape) == want, (len(hay), shape)


def test_producer_lengths_off_the_step(cfg3):
    """haystack lengths that are not a multiple of a step (2 KiB at 32 positions per lane, 1 KiB at 16), first byte unaligned"""
    import torch
    pats, o, p = cfg3
    soup = synth.wordsoup_haystack(1 << 17, 17, pats, 20)
    uni = synth.uniform_haystack(1 << 17, 18, synth.ALPHA_LOWER_SPACE)
    buf = torch.from_numpy(np.concatenate([np.zeros(3, dtype=np.uint8), soup, uni])).cuda()
    for n in (1, 31, 1000, 2047, 2049, 3333, 6143, 65535 + 2048, 100001):
        for start in (3, 3 + (1 << 17) - n // 2):
            hay = buf[start:start + n]
            want = o.overlapping_count(hay.cpu().numpy(), threads=4)[0]
            for shape in ((32, 0, 1, 1024), (32, 1, 1, 1024), (16, 0, 0, 512)):
                assert _count(p, hay, *shape, region=4096) == want, (n, start, shape)
