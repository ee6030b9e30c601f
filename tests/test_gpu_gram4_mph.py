"""gram4's FILT body with a survivor's record fetched by perfect hash (gram4_mph.hpp, round 10) against the rank path (option gram4_mph = 0,
read at upload) and the oracle: cfg3 on uniform text and word soup (64 MiB), cfg2, a dictionary whose byte classes are not arithmetic, and a
dictionary too dense for a displacement table the size of its coarse directory — that handle runs the rank path and daac_last_kernel() says so."""
import numpy as np
import pytest

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

import daachorse_amd as da
from daachorse_amd import Engine, ScanMode, synth


def _handles(pats):
    """the same dictionary twice: with the hash (the default) and with records by rank"""
    o = orc.OraclePma.build(pats)
    out = []
    for mph in (8, 0):
        p, _ = da.DoubleArrayAhoCorasick.deserialize(o.serialize())
        p.set_option("gram4_mph", mph)   # (read when the tables are laid out)
        assert p.upload().info().gram2_available
        out.append(p)
    return o, out[0], out[1]


def _count(p, hay, **opts):
    for k, v in {"gram_version": 4, "gram_ppl": 0, "gram3_tail": -1, "gram2_rfull": 1, "threads": 1024, "gram4_arith": 1, "gram4_filter": 1, **opts}.items():
        p.set_option(k, v)
    got = p.count(ScanMode.FindOverlapping, hay, engine=Engine.Gram)
    lk = da.last_kernel()
    assert da.last_engine() == int(Engine.Gram) and lk.startswith("gram4 "), lk
    return got, dict(kv.split("=") for kv in lk.split()[1:])


SHAPES = [{}, {"gram_ppl": 16}, {"gram3_tail": 0}, {"gram3_tail": 1}, {"gram2_rfull": 0}, {"threads": 512}, {"gram4_arith": 0}, {"gram_ppl": 16, "threads": 512, "gram2_rfull": 0}]


def _check(pats, hay, want_mph):
    import torch
    o, with_hash, by_rank = _handles(pats)
    want = o.overlapping_count(hay if isinstance(hay, np.ndarray) else hay.cpu().numpy(), threads=8)[0]
    dev = hay if not isinstance(hay, np.ndarray) else torch.from_numpy(np.concatenate([np.zeros(3, dtype=np.uint8), hay])).cuda()[3:]
    for shape in SHAPES:
        got, lk = _count(with_hash, dev, **shape)
        assert got == want, (shape, lk, got, want)
        if want_mph is not None:
            assert lk["mph"] == ("1" if want_mph and lk["filter"] == "1" else "0"), (shape, lk)
        got, lk = _count(by_rank, dev, **shape)
        assert got == want and lk["mph"] == "0", (shape, lk, got, want)
    got, lk = _count(with_hash, dev, gram4_filter=0)
    assert got == want and lk["filter"] == "0" and lk["mph"] == "0", lk
    return _count(with_hash, dev)[1]


def test_mph_cfg3_uniform_and_word_soup():
    import torch
    pats = synth.patterns_cfg3()
    dev = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")
    synth.device_uniform(dev, synth.SEEDS["cfg3_hay"], synth.ALPHA_LOWER_SPACE)
    lk = _check(pats, dev, True)
    assert lk["filter"] == "1" and lk["mph"] == "1", lk   # the flagship shape runs the hash
    synth.device_wordsoup(dev, synth.SEEDS["cfg3_dense"], pats, 20, noise_256=77)
    _check(pats, dev, True)


def test_mph_cfg2_and_class_table_dictionary():
    rng = np.random.default_rng(77)
    _check(synth.patterns_cfg2(), synth.uniform_haystack(8 << 20, 6, synth.ALPHA_LOWER), True)
    gapped = sorted(set(bytes(rng.choice(np.frombuffer(b"acegikmoqsuwy", dtype=np.uint8), size=int(rng.integers(2, 9)))) for _ in range(3000)))
    lk = _check(gapped, rng.choice(np.frombuffer(b"abcdefghijklmnopqrstuvwxyz{ ", dtype=np.uint8), size=4 << 20), True)
    assert lk["arith"] == "0", lk
    high = sorted(set(bytes(rng.choice(np.arange(0xf0, 0x100, dtype=np.uint8), size=int(rng.integers(2, 7)))) for _ in range(2000)))
    _check(high, rng.choice(np.arange(0xe8, 0x100, dtype=np.uint8), size=4 << 20), True)
    # K = 2 (a small table budget), every position a hit that goes on
    syms = np.frombuffer(b"acinrs", dtype=np.uint8)
    six = [bytes(syms[rng.integers(0, 6, size=int(rng.integers(4, 9)))]) for _ in range(5000)]
    _check(six, np.frombuffer(b"".join(six[i] for i in rng.integers(0, 5000, size=60_000).tolist())[:300_000], dtype=np.uint8).copy(), None)


def test_mph_builder_declines_and_the_handle_ranks():
    """every 4-gram over twelve letters: no displacement table within the coarse directory's bytes — the handle keeps the rank path, says mph=0, counts right"""
    letters = b"abcdefghijkl"
    pats = [bytes([a, b, c, d]) for a in letters for b in letters for c in letters for d in letters]
    hay = np.random.default_rng(7).choice(np.frombuffer(letters + b" ", dtype=np.uint8), size=4 << 20)
    _check(pats, hay, False)
