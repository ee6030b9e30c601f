"""The perfect hash over gram4's depth-(K+1) states (gram4_mph.hpp, build_gram4_mph) on the CPU: tests/native/gram4_mph_check.cpp on cfg3,
cfg2, the dictionaries tests/test_gpu_gram4.py scans with and a few hundred small random ones — every key on a slot of its own, the record
there the one the key's rank names, the displacement table no larger than the coarse directory, two builds the same bytes, and 2 MB of
uniform cfg3 text walked through probe + hash giving the same pattern ends and go-ons as probe + rank."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from oracle import oracle as orc

from daachorse_amd import synth


@pytest.fixture(scope="module")
def mph_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("native") / "gram4_mph_check")
    csrc = os.path.join(ROOT, "daachorse_amd", "csrc")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "native", "gram4_mph_check.cpp"),
                           os.path.join(csrc, "pma.cpp"), os.path.join(csrc, "repack.cpp"), os.path.join(csrc, "gram2.cpp"), os.path.join(csrc, "gram4.cpp")])
    return exe


def _run(exe, tmp_path, pats, hay, budget=160000, *more):
    blob, h = tmp_path / "a.blob", tmp_path / "h.bin"
    blob.write_bytes(orc.OraclePma.build(pats).serialize())
    np.asarray(hay, dtype=np.uint8).tofile(h)
    out = subprocess.check_output([exe, str(blob), str(budget), str(h)] + [str(m) for m in more]).decode()
    assert out.startswith(("OK", "DECLINED", "UNAVAILABLE")), (out, pats[:3])
    return out


def _fields(out):
    return dict(kv.split("=") for kv in out.split()[1:])


def test_mph_cfg3_and_cfg2(mph_check, tmp_path):
    """the benchmark's dictionaries build within the retry bound, inside the directory's bytes; 2 MB of uniform cfg3 text: the same ends and go-ons"""
    out = _run(mph_check, tmp_path, synth.patterns_cfg3(), synth.uniform_haystack(2 << 20, synth.SEEDS["cfg3_hay"], synth.ALPHA_LOWER_SPACE))
    f = _fields(out)
    assert out.startswith("OK") and f["K"] == "3" and f["filter"] == "1", out
    assert int(f["buckets"]) <= int(f["s_bytes"]) and int(f["keys"]) <= int(f["slots"]) <= 2 * int(f["keys"]), out
    assert int(f["ends"]) > 0 and int(f["goons"]) > 0 and int(f["passed"]) < int(f["hits"]) // 2, out
    pats = synth.patterns_cfg3()
    out = _run(mph_check, tmp_path, pats, synth.wordsoup_haystack(200000, synth.SEEDS["cfg3_dense"], pats, 20))
    assert out.startswith("OK") and int(_fields(out)["goons"]) > 0, out   # (word soup: the walk must have met hits that go on)
    out = _run(mph_check, tmp_path, synth.patterns_cfg2(), synth.uniform_haystack(1 << 20, 6, synth.ALPHA_LOWER))
    assert out.startswith("OK"), out


def test_mph_dictionaries_of_the_gpu_suite(mph_check, tmp_path):
    rng = np.random.default_rng(303)
    pats3 = synth.patterns_cfg3(30000)
    gapped = sorted(set(bytes(rng.choice(np.frombuffer(b"acegikmoqsuwy", dtype=np.uint8), size=int(rng.integers(2, 9)))) for _ in range(3000)))
    high = sorted(set(bytes(rng.choice(np.arange(0xf0, 0x100, dtype=np.uint8), size=int(rng.integers(2, 7)))) for _ in range(2000)))
    syms = np.frombuffer(b"acinrs", dtype=np.uint8)
    six = [bytes(syms[rng.integers(0, 6, size=int(rng.integers(4, 9)))]) for _ in range(5000)]
    cases = [(synth.patterns_cfg1(), synth.uniform_haystack(70001, 5, synth.ALPHA_ABCD)),
             (synth.patterns_cfg2(500), synth.uniform_haystack(1 << 18, 6, synth.ALPHA_LOWER)),
             (pats3, synth.uniform_haystack(1 << 19, synth.SEEDS["cfg3_hay"], synth.ALPHA_LOWER_SPACE)),
             (pats3, synth.wordsoup_haystack(1 << 18, synth.SEEDS["cfg3_dense"], pats3, 20)),
             (synth.patterns_cfg3(5000), synth.wordsoup_haystack(1 << 18, 11, synth.patterns_cfg3(5000), 20)),
             (["ab", "ab", "b", "abab", "bababab"], np.frombuffer(b"abababbab" * 3000, dtype=np.uint8)),
             (gapped, rng.choice(np.frombuffer(b"abcdefghijklmnopqrstuvwxyz{ ", dtype=np.uint8), size=1 << 18)),
             (high, rng.choice(np.arange(0xe8, 0x100, dtype=np.uint8), size=1 << 18)),
             (six, np.frombuffer(b"".join(six[i] for i in rng.integers(0, 5000, size=20000).tolist()), dtype=np.uint8)),
             ([b"a" * k for k in range(1, 40)], np.frombuffer(b"a" * 10000 + b"b" + b"a" * 500, dtype=np.uint8))]
    for pats, hay in cases:
        for budget in (160000, 24 * 1024, 9216):
            out = _run(mph_check, tmp_path, pats, hay, budget)
            # With the table budget the upload has by default none of them is too dense for a byte a bucket (cfg1 at K = 3 holds no (K+1)-gram: nothing
            # to hash).  Squeezed to K = 2 the larger ones have twenty keys for every byte of their coarse directory: there the size condition says no
            # (the check has already made sure nothing was left behind) and the handle keeps the rank path.
            if budget == 160000:
                assert out.startswith("OK") or " keys=0 " in out, (out, pats[:3], budget)


def test_mph_random_small_dictionaries(mph_check, tmp_path):
    rng = np.random.default_rng(1010)
    ok = 0
    for i in range(300):
        nsym = int(rng.integers(2, 30))
        first = int(rng.integers(0, 256 - 2 * nsym))
        step = 1 if i % 3 else 2   # one byte range (arithmetic classes) / gapped (class table)
        syms = np.arange(first, first + step * nsym, step, dtype=np.uint8)
        pats = sorted(set(bytes(syms[rng.integers(0, nsym, size=int(rng.integers(1, 10)))]) for _ in range(int(rng.integers(1, 400)))))
        alpha = np.concatenate([syms, np.array([(first + step * nsym + 3) & 0xff, (first - 1) & 0xff], dtype=np.uint8)])
        out = _run(mph_check, tmp_path, pats, rng.choice(alpha, size=20000), (160000, 9216)[i % 2])
        ok += out.startswith("OK")
    assert ok >= 250, ok   # (a few hold no (K+1)-gram at all — nothing to hash — or have no room for the second table set)


def test_mph_declines_rather_than_shrinking_the_bloom_array(mph_check, tmp_path):
    """every 4-gram over twelve letters: 19 keys for every byte the coarse directory has — no displacement table of that size exists, the builder says
    no and leaves nothing behind; and a retry bound of 0 declines whatever the dictionary"""
    letters = b"abcdefghijkl"
    pats = [bytes([a, b, c, d]) for a in letters for b in letters for c in letters for d in letters]
    hay = np.random.default_rng(7).choice(np.frombuffer(letters + b" ", dtype=np.uint8), size=50000)
    assert _run(mph_check, tmp_path, pats, hay).startswith("DECLINED")
    assert _run(mph_check, tmp_path, synth.patterns_cfg2(300), hay, 160000, 0).startswith("DECLINED")
    assert _run(mph_check, tmp_path, synth.patterns_cfg2(300), hay, 160000, 1).startswith("OK")
