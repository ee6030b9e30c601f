"""The tier layouts tests/test_gpu_tier_layouts.py names (tests/tier_layouts.py) exist: each (dictionary, options) pair goes through
build_tier_tables on the CPU (tests/native/repack_check.cpp), which prints the N / NA / NB / row32 it gave and walks the host tables
with TierEngine::step's rule over the device test's own texts, byte by byte against the reference's transition function."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from oracle import oracle as orc

import tier_layouts as tl


@pytest.fixture(scope="module")
def repack_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("native") / "repack_check")
    csrc = os.path.join(ROOT, "daachorse_amd", "csrc")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "native", "repack_check.cpp"),
                           os.path.join(csrc, "pma.cpp"), os.path.join(csrc, "repack.cpp")])
    return exe


def _run(exe, blob, hay, opts):
    args = [exe, str(blob), str(opts.get("lds_budget", tl.DEFAULT_BUDGET)), str(opts.get("dense_depth", -1)), str(hay)]
    if "rows_share_pct" in opts:
        args.append(str(opts["rows_share_pct"]))
    return subprocess.check_output(args).decode()


def _fields(out):
    assert out.startswith("OK "), out
    return {k: int(v) for k, v in (kv.split("=") for kv in out.split()[2:])}


@pytest.fixture(scope="module")
def w_files(tmp_path_factory):
    """the three dictionaries' blobs and one file of all the device test's texts, one after the other"""
    d = tmp_path_factory.mktemp("w")
    texts = tl.w_texts()
    hay = d / "texts.bin"
    np.concatenate([texts[k] for k in sorted(texts)]).tofile(hay)
    blobs = {}
    for name in ("W", "W_lo", "W_hi"):
        pats = tl.w_patterns(name)
        o = orc.OraclePma.build(pats)
        blobs[name] = d / f"{name}.blob"
        blobs[name].write_bytes(o.serialize())
        assert len(o.outputs()) == len(pats)
    return blobs, hay


def test_w_is_what_the_layouts_assume():
    words = tl.w_words()
    assert len(words) == len(set(words)) == 31713 and len(tl.ALPHABET) == len(set(tl.ALPHABET)) == 31 and tl.OTHER not in tl.ALPHABET
    prefixes = {w[:i] for w in words for i in range(5)}
    assert len(prefixes) == 32801 and all(p in prefixes for p in tl.PREFIXES)            # the extra patterns add no state
    for name, n in (("W", 32801), ("W_lo", 32767), ("W_hi", 32768)):
        assert tl.trie_shape(tl.w_patterns(name)) == (n, 32, 32), name
    lo, hi = tl.extreme_words()
    for name in ("W", "W_lo", "W_hi"):                                                    # both survive the cut of the last words
        pats = tl.w_patterns(name)
        assert lo in pats and hi in pats and b"aaaa" in pats, name


@pytest.mark.parametrize("layout", [l[0] for l in tl.W_LAYOUTS])
def test_w_layouts(repack_check, w_files, layout):
    blobs, hay = w_files
    _, dname, opts, shape = next(l for l in tl.W_LAYOUTS if l[0] == layout)
    out = _run(repack_check, blobs[dname], hay, opts)
    if shape is None:
        assert out.startswith("UNAVAILABLE"), out
        return
    f = _fields(out)
    print(layout, out.strip())
    assert {k: f[k] for k in shape} == shape and f["C"] == 32, out
    assert f["lds"] <= opts.get("lds_budget", tl.DEFAULT_BUDGET), out
    if layout == "rows16_edge":
        assert f["N"] - 1 == 32766 and f["row32"] == 0   # a row of depth 3 names every state: the largest id takes all 15 bits beside the flag


@pytest.mark.parametrize("layout", tl.TINY_LAYOUTS)
def test_tiny_layouts(repack_check, tmp_path, layout):
    blob, hay = tmp_path / "a.blob", tmp_path / "h.bin"
    seen = set()
    for pats, text, opts, shape in tl.tiny_cases(layout):
        blob.write_bytes(orc.OraclePma.build(pats).serialize())
        text.tofile(hay)
        f = _fields(_run(repack_check, blob, hay, opts))
        assert {k: f[k] for k in shape} == shape and f["C"] == tl.trie_shape(pats)[2], (pats, opts, f)
        assert f["lds"] <= opts["lds_budget"], (pats, opts, f)
        seen.add("a" if f["NB"] == f["NA"] else "b" if f["NB"] < f["N"] else "ab")
    # the trials of a layout reach what it is there for
    want = {"root_c": {"a"}, "root_half": {"b"}, "root_all": {"ab"}, "depth1_half": {"b"}}[layout]
    assert want <= seen, (layout, seen)
    with_empty = sum(1 for pats, _, _, _ in tl.tiny_cases(layout) if b"" in pats)
    with_copies = sum(1 for pats, _, _, _ in tl.tiny_cases(layout) if len(set(pats)) < len(pats))
    assert with_empty >= 5 and with_copies >= 5, (with_empty, with_copies)
