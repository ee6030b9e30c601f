"""Token ids back to text (daac_decoder_create, daac_tokens_decode, Decoder and its builders) on the host side: the exports, every answer
the C ABI and the Python wrappers give before they touch a device, in the header's order, the three builders on hand cases, the
pure-Python definition (tests/decode_golden.py) against the fixture of tests/golden/ that `tokenizers` produced, the fixture's maker,
and the kernels' per-lane bodies run on the CPU under ASan and UBSan (tests/native/decode_check.cpp, a stand-alone program).  No GPU."""
import ctypes as C
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import decode_golden as dg

import daachorse_amd as da
from daachorse_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _err():
    return _ffi.lib().daac_last_error().decode()


class _Call:
    """the raw arguments of daac_tokens_decode over host arrays that no refused call reads; the names in `null` go as NULL"""

    def __init__(self, dec, csr=True, width=4, n=2, tokens=4, row_length=0):
        self.dec, self.csr, self.width, self.n, self.tokens, self.row_length = dec, csr, width, n, tokens, row_length
        self.buf = np.zeros(16, dtype=np.uint64)
        self.null = set()
        self.outs = {k: C.c_void_p() for k in ("out", "out_offsets", "token_starts")}
        self.bytes = C.c_uint64()

    def run(self):
        p = self.buf.ctypes.data
        arg = lambda name, v=None: None if name in self.null else (p if v is None else v)
        out = lambda name: None if name in self.null else C.byref(self.outs[name])
        return _ffi.lib().daac_tokens_decode(arg("dec", self.dec._h), arg("ids"), self.width, arg("offsets") if self.csr else None, self.tokens, self.n,
                                             self.row_length, 1, 0, None, out("out"), out("out_offsets"), out("token_starts"), arg("bytes", C.byref(self.bytes)))


def _create(pool, pieces, flags, n_ids=None, pool_bytes=None, null=()):
    pool_a = np.frombuffer(pool or b"\0", dtype=np.uint8)
    pc = np.ascontiguousarray(pieces, dtype=np.uint32).reshape(-1, 4)
    fl = np.ascontiguousarray(flags, dtype=np.uint8)
    h = C.c_void_p(7)
    st = _ffi.lib().daac_decoder_create(None if "pool" in null else pool_a.ctypes.data, len(pool) if pool_bytes is None else pool_bytes,
                                        None if "pieces" in null else pc.ctypes.data, None if "flags" in null else fl.ctypes.data,
                                        len(fl) if n_ids is None else n_ids, None if "out" in null else C.byref(h))
    if st == 0:
        _ffi.lib().daac_decoder_free(h)
    return st, h.value


def test_decode_symbols_are_exported():
    lib = C.CDLL(_ffi._build.LIB_PATH)
    for name in ("daac_decoder_create", "daac_decoder_free", "daac_tokens_decode"):
        assert hasattr(lib, name), name
    assert callable(da.Decoder) and "Decoder" in da.__all__
    for name in ("byte_level", "wordpiece", "metaspace", "decode_batch", "decode", "free"):
        assert callable(getattr(da.Decoder, name)), name
    assert _ffi.lib().daac_abi_version() == 6 == _ffi.ABI_VERSION
    with open(os.path.join(ROOT, "include", "daachorse_amd.h"), encoding="utf-8") as f:
        header = f.read()
    for name in ("daac_decoder_create", "daac_decoder_free", "daac_tokens_decode", "daac_decode_piece", "DAAC_DECODE_SPECIAL", "DAAC_DECODE_ABSENT"):
        assert name in header, name
    import importlib
    build = importlib.import_module("daachorse_amd._build")
    assert {"api_decode.hip", "decode_kernels.hip"} <= set(build.SOURCES) and "decode.hpp" in build.HEADERS


def test_create_refusals_without_a_device():
    ok = ([[0, 1, 0, 1], [1, 2, 0, 1]], [0, 1])
    assert _create(b"abc", *ok)[0] == 0
    st, h = _create(b"abc", *ok, null={"out"})
    assert st == 1 and "null" in _err()
    for null in ("pool", "pieces", "flags"):
        st, h = _create(b"abc", *ok, null={null})
        assert st == 1 and "NULL" in _err() and h is None, null
    assert _create(b"", [], [], null={"pool", "pieces", "flags"})[0] == 0   # nothing to read: no id has an entry
    st, _ = _create(b"abc", *ok, pool_bytes=1 << 32)
    assert st == 1 and "below 4 GiB" in _err()
    st, _ = _create(b"abc", *ok, n_ids=(1 << 32) + 1)
    assert st == 1 and "32 bits" in _err()
    st, _ = _create(b"abc", ok[0], [0, 4])
    assert st == 1 and "id 1: flags" in _err()
    for bad in ([3, 1, 0, 0], [0, 0, 2, 2], [0xFFFFFFFF, 2, 0, 0]):
        st, _ = _create(b"abc", [[0, 1, 0, 1], bad], [0, 0])
        assert st == 1 and "id 1: an image leaves the pool" in _err(), bad
    assert _create(b"abc", [[3, 0, 0, 3]], [3])[0] == 0   # an empty image at the pool's end, both flags


def test_decode_refusals_in_the_stated_order_without_a_device():
    dec = da.Decoder(["a", "bc"])
    # 1. null arguments, in front of everything else
    for name in ("dec", "out", "out_offsets", "bytes", "ids"):
        c = _Call(dec, width=3)
        c.null.add(name)
        assert c.run() == 1 and "null" in _err(), name
    c = _Call(dec, csr=False, width=3, row_length=4)
    c.null.add("ids")
    assert c.run() == 1 and "null" in _err()
    # 2. the width, in front of 3. a plane without a row length
    assert _Call(dec, width=3).run() == 1 and "id_width is 3" in _err()
    assert _Call(dec, csr=False, width=2).run() == 1 and "id_width is 2" in _err()
    assert _Call(dec, width=8).run() == 1 and "CSR" in _err()
    c = _Call(dec, csr=False, width=8)
    assert c.run() == 1 and "row_length" in _err()
    # 4. max_result_bytes: the offsets, a plane's tokens, the token starts
    da.set_option("max_result_bytes", 16)
    try:
        assert _Call(dec, n=2).run() == 2 and "out_offsets" in _err()
        assert _Call(dec, csr=False, n=2).run() == 1 and "row_length" in _err()   # behind 3.
        assert _Call(dec, csr=False, n=1, row_length=3).run() == 2 and "plane" in _err()
        assert _Call(dec, n=1, tokens=2).run() == 2 and "token_starts" in _err()
    finally:
        da.set_option("max_result_bytes", 8 << 30)
    # every refused call leaves what it was given
    c = _Call(dec, width=3)
    c.outs["out"].value, c.outs["out_offsets"].value, c.bytes.value = 5, 6, 7
    assert c.run() == 1 and (c.outs["out"].value, c.outs["out_offsets"].value, c.bytes.value) == (5, 6, 7)


def test_refusals_through_the_wrappers():
    for call, what in ((lambda: da.Decoder({-1: "a"}), "id -1"), (lambda: da.Decoder(["a"], first={3: "b"}), "no rest image"), (lambda: da.Decoder(["a"], special=["a"]), "special"),
                       (lambda: da.Decoder.byte_level({b"a": 0, b"b": 0}), "comes twice"), (lambda: da.Decoder.byte_level([b"a"], gap_id=-1), "gap_id"),
                       (lambda: da.Decoder.metaspace(["a"], prepend_scheme="last"), "prepend_scheme"), (lambda: da.Decoder.metaspace(["a"], first="some"), "strip_one"),
                       (lambda: da.Decoder(["a"], special=da.SpecialTokens(da.DoubleArrayAhoCorasick.new([b"a"]))), "no texts")):
        with pytest.raises(da.DaachorseError) as ei:
            call()
        assert ei.value.code == 1 and what in str(ei.value), what
    dec = da.Decoder(["a", None, "bc"], special=[2, 5])
    assert dec.n_ids == 6 and dec.special == {2, 5} and sorted(dec.rest) == [0, 2] and dec.pool_bytes == 3
    for tokens, what in ((np.zeros(3, dtype=np.int64), "two-dimensional"), (np.zeros((2, 2), dtype=np.float32), "int32 / uint32 / int64"),
                         ((1, 2, 3, 4), "(ids, offsets)"), (([0.5], [0, 1]), "integers"), (([-1], [0, 1]), "integers"), (([0], [-1, 1]), "non-negative"), ("ab", "plane")):
        with pytest.raises(da.DaachorseError) as ei:
            dec.decode_batch(tokens)
        assert ei.value.code == 1 and what in str(ei.value), tokens
    with pytest.raises(da.DaachorseError) as ei:
        dec.decode_batch(np.zeros((1, 1), dtype=np.int32), unknown="drop")
    assert ei.value.code == 1 and '"error" or "skip"' in str(ei.value)
    dec.free()
    with pytest.raises(da.DaachorseError) as ei:
        dec.decode_batch(np.zeros((1, 1), dtype=np.int32))
    assert ei.value.code == 1 and "freed" in str(ei.value)


# ------------------------------------------------------------------------------------------ the builders, the definition and the fixture
def _table_of(dec):
    return dec.rest, {i: dec.first.get(i, dec.rest[i]) for i in dec.rest}, set(dec.special)


def test_the_builders_on_hand_cases():
    wp = ["hello", "##s", ",", "world", "'", "s", "do", "not", "##", "[CLS]"]
    dec = da.Decoder.wordpiece({p: i for i, p in enumerate(wp)}, special=[9])
    t = _table_of(dec)
    assert dg.decode(t, [0, 1, 2, 3, 4, 5]) == b"hellos, world ' s"
    assert dg.decode(t, [1, 0]) == b"##s hello" and dg.decode(t, [9, 1, 0]) == b"##s hello" and dg.decode(t, [9, 1, 0], skip_special=False) == b"[CLS]s hello"
    assert dg.decode(t, [6, 7]) == b"do not" and dg.decode(t, [0, 8]) == b"hello" and dg.decode(t, [8]) == b"##" and dg.decode(t, []) == b""
    assert _table_of(da.Decoder.wordpiece({" do not": 0, "x .": 1, "n't": 2}))[0] == {0: b"  don't", 1: b" x.", 2: b"n't"}
    assert _table_of(da.Decoder.wordpiece({" do not": 0, "n't": 1}, cleanup=False))[0] == {0: b"  do not", 1: b" n't"}
    assert _table_of(da.Decoder.wordpiece({"@@a": 0, "a": 1}, prefix="@@"))[0] == {0: b"a", 1: b" a"}
    ms = ["▁hello", "▁wor", "ld", "▁", "▁▁a▁b", "<0x41>", "<s>"]
    for scheme in ("always", "first"):
        t = _table_of(da.Decoder.metaspace(ms, prepend_scheme=scheme, special=[6]))
        assert dg.decode(t, [0, 1, 2, 3]) == b"hello world " and dg.decode(t, [6, 3, 0]) == b" hello" and dg.decode(t, [4, 4]) == b"ab  a b"
        assert dg.decode(t, [5]) == b"<0x41>"
    t = _table_of(da.Decoder.metaspace(ms, prepend_scheme="never"))
    assert dg.decode(t, [0, 1, 2, 3]) == b" hello world "
    t = _table_of(da.Decoder.metaspace(ms, byte_fallback=True))
    assert dg.decode(t, [4, 5, 4]) == b" a bA  a b" and dg.decode(t, [0, 1, 2, 3]) == b"hello world "
    assert _table_of(da.Decoder.metaspace(ms, first="strip_one"))[1][4] == b" a b" and _table_of(da.Decoder.metaspace(ms, byte_fallback=True, first="drop_all"))[1][4] == b"ab"
    assert _table_of(da.Decoder.metaspace(["_a", "<0x4a>", "<0xZZ>", "<0x20>"], replacement="_", byte_fallback=True))[1] == {0: b"a", 1: b"J", 2: b"<0xZZ>", 3: b""}
    bl = da.Decoder.byte_level([b"ab", b"\xe2\x82"], gap_id=2, special=da.SpecialTokens({"<|e|>": 300}))
    t = _table_of(bl)
    assert bl.n_ids == 301 and t[2] == {300} and dg.decode(t, [0, 1, 2 + 0xAC, 300, 2]) == b"ab\xe2\x82\xac\x00"
    assert dg.decode(t, [300, 0], skip_special=False) == b"<|e|>ab"
    with pytest.raises(dg.DecodeError) as ei:
        dg.decode(t, [0, 299, 280])
    assert ei.value.token == 1 and dg.decode(t, [0, 299, -100, 1 << 32, 1], unknown="skip") == b"ab\xe2\x82"
    assert dg.decode_batch(t, [[0, 300], [], [1, 2]])[1] == [0, 2, 2, 4, 5]
    # the library's builders give the definition's tables for the fixture's four tokenizers
    for name in dg.NAMES:
        assert _table_of(dg.library_decoder(name)) == dg.table(name), name


def test_the_definition_agrees_with_the_fixture():
    cases = dg.cases()
    lossy = sum(c[3] for c in cases)
    assert len(cases) >= 60 and 2 <= lossy <= 0.10 * len(cases) and {c[0] for c in cases} == set(dg.NAMES)
    assert any(not c[1] for c in cases) and sum(c[2][True] != c[2][False] for c in cases) >= 20
    for name, ids, text, is_lossy in cases:
        for skip in (True, False):
            got = dg.decode(dg.table(name), ids, skip_special=skip)
            if is_lossy:
                assert "�" in text[skip] and got != text[skip].encode() and got.decode("utf-8", "replace").replace("�", "") == text[skip].replace("�", "")
            else:
                assert got == text[skip].encode(), (name, ids, skip)
    pipe = dg.load()["bert_pipeline"]
    assert len(pipe["text"]) == len(__import__("normalize_golden").docs()) and pipe["row_length"] == 16


def test_the_maker_reproduces_the_fixture():
    if importlib.util.find_spec("tokenizers") is None:
        pytest.skip("the maker needs `tokenizers`")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_decode_golden.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("checked "), (r.stdout[-2000:], r.stderr[-2000:])
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "decode_cases.json")) < 64 * 1024


# ---------------------------------------------------------------------------------------------- the lane bodies under sanitizers
def _exe(tmp_path):
    exe = str(tmp_path / "decode_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-o", exe, os.path.join(ROOT, "tests", "native", "decode_check.cpp")])
    return exe


def _hex(b):
    return b.hex() or "-"


def test_decode_lane_bodies_on_the_host_under_sanitizers(tmp_path):
    """the sizing, header and copy bodies of decode_kernels.hip as plain C++: every case of the fixture as a CSR batch and as dense planes
    padded on the right and on the left, in both widths and for both values of skip_special, against the definition (and, where the
    case is not lossy, `tokenizers`' recorded text); unknown ids and their error; then 2 x 3000 random and hostile rounds against a
    sequential restatement"""
    exe = _exe(tmp_path)
    for name in dg.NAMES:
        rest, first, special = dg.table(name)
        n_ids = max(rest) + 1
        lines = [f"T {n_ids}"] + [f"{int(i in special)} {_hex(rest[i])} {_hex(first[i])}" if i in rest else "2 - -" for i in range(n_ids)]
        mine = [c for c in dg.cases() if c[0] == name]
        docs, pad = [c[1] for c in mine], dg.pad_id(name)
        batches = []
        for skip in (True, False):
            for form, width in (("csr", 4), ("right", 4), ("right", 8), ("left", 4), ("left", 8)):
                rows = docs if form == "csr" else dg.padded(docs, pad, left=form == "left")
                batches.append((skip, form, rows))
                lines.append(f"C {width} {int(form != 'csr')} {int(skip)} 0 {len(rows[0]) if form != 'csr' else 0} {len(rows)}")
                lines += [" ".join(["D", str(len(r))] + [str(i) for i in r]) for r in rows]
        # ids without an entry: refused at the lowest, left out with unknown_skip; -100 and 2^32 in an 8-byte plane
        bad = [docs[0] + [n_ids + 3], [-100] + docs[1], docs[2] + [1 << 32]]
        bad_rows = dg.padded(bad, pad)
        lines.append(f"C 8 1 1 0 {len(bad_rows[0])} 3")
        lines += [" ".join(["D", str(len(r))] + [str(i) for i in r]) for r in bad_rows]
        lines.append(f"C 8 1 1 1 {len(bad_rows[0])} 3")
        lines += [" ".join(["D", str(len(r))] + [str(i) for i in r]) for r in bad_rows]
        path = tmp_path / f"{name}.txt"
        path.write_text("\n".join(lines) + "\n")
        r = subprocess.run([exe, "batch", str(path)], capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", (r.stdout[-2000:], r.stderr[-2000:])
        out = r.stdout.split("\n")[:-1]
        assert len(out) == 3 * len(batches) + 1 + 3
        for k, (skip, form, rows) in enumerate(batches):
            texts, starts = dg.decode_batch(dg.table(name), rows, skip_special=skip)
            o, f, s = out[3 * k:3 * k + 3]
            assert o == "O " + _hex(b"".join(texts)), (name, skip, form)
            assert [int(x) for x in f.split()[1:]] == np.cumsum([0] + [len(t) for t in texts]).tolist(), (name, skip, form)
            assert [int(x) for x in s.split()[1:]] == starts, (name, skip, form)
            if skip:
                for c, t in zip(mine, texts):
                    assert c[3] or t == c[2][True].encode(), (name, form, c[1])
        assert out[3 * len(batches)] == f"U {len(docs[0])}"
        texts, starts = dg.decode_batch(dg.table(name), bad_rows, unknown="skip")
        assert out[3 * len(batches) + 1] == "O " + _hex(b"".join(texts)) and [int(x) for x in out[-1].split()[1:]] == starts
    for seed in (1, 2):
        r = subprocess.run([exe, "random", "3000", str(seed)], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.startswith("OK 3000 rounds") and r.stderr == "", (r.stdout, r.stderr)
