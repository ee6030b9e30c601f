"""Special tokens in raw text (daac_cut_batch / daac_tokens_splice, SpecialTokens, splice_special) on the host side: the exports, every
answer the C ABI and the Python wrappers give before they touch a device, in the header's order, the fixture of tests/golden/ against
the pure-Python definition (tests/special_golden.py) with the CPU oracle's leftmost_find_iter as the scan, the fixture's maker, and the
kernels' per-lane bodies run on the CPU under ASan and UBSan (tests/native/cut_check.cpp, a stand-alone program).  No GPU."""
import ctypes as C
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as orc
import normalize_golden as ng
import special_golden as sg
import wordpiece_golden as wg
from test_split_host import scan_batch as split_scan

import daachorse_amd as da
from daachorse_amd import Split, _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LL = orc.LEFTMOST_LONGEST


def _pma(patterns, values=None, kind=LL, charwise=False):
    o = (orc.OracleCharwisePma if charwise else orc.OraclePma).build(patterns, values=values, kind=kind)
    p, rest = (da.CharwiseDoubleArrayAhoCorasick if charwise else da.DoubleArrayAhoCorasick).deserialize(o.serialize())
    assert rest == b""
    return p


def _err():
    return _ffi.lib().daac_last_error().decode()


class _Cut:
    """the raw arguments of daac_cut_batch; the pointers named in `null` go as NULL"""

    def __init__(self, p, hay=b"a<|x|>b", offsets=(0, 3, 7)):
        self.h = p._h if p is not None else None
        self.hay = np.frombuffer(hay, dtype=np.uint8)
        self.offsets = None if offsets is None else np.asarray(offsets, dtype=np.uint64)
        self.n = 0 if offsets is None else len(offsets) - 1
        self.so, self.ds, self.sv, self.n_segs, self.n_special = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint64()
        self.null = set()

    def run(self, engine=0):
        ptr = lambda a: None if a is None else a.ctypes.data
        ref = lambda name, v: None if name in self.null else C.byref(v)
        return _ffi.lib().daac_cut_batch(self.h, int(engine), ptr(self.hay), ptr(self.offsets), self.n, 0, None, ref("so", self.so), ref("ds", self.ds),
                                         ref("sv", self.sv), ref("n_segs", self.n_segs), ref("n_special", self.n_special))


def test_special_symbols_are_exported():
    lib = C.CDLL(_ffi._build.LIB_PATH)
    for name in ("daac_cut_batch", "daac_tokens_splice"):
        assert hasattr(lib, name), name
    assert callable(da.SpecialTokens) and callable(da.splice_special) and callable(da.SpecialTokens.cut_batch)
    assert "SpecialTokens" in da.__all__ and "splice_special" in da.__all__
    assert _ffi.lib().daac_abi_version() == 6 == _ffi.ABI_VERSION


def test_cut_refusals_in_the_stated_order_without_a_device():
    good = _pma(["<|x|>"], [7])
    standard = _pma(["<|x|>"], [7], kind=orc.STANDARD)
    with_empty = _pma(["<|x|>", ""], [7, 8])
    with_text_value = _pma(["<|x|>", "y"], [7, 0xFFFFFFFF])
    empty_and_value = _pma(["", "y"], [7, 0xFFFFFFFF])
    # 1. a NULL out-pointer or handle: in front of everything else, broken offsets and a Standard handle included
    for name in ("so", "ds", "sv", "n_segs", "n_special"):
        c = _Cut(standard, offsets=(0, 3, 2))
        c.null.add(name)
        assert c.run() == 1 and "null" in _err(), name
    assert _Cut(None).run() == 1 and "null" in _err()
    # 2. the batch offset rules, in front of the match kind
    assert _Cut(standard, offsets=(0, 3, 2)).run() == 1 and "document 1" in _err()
    c = _Cut(standard)
    c.offsets = None
    assert c.run() == 1 and "offsets" in _err()
    c = _Cut(standard)
    c.hay = None
    assert c.run() == 1 and "hay" in _err()
    # 3. a Standard automaton: 5, in front of the patterns' own faults
    assert _Cut(standard).run() == 5 and "leftmost" in _err()
    assert _Cut(_pma(["", "y"], [7, 0xFFFFFFFF], kind=orc.STANDARD)).run() == 5
    # 4. "" among the patterns, in front of 5. the value of a text segment
    assert _Cut(with_empty).run() == 1 and "empty pattern" in _err()
    assert _Cut(empty_and_value).run() == 1 and "empty pattern" in _err()
    assert _Cut(with_text_value).run() == 1 and "0xFFFFFFFF" in _err()
    # 6. max_result_bytes, by the rule of split_batch's lists: 8 bytes a document
    da.set_option("max_result_bytes", 16)
    try:
        assert _Cut(with_text_value).run() == 1
        assert _Cut(good).run() == 2 and "max_result_bytes" in _err()
        good.set_option("max_result_bytes", 1 << 20)   # the handle's own value is the one that counts
        assert _Cut(good).run() in (0, 7)
        good.set_option("max_result_bytes")
    finally:
        da.set_option("max_result_bytes", 8 << 30)
    # the scan's own refusals are this call's: the engines that serve no batch, and TIERED for a leftmost scan (with documents the
    # tuple call answers behind the upload, so a machine without a device says 7 first: n = 0 here)
    for engine in (da.Engine.Gram, da.Engine.Pfx, da.Engine.Tiered):
        assert _Cut(good, offsets=None).run(engine) == 6, engine
    # the charwise handle passes the same checks
    assert _Cut(_pma(["<|x|>"], [7], kind=orc.STANDARD, charwise=True)).run() == 5
    assert _Cut(_pma(["<|x|>", "é"], [7, 0xFFFFFFFF], charwise=True)).run() == 1 and "0xFFFFFFFF" in _err()
    # n = 0 passes every check, NULL hay and offsets included: what is left is the device (0 with one, 7 without)
    c = _Cut(good, offsets=None)
    c.hay = None
    st = c.run()
    assert st in (0, 7), (st, _err())
    if st == 0:
        assert (c.n_segs.value, c.n_special.value, c.sv.value) == (0, 0, None)
        for p in (c.so, c.ds):
            out = np.ones(1, dtype=np.uint64)
            assert _ffi.lib().daac_device_to_host(out.ctypes.data, p, 8) == 0 and out[0] == 0
            _ffi.lib().daac_device_free(p)


def test_cut_refusals_through_the_wrappers():
    def raised(special, docs=(b"a<|x", b"|>b"), **kw):
        with pytest.raises(da.DaachorseError) as ei:
            special.cut_batch(list(docs), **kw)
        return ei.value.code, str(ei.value)

    assert raised(da.SpecialTokens(_pma(["<|x|>"], [7], kind=orc.STANDARD)))[0] == 5
    code, msg = raised(da.SpecialTokens(_pma(["<|x|>", ""], [7, 8])))
    assert code == 1 and "empty pattern" in msg
    code, msg = raised(da.SpecialTokens(_pma(["<|x|>"], [0xFFFFFFFF])))
    assert code == 1 and "0xFFFFFFFF" in msg
    assert raised(da.SpecialTokens({"<|x|>": 7}), docs=(), engine=da.Engine.Gram)[0] == 6
    # tokenize_*_docs take None or a SpecialTokens (the documents are uploaded first: with a device only)
    assert da.SpecialTokens({"<|x|>": 7}).pma.match_kind() == da.MatchKind.LeftmostLongest


def test_splice_refusals_without_a_device():
    L = _ffi.lib()
    a = np.zeros(4, dtype=np.uint64)
    p = a.ctypes.data   # (never read: every call below is refused before a device is touched)
    oi, osp, dt, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64()
    outs = (C.byref(oi), C.byref(osp), C.byref(dt), C.byref(n))
    args = [p, p, p, p, p, p, p]   # ids, spans, seg_tok, seg_values, seg_offsets, doc_segs, doc_offsets
    for k in (2, 3, 4, 5, 6):
        bad = list(args)
        bad[k] = None
        assert L.daac_tokens_splice(*bad, 1, 1, None, *outs) == 1 and "null" in _err(), k
    for k in (0, 2, 3):
        bad = list(outs)
        bad[k] = None
        assert L.daac_tokens_splice(*args, 1, 1, None, *bad) == 1 and "null" in _err(), k
    assert L.daac_tokens_splice(*args, 1, 0, None, *outs) == 1 and "without a document" in _err()
    da.set_option("max_result_bytes", 16)
    try:
        assert L.daac_tokens_splice(*args, 1, 2, None, *outs) == 2 and "max_result_bytes" in _err()
    finally:
        da.set_option("max_result_bytes", 8 << 30)
    with pytest.raises(da.DaachorseError) as ei:
        da.splice_special(None, None, None, (1, 2), [b"a"])
    assert ei.value.code == 1 and "cut_batch" in str(ei.value)


def test_special_tokens_own_refusals():
    for bad, what in (({"": 1}, "empty"), ([("a", 1), (b"a", 2)], "twice"), ({"a": 0xFFFFFFFF}, "0xFFFFFFFE"), ({"a": -1}, "0xFFFFFFFE"), ([(b"", 0)], "empty")):
        with pytest.raises(da.DaachorseError) as ei:
            da.SpecialTokens(bad)
        assert ei.value.code == 1 and what in str(ei.value), bad
    s = da.SpecialTokens([("<|a|>", 5), (b"<|a|><|b|>", 0xFFFFFFFE), ("é", 0)])
    assert s.tokens == {b"<|a|>": 5, b"<|a|><|b|>": 0xFFFFFFFE, "é".encode(): 0}
    assert s.pma.match_kind() == da.MatchKind.LeftmostLongest
    out = {(int(v), int(n)) for v, n, _ in s.pma.outputs().tolist()}
    assert out == {(5, 5), (0xFFFFFFFE, 10), (0, 2)}
    with pytest.raises(da.DaachorseError) as ei:
        da.bytewise._special_docs(None, "<|a|>", False, None, None)   # what tokenize_*_docs(special="<|a|>") reaches behind the upload
    assert ei.value.code == 1 and "SpecialTokens" in str(ei.value)


# ------------------------------------------------------------------------------------------ the fixture against the definition
def _oracle_scan(spec):
    o = orc.OraclePma.build([t for t, _ in spec], values=[i for _, i in spec], kind=LL)
    return lambda d: [(int(s), int(e), int(v)) for s, e, v, _ in o.leftmost_find_iter(d).tolist()]


def test_hand_cases_of_the_definition():
    spec = [(b"<|a|>", 50), (b"<|a|><|b|>", 51), (b"the", 52)]
    scan = _oracle_scan(spec)
    for d in (b"", b"<|a|><|b|>", b"x<|a|><|c|>", b"other", b"<|endoftext", b"<|a|><|a|>", b"xx<|a|>"):
        assert scan(d) == sg.leftmost(d, spec), d
    so, ds, sv = sg.cut([b"", b"<|a|><|b|>", b"x<|a|><|c|>", b"", b"other", b"ab"], scan, base=3)
    assert so.tolist() == [3, 13, 14, 19, 24, 25, 28, 29, 31]
    assert ds.tolist() == [0, 0, 1, 4, 4, 7, 8]
    assert sv.tolist() == [51, sg.TEXT, 50, sg.TEXT, sg.TEXT, 52, sg.TEXT, sg.TEXT]
    # a special's garbage tokens are dropped, spans count from the document
    ids, spans, dt = sg.splice([9, 9, 1, 2, 9, 3], [(0, 1)] * 6, [0, 2, 4, 5, 6, 6, 6, 6, 6], sv, so, ds, [3, 3, 13, 24, 24, 29, 31])
    assert ids.tolist() == [51, 1, 2, 50, 3, 52] and dt.tolist() == [0, 0, 1, 5, 5, 6, 6]
    assert spans.tolist() == [[0, 10], [0, 1], [0, 1], [1, 6], [6, 7], [1, 4]]


def test_fixture_against_the_definition_with_the_oracle_as_the_scan():
    case = sg.load()
    docs = sg.docs()
    assert len(docs) >= 300 and docs.count(b"") >= 2
    # ---- byte-level BPE: the GPT-2 split and a rank merge on every text segment
    with open(os.path.join(ROOT, "tests", "golden", "tokenizer_bpe_vocab.json"), encoding="utf-8") as f:
        pieces = [bytes.fromhex(h) for h in json.load(f)["pieces_hex"]]
    rank_of = {p: i for i, p in enumerate(pieces)}
    cc = da.char_classes()

    def bpe_text(seg):
        wo, _ = split_scan([seg], Split.Gpt2, cc)
        ids, spans, pos = [], [], 0
        for a, b in zip(wo.tolist(), wo.tolist()[1:]):
            for i in _rank_merge(seg[a:b], rank_of):
                ids.append(i)
                spans.append((pos, pos + len(pieces[i])))
                pos += len(pieces[i])
        return ids, spans

    spec = sg.specials("bpe")
    got = sg.tokenize_docs(docs, _oracle_scan(spec), bpe_text)
    want_spans = sg.bpe_spans([len(p) for p in pieces], {i: len(t) for t, i in spec})
    for d, (ids, spans), want, ws in zip(docs, got, case["bpe_ids"], want_spans):
        assert ids == want and spans == ws, d
    # ---- BERT: the normalizer, Split.Bert and WordPiece on every text segment, spans back to the raw segment
    vocab, unk_id, max_chars, prefix = wg.model()
    table = wg.class_table(da.bert_char_classes())

    def wp_text(seg):
        out, src = ng.bert_scan(seg, ng.OPTIONS["default"])
        ids, spans = wg.wordpiece_doc(out, table, vocab, unk_id, max_chars, prefix.encode())
        return ids, ng.spans_to_source(spans, src, seg)

    got = sg.tokenize_docs(docs, _oracle_scan(sg.specials("wordpiece")), wp_text)
    for d, (ids, spans), want, ws in zip(docs, got, case["wordpiece_ids"], sg.wordpiece_spans()):
        assert ids == want and spans == [tuple(x) for x in ws], d


def _rank_merge(word, rank_of):
    """tiktoken's byte_pair_merge: the neighbouring pair whose bytes have the lowest rank is merged, ties to the left"""
    b = list(range(len(word) + 1))
    while True:
        best, at = None, None
        for i in range(len(b) - 2):
            r = rank_of.get(word[b[i]:b[i + 2]])
            if r is not None and (best is None or r < best):
                best, at = r, i
        if at is None:
            break
        del b[at + 1]
    return [rank_of[word[s:e]] for s, e in zip(b, b[1:])]


def test_the_maker_reproduces_the_fixture():
    if importlib.util.find_spec("tokenizers") is None or importlib.util.find_spec("regex") is None:
        pytest.skip("the maker needs `tokenizers` and `regex`")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_special_golden.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("checked "), (r.stdout[-2000:], r.stderr[-2000:])


# ---------------------------------------------------------------------------------------------- the lane bodies under sanitizers
def _exe(tmp_path):
    exe = str(tmp_path / "cut_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-o", exe, os.path.join(ROOT, "tests", "native", "cut_check.cpp")])
    return exe


def test_cut_and_splice_lane_bodies_on_the_host_under_sanitizers(tmp_path):
    """the count and write bodies of cut_kernels.hip as plain C++: the fixture's documents as one batch with offsets[0] = 5 against the
    definition, for both lists of specials; then 2 x 3000 rounds of random and hostile batches, the splice included"""
    exe = _exe(tmp_path)
    docs = sg.docs()
    for which in ("bpe", "wordpiece"):
        scan = _oracle_scan(sg.specials(which))
        lines = ["B 5"] + [" ".join(["D", str(len(d))] + [f"{s} {e} {v}" for s, e, v in scan(d)]) for d in docs]
        path = tmp_path / f"{which}.txt"
        path.write_text("\n".join(lines) + "\n")
        r = subprocess.run([exe, "batch", str(path)], capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", (r.stdout[-2000:], r.stderr[-2000:])
        got = {ln[0]: [int(x) for x in ln.split()[1:]] for ln in r.stdout.split("\n")[:-1]}
        so, ds, sv = sg.cut(docs, scan, base=5)
        assert (got["O"], got["S"], got["V"]) == (so.tolist(), ds.tolist(), sv.tolist()), which
    for seed in (1, 2):
        r = subprocess.run([exe, "random", "3000", str(seed)], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.startswith("OK 3000 rounds") and r.stderr == "", (r.stdout, r.stderr)
