"""Model inputs (daac_tokens_pack, Packer, bert_template / roberta_template and pack= on tokenize_*_docs) on the host side: the exports,
every answer the C ABI and the Python wrappers give before they touch a device, in the header's order, the pure-Python definition
(tests/pack_golden.py) against the fixture of tests/golden/ that `tokenizers` produced, the fixture's maker, and the kernels' per-lane
bodies run on the CPU under ASan and UBSan (tests/native/pack_check.cpp, a stand-alone program).  No GPU."""
import ctypes as C
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import pack_golden as pg

import daachorse_amd as da
from daachorse_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BERT = da.bert_template(101, 102)


def _err():
    return _ffi.lib().daac_last_error().decode()


class _Call:
    """the raw arguments of daac_tokens_pack over host arrays that no refused call reads; the names in `null` go as NULL"""

    def __init__(self, packer=None, pair=False, n=2, tokens=4, **kw):
        self.params = (packer or da.Packer(BERT, **kw)).params
        self.buf = np.zeros(16, dtype=np.uint64)
        self.pair, self.n, self.tokens = pair, n, tokens
        self.null = set()
        self.outs = {k: C.c_void_p() for k in ("input_ids", "type_ids", "attention", "special", "offsets", "row_offsets")}
        self.L, self.slots = C.c_uint64(), C.c_uint64()

    def run(self):
        p = self.buf.ctypes.data
        arg = lambda name, v=None: None if name in self.null else (p if v is None else v)
        out = lambda name: None if name in self.null else C.byref(self.outs[name])
        b = (lambda name: arg(name)) if self.pair else (lambda name: None)
        return _ffi.lib().daac_tokens_pack(arg("params", C.byref(self.params)), arg("a_ids"), arg("a_spans"), arg("a_offsets"), self.tokens,
                                           b("b_ids"), b("b_spans"), b("b_offsets"), self.tokens if self.pair else 0, self.n, None,
                                           out("input_ids"), out("type_ids"), out("attention"), out("special"), out("offsets"), out("row_offsets"),
                                           arg("L", C.byref(self.L)), arg("slots", C.byref(self.slots)))


def test_pack_symbols_are_exported():
    lib = C.CDLL(_ffi._build.LIB_PATH)
    assert hasattr(lib, "daac_tokens_pack")
    for name in ("Packer", "bert_template", "roberta_template"):
        assert callable(getattr(da, name)) and name in da.__all__, name
    assert callable(da.Packer.pack)
    assert _ffi.lib().daac_abi_version() == 6 == _ffi.ABI_VERSION
    assert C.sizeof(_ffi.PackParams) == 456 and _ffi.PackParams.max_length.offset == 432   # the header's layout
    single, pair = da.roberta_template(0, 2)
    assert single == [("special", 0, 0), ("A", 0, 0), ("special", 2, 0)] and [p[0] for p in pair] == ["special", "A", "special", "special", "B", "special"]
    single, pair = BERT
    assert pair == [("special", 101, 0), ("A", 0, 0), ("special", 102, 0), ("B", 0, 1), ("special", 102, 1)] and single == pair[:3]


def test_refusals_in_the_stated_order_without_a_device():
    broken = dict(single=[("A", 0, 0), ("A", 0, 0)])   # what every later refusal stands behind
    # 1. null arguments, in front of everything else
    for name in ("params", "input_ids", "L", "slots", "a_offsets", "a_ids"):
        c = _Call(da.Packer(**broken, dtype=np.int16))
        c.null.add(name)
        assert c.run() == 1 and "null" in _err(), name
    c = _Call(da.Packer(**broken), pair=True)
    c.null.add("b_ids")
    assert c.run() == 1 and "null" in _err()
    c = _Call(da.Packer(BERT), tokens=0, n=0)   # no token, no document: neither list is needed
    c.null |= {"a_ids", "a_spans", "a_offsets", "type_ids", "attention", "special", "offsets", "row_offsets"}
    assert c.run() == 0 and (c.L.value, c.slots.value, c.outs["input_ids"].value) == (0, 0, None)
    assert _ffi.last_kernel() == "pack docs=0 pair=0 row=0 tokens=0 dropped=0"
    # 2. the struct's size
    p = da.Packer(**broken, dtype=np.int16)
    p.params.struct_size -= 8
    assert _Call(p).run() == 1 and "struct_size" in _err()
    # 3. the templates
    for kw, what in ((dict(single=[("special", 1, 0)] * 16 + [("A", 0, 0)]), "at most 16"), (dict(single=[("special", 1, 0)]), "sequence A 0 times"),
                     (broken, "sequence A 2 times"), (dict(single=[("A", 0, 0), ("B", 0, 0)]), "sequence B 1 times: never"),
                     (dict(single=[("A", 0, 0)], pair=[("A", 0, 0)]), "pair template holds sequence B 0 times"),
                     (dict(single=[("A", 0, 0)], pair=[("A", 0, 0), ("B", 0, 0), ("B", 0, 1)]), "sequence B 2 times")):
        if len(kw["single"]) > 16:
            with pytest.raises(da.DaachorseError) as ei:
                da.Packer(**kw)
            assert ei.value.code == 1 and what in str(ei.value)
            p = da.Packer(dtype=np.int16)
            p.params.n_single = 17
        else:
            p = da.Packer(**kw, dtype=np.int16)
        assert _Call(p).run() == 1 and what in _err(), kw
    p = da.Packer(dtype=np.int16)
    p.params.single[0].kind = 3
    assert _Call(p).run() == 1 and "no such kind" in _err()
    assert _Call(da.Packer(dtype=np.int16), pair=True).run() == 1 and "without a pair template" in _err()
    # 4. the width, in front of 5. the enums and the multiple
    p = da.Packer(BERT, dtype=np.int16, pad_to_multiple_of=0)
    assert _Call(p).run() == 1 and "width is 2" in _err()
    assert _Call(da.Packer(BERT, dtype=np.float32, pad_to_multiple_of=0)).run() == 1 and "width is 0" in _err()
    p = da.Packer(BERT, pad_to_multiple_of=0, max_length=1, strategy="only_second")
    assert _Call(p).run() == 1 and "pad_multiple is 0" in _err()
    p.params.padding = 3
    assert _Call(p).run() == 1 and "no such padding" in _err()
    p.params.strategy = 3
    assert _Call(p).run() == 1 and "no such truncation strategy" in _err()
    # 6. only_second without B, in front of 7. max_length below the template's special tokens
    p = da.Packer(BERT, max_length=1, strategy="only_second", padding=None)
    assert _Call(p).run() == 1 and "only_second" in _err()
    c = _Call(da.Packer(BERT, max_length=2, strategy="only_second", padding=None), pair=True)
    assert c.run() == 1 and "max_length 2 is below the template's 3 special tokens" in _err()
    c = _Call(da.Packer(BERT, max_length=1, padding=None))
    c.null.add("row_offsets")
    assert c.run() == 1 and "max_length 1 is below the template's 2 special tokens" in _err()
    # 8. the CSR form has row offsets, in front of 9. offsets want spans
    c = _Call(da.Packer(BERT, max_length=2, padding=None))
    c.null |= {"row_offsets", "a_spans"}
    assert c.run() == 1 and "row offsets" in _err()
    c = _Call(da.Packer(BERT, max_length=2, padding=None))
    c.null.add("a_spans")
    assert c.run() == 1 and "no spans" in _err()
    c = _Call(da.Packer(BERT), pair=True)
    c.null.add("b_spans")
    assert c.run() == 1 and "no spans" in _err()
    # 10. max_result_bytes, for the row offsets: 8 bytes a document
    da.set_option("max_result_bytes", 16)
    try:
        assert _Call(da.Packer(BERT, padding=None), n=2).run() == 2 and "max_result_bytes" in _err()
        assert _Call(da.Packer(BERT, padding=None, dtype=np.int16), n=2).run() == 1
    finally:
        da.set_option("max_result_bytes", 8 << 30)
    # every refused call leaves what it was given
    c = _Call(da.Packer(**broken))
    c.outs["input_ids"].value = 5
    assert c.run() == 1 and c.outs["input_ids"].value == 5


def test_refusals_through_the_wrappers():
    for kw, what in ((dict(strategy="shortest"), "longest_first"), (dict(padding_side="up"), "left or right"), (dict(padding="max_length"), "longest"),
                     (dict(max_length=-1), "max_length"), (dict(pad_id=1 << 32), "pad_id"), (dict(single=[("C", 0, 0)]), "kind 'C'"),
                     (dict(pad_to_multiple_of=-8), "pad_to_multiple_of")):
        with pytest.raises(da.DaachorseError) as ei:
            da.Packer(**kw)
        assert ei.value.code == 1 and what in str(ei.value), kw
    p = da.Packer(BERT)
    for seq, what in ((np.zeros(3, dtype=np.uint32), "(ids, offsets)"), ((1, 2, 3, 4), "(ids, offsets)")):
        with pytest.raises(da.DaachorseError) as ei:
            p.pack(seq)
        assert ei.value.code == 1 and what in str(ei.value)
    assert p.params.n_single == 3 and p.params.n_pair == 5 and not p.csr and da.Packer(padding=None).csr
    assert (da.Packer(padding=32).params.padding, da.Packer(padding=32).params.pad_length) == (2, 32)
    # pack= is None or a Packer: answered before the documents are uploaded
    pma = da.DoubleArrayAhoCorasick.new([b"a"])
    for call in (lambda: pma.tokenize_bpe_docs([b"a"], pack="bert"), lambda: pma.tokenize_wordpiece_docs([b"a"], [0], [0], 0, pack=BERT)):
        with pytest.raises(da.DaachorseError) as ei:
            call()
        assert ei.value.code == 1 and "Packer" in str(ei.value)


# ------------------------------------------------------------------------------------------ the definition and the fixture
def test_hand_cases_of_the_definition():
    t = pg.truncate
    assert t(5, 9, True, 0, "only_first") == (0, 0) and t(5, 0, False, 3, "longest_first") == (3, 0) and t(3, 4, True, 7, "only_second") == (3, 4)
    assert t(3, 100, True, 10, "longest_first") == (3, 7) and t(100, 3, True, 10, "longest_first") == (7, 3)   # only the longer is cut
    assert t(9, 8, True, 11, "longest_first") == (6, 5) and t(8, 9, True, 11, "longest_first") == (5, 6)       # halved, the odd one to the longer
    assert t(8, 8, True, 11, "longest_first") == (5, 6) and t(20, 12, True, 10, "longest_first") == (5, 5)
    assert t(6, 5, True, 10, "longest_first") == (5, 5) and t(5, 7, True, 10, "longest_first") == (5, 5)
    assert t(5, 9, True, 10, "only_first") == (1, 9) and t(4, 9, True, 9, "only_first") is None and t(9, 4, True, 9, "only_second") is None
    seq = pg.sequence([[1, 2, 3, 4, 5], []])
    cfg = pg.config(single=[["special", 9, 0], ["A", 0, 1], ["special", 8, 0]], max_length=5, truncation_side="left", padding=6, padding_side="left", pad_id=7, pad_type_id=2)
    out = pg.pack(seq, None, cfg)
    assert out["input_ids"].tolist() == [[7, 9, 3, 4, 5, 8], [7, 7, 7, 7, 9, 8]] and out["token_type_ids"].tolist() == [[2, 0, 1, 1, 1, 0], [2, 2, 2, 2, 0, 0]]
    assert out["attention_mask"].tolist() == [[0, 1, 1, 1, 1, 1], [0, 0, 0, 0, 1, 1]] and out["special_tokens_mask"].tolist() == [[1, 1, 0, 0, 0, 1], [1, 1, 1, 1, 1, 1]]
    assert out["offsets"][0].tolist() == [[0, 0], [0, 0], [6, 8], [9, 11], [12, 14], [0, 0]]
    out = pg.pack(seq, None, {**cfg, "padding": None})
    assert out["input_ids"].tolist() == [9, 3, 4, 5, 8, 9, 8] and out["row_offsets"].tolist() == [0, 5, 7] and "attention_mask" not in out
    assert pg.pack(seq, None, {**cfg, "padding": 4, "pad_to_multiple_of": 4})["input_ids"].shape == (2, 8)   # a longer row widens L
    for bad in (dict(single=[["special", 1, 0]]), dict(single=[["A", 0, 0], ["B", 0, 0]]), dict(max_length=1, strategy="only_second"),
                dict(single=cfg["single"], max_length=1), dict(pad_to_multiple_of=0)):
        with pytest.raises(pg.PackError) as ei:
            pg.pack(seq, None, pg.config(**bad))
        assert ei.value.doc is None
    with pytest.raises(pg.PackError) as ei:
        pg.pack(pg.sequence([[1] * 9, [1]]), pg.sequence([[2], [2] * 9]), pg.config(pair=[["A", 0, 0], ["B", 0, 1]], max_length=4, strategy="only_first"))
    assert ei.value.doc == 1


def test_the_definition_agrees_with_the_fixture():
    c = pg.load()
    cases = c["cases"]
    assert len(cases) >= 40 and sum("error" in x for x in cases) >= 10 and 0 < sum(x.get("definition_only", False) for x in cases) <= 0.05 * len(cases)
    seen = set()
    for case in cases:
        cfg = pg.case_config(case)
        a, b = pg.case_sequences(case)
        seen.add((case["template"], cfg["strategy"], cfg["truncation_side"], b is not None))
        seen.add(("padding", cfg["padding"] if cfg["padding"] in (None, "longest") else "fixed", cfg["pad_to_multiple_of"], cfg["padding_side"]))
        want = pg.case_planes(case)
        if want is None:
            with pytest.raises(pg.PackError) as ei:
                pg.pack(a, b, cfg)
            assert ei.value.doc == case["error"]
            continue
        got = pg.pack(a, b, cfg)
        assert got.keys() == want.keys()
        for k in got:
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (case, k)
    for template in ("none", "bert", "roberta"):
        for strategy in ("longest_first", "only_first", "only_second"):
            for side in ("left", "right"):
                assert (template, strategy, side, True) in seen
        assert (template, "longest_first", "right", False) in seen and (template, "longest_first", "left", False) in seen
    for pad in (("padding", "longest", None), ("padding", "fixed", None), ("padding", "longest", 8), ("padding", None, None)):
        assert pad + ("left",) in seen and pad + ("right",) in seen, pad
    # the BERT pipeline's block: the definition over the untruncated tokens that normalize_cases.json holds
    import normalize_golden as ng
    ids, spans = ng.tokens()
    seq = [[(i, s, e) for i, (s, e) in zip(x, y)] for x, y in zip(ids, spans)]
    got, want = pg.pack(seq, None, c["bert"]["config"]), pg.pipeline_planes(c["bert"])
    assert want["input_ids"].shape == (len(ng.docs()), 16)
    for k in got:
        assert np.array_equal(got[k], want[k]), k


def test_the_maker_reproduces_the_fixture():
    if importlib.util.find_spec("tokenizers") is None:
        pytest.skip("the maker needs `tokenizers`")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_pack_golden.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("checked "), (r.stdout[-2000:], r.stderr[-2000:])
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "pack_cases.json")) < 64 * 1024


# ---------------------------------------------------------------------------------------------- the lane bodies under sanitizers
def _exe(tmp_path):
    exe = str(tmp_path / "pack_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-o", exe, os.path.join(ROOT, "tests", "native", "pack_check.cpp")])
    return exe


def _batch_file(cfg, a, b, width):
    pair = b is not None
    template = cfg["pair"] if pair else cfg["single"]
    n_added = sum(p[0] == "special" for p in template)
    kind = {"special": 0, "A": 1, "B": 2}
    lines = [" ".join(["P", str(len(template))] + [f"{kind[k]} {i} {t}" for k, i, t in template])]
    trunc = cfg["max_length"] is not None
    pad = 0 if cfg["padding"] is None else 1 if cfg["padding"] == "longest" else 2
    lines.append(" ".join(str(x) for x in ("C", int(trunc), cfg["max_length"] - n_added if trunc else 0, ["longest_first", "only_first", "only_second"].index(cfg["strategy"]),
                                           int(cfg["truncation_side"] == "left"), pad, cfg["padding"] if pad == 2 else 0, cfg["pad_to_multiple_of"] or 1,
                                           int(cfg["padding_side"] == "left"), cfg["pad_id"], cfg["pad_type_id"], width, int(pair))))
    for d in range(len(a)):
        for tag, seq in (("A", a), ("B", b)):
            if seq is not None:
                lines.append(" ".join([tag, str(len(seq[d]))] + [f"{i} {s} {e}" for i, s, e in seq[d]]))
    return "\n".join(lines) + "\n"


def test_pack_lane_bodies_on_the_host_under_sanitizers(tmp_path):
    """the header and slot bodies of pack_kernels.hip as plain C++: every case of the fixture, error cases included, in both widths
    against the recorded planes; then 2 x 3000 rounds of random and hostile batches against a sequential restatement"""
    exe = _exe(tmp_path)
    names = {"I": "input_ids", "T": "token_type_ids", "M": "attention_mask", "S": "special_tokens_mask", "O": "offsets", "R": "row_offsets"}
    for k, case in enumerate(pg.load()["cases"]):
        cfg = pg.case_config(case)
        a, b = pg.case_sequences(case)
        want = pg.case_planes(case)
        for width in (4, 8):
            path = tmp_path / f"case{k}.txt"
            path.write_text(_batch_file(cfg, a, b, width))
            r = subprocess.run([exe, "batch", str(path)], capture_output=True, text=True)
            assert r.returncode == 0 and r.stderr == "", (r.stdout[-2000:], r.stderr[-2000:])
            got = {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in r.stdout.split("\n")[:-1]}
            if want is None:
                assert got == {"E": [case["error"], 1]}, (k, got)
                continue
            assert set(got) == {"L"} | {t for t, name in names.items() if name in want}, k
            L = want["input_ids"].shape[-1] if cfg["padding"] is not None else int(np.diff(want["row_offsets"].astype(np.int64)).max())
            assert got["L"] == [L, want["input_ids"].size], k
            for t, name in names.items():
                if name in want:
                    assert got[t] == want[name].reshape(-1).tolist(), (k, name, width)
    for seed in (1, 2):
        r = subprocess.run([exe, "random", "3000", str(seed)], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.startswith("OK 3000 rounds") and r.stderr == "", (r.stdout, r.stderr)
