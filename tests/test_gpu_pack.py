"""Model inputs on the MI355X (daac_tokens_pack; Packer and tokenize_wordpiece_docs / tokenize_bpe_docs with pack=..).  The expected
planes come from `tokenizers`' own results in tests/golden/pack_cases.json (make_pack_golden.py writes them) and from the pure-Python
definition (tests/pack_golden.py), which test_pack_host.py ties to the fixture; nothing here reads the library under test for its
expectations, and every comparison is exact.

Shapes are the smallest that cross the slot kernel's boundaries: rows of 1, 63, 64, 65 and 130 slots, so that a wave of 64 lanes holds
several rows, one row exactly, or a part of one, in batches of 1, 2, 257 and 1031 rows, which span several workgroups of 256 lanes; one
row of 5 000 tokens beside empty rows; no document at all.  The call on a caller's busy stream is tests/test_gpu_tokens_pack_stream.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import normalize_golden as ng
import pack_golden as pg
import tokenizer_golden as tg
import wordpiece_golden as wg
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

import daachorse_amd as da
from daachorse_amd import Gap, Split, _ffi

BERT_SINGLE = [["special", 101, 0], ["A", 0, 0], ["special", 102, 0]]
BERT_PAIR = BERT_SINGLE + [["B", 0, 1], ["special", 102, 1]]


def _packer(cfg, dtype=np.int64):
    return da.Packer(**pg.packer_kwargs(cfg), dtype=dtype)


def _same(got, want, dtype, what):
    assert got.keys() == want.keys(), (what, sorted(got), sorted(want))
    for k, w in want.items():
        g = got[k]
        assert g.dtype == (w.dtype if k in ("offsets", "row_offsets") else dtype) and g.shape == w.shape and np.array_equal(g, w), (what, k)


def _without_offsets(planes):
    return {k: v for k, v in planes.items() if k != "offsets"}


def _seeded(seed, lengths, lo=10, hi=30000):
    """a sequence of documents of the given token counts: seeded ids, spans that tile the document with tokens of 1 .. 5 bytes"""
    rng = np.random.default_rng(seed)
    out = []
    for n in lengths:
        ids = rng.integers(lo, hi, size=n).tolist()
        ends = np.cumsum(rng.integers(1, 6, size=n)).tolist()
        out.append(list(zip(ids, [0] + ends[:-1], ends)))
    return out


# ------------------------------------------------------------------------------------------------------------- 1. the fixture
@pytest.mark.parametrize("with_spans", [True, False], ids=["spans", "no_spans"])
@pytest.mark.parametrize("dtype", [np.int32, np.int64], ids=["int32", "int64"])
def test_pack_on_the_fixture(dtype, with_spans):
    """every case of the first block, the CSR cases and the error cases included, on every plane"""
    n_csr = n_err = 0
    for k, case in enumerate(pg.load()["cases"]):
        cfg = pg.case_config(case)
        a, b = pg.case_sequences(case)
        p = _packer(cfg, dtype)
        args = (pg.flatten(a, with_spans), None if b is None else pg.flatten(b, with_spans))
        want = pg.case_planes(case)
        if want is None:
            with pytest.raises(da.DaachorseError) as ei:
                p.pack(*args)
            assert ei.value.code == 1 and f"document {case['error']}:" in str(ei.value) and cfg["strategy"] in str(ei.value), k
            n_err += 1
            continue
        n_csr += cfg["padding"] is None
        _same(p.pack(*args), want if with_spans else _without_offsets(want), dtype, k)
    assert n_csr >= 5 and n_err >= 10   # (the CSR form is a quarter of the cases; a dozen of the cases are errors)


def test_device_inputs_and_device_results():
    """the token calls' own result objects in, DeviceMatches / DeviceOffsets out: a pair batch of the fixture, dense and CSR"""
    case = next(c for c in pg.load()["cases"] if c["b"] is not None and "want" in c and c["template"] == "bert")
    a, b = pg.case_sequences(case)

    def dev(seq):
        ids, spans, off = pg.flatten(seq)
        t = [torch.from_numpy(ids.view(np.int32)).cuda(), torch.from_numpy(spans.view(np.int64)).cuda(), torch.from_numpy(off.view(np.int64)).cuda()]
        return t, (da.bytewise.DeviceMatches(t[0].data_ptr(), len(ids), np.dtype(np.uint32)), da.bytewise.DeviceMatches(t[1].data_ptr(), len(ids), da.bytewise.SPAN_DTYPE),
                   da.bytewise.DeviceOffsets(t[2].data_ptr(), len(off)))

    keep_a, da_ = dev(a)
    keep_b, db_ = dev(b)
    try:
        for padding in ("longest", None):
            cfg = {**pg.case_config(case), "padding": padding}
            out = _packer(cfg).pack(da_, db_, device=True)
            want = pg.pack(a, b, cfg)
            assert {k: v.shape for k, v in out.items() if k != "row_offsets"} == {k: v.shape for k, v in want.items() if k != "row_offsets"}
            got = {k: (v.to_numpy().reshape(v.shape) if k != "row_offsets" else v.to_numpy()) for k, v in out.items()}
            for v in out.values():
                v.free()
            _same(got, want, np.int64, padding)
            _same(_packer(cfg).pack(tuple(keep_a), tuple(keep_b)), want, np.int64, "CUDA tensors")   # int32 / int64 tensors of the same bits
    finally:
        for o in da_ + db_:
            o.ptr = None   # the tensors own the memory


# --------------------------------------------------------------------------------------------------- 2. the slot kernel's shapes
@pytest.mark.parametrize("L", [1, 63, 64, 65, 130])
def test_rows_that_straddle_waves_and_blocks(L):
    """rows of exactly L slots (the longest row is L) in batches of 1, 2, 257 and 1031: dense with the padding on either side, and
    the same rows in the CSR form; int32 for the odd batches"""
    for n in (1, 2, 257, 1031):
        single = BERT_SINGLE if L >= 3 else [["A", 0, 0]]
        room = L - (2 if L >= 3 else 0)
        rng = np.random.default_rng(1000 * L + n)
        lengths = rng.integers(0, room + 1, size=n)
        lengths[rng.integers(0, n)] = room
        a = _seeded(L * 7919 + n, lengths.tolist())
        dtype = np.int32 if n % 2 else np.int64
        for kw in (dict(padding_side="right"), dict(padding_side="left"), dict(padding=None)):
            cfg = pg.config(single=single, pad_id=7, pad_type_id=1, **kw)
            want = pg.pack(a, None, cfg)
            assert cfg["padding"] is None or want["input_ids"].shape == (n, L)
            _same(_packer(cfg, dtype).pack(pg.flatten(a)), want, dtype, (L, n, kw))
    assert _ffi.last_kernel().startswith("pack docs=1031 pair=0 row=" + str(L))


def test_edges_of_the_definition():
    P = lambda cfg, a, b=None, dtype=np.int64: _packer(cfg, dtype).pack(pg.flatten(a), None if b is None else pg.flatten(b))
    # all documents empty: without a template there is no slot at all, with one the rows are the template's
    empty = [[] for _ in range(70)]
    for cfg in (pg.config(), pg.config(padding=None), pg.config(padding=8), pg.config(single=BERT_SINGLE), pg.config(single=BERT_SINGLE, pair=BERT_PAIR, padding=None)):
        b = empty if cfg["pair"] else None
        _same(P(cfg, empty, b), pg.pack(empty, b, cfg), np.int64, ("empty documents", cfg))
    assert P(pg.config(), empty)["input_ids"].shape == (70, 0)
    # no document
    for cfg in (pg.config(single=BERT_SINGLE), pg.config(single=BERT_SINGLE, padding=None), pg.config(single=BERT_SINGLE, padding=32)):
        got = P(cfg, [])
        if cfg["padding"] is None:
            assert got["row_offsets"].tolist() == [0] and got["input_ids"].shape == (0,) and got["offsets"].shape == (0, 2) and "attention_mask" not in got
        else:
            assert got["input_ids"].shape == (0, 0) and got["offsets"].shape == (0, 0, 2) and got["attention_mask"].dtype == np.int64
    assert _ffi.last_kernel() == "pack docs=0 pair=0 row=0 tokens=0 dropped=0"
    # one row of 5 000 tokens beside empty rows
    a = _seeded(5, [0, 0, 5000, 0, 0, 0, 0])
    for cfg in (pg.config(single=BERT_SINGLE), pg.config(single=BERT_SINGLE, padding=None), pg.config(padding_side="left", pad_to_multiple_of=64)):
        _same(P(cfg, a, dtype=np.int32), pg.pack(a, None, cfg), np.int32, ("a long row", cfg))
    assert "tokens=5000 dropped=0" in _ffi.last_kernel()
    # left padding combined with left truncation, pairs; an odd budget with n1 > n2; a multiple that already divides L
    a, b = _seeded(6, [9, 3, 0, 20, 7, 8]), _seeded(7, [8, 30, 4, 20, 0, 7])
    cfg = pg.config(single=BERT_SINGLE, pair=BERT_PAIR, max_length=14, truncation_side="left", padding_side="left", pad_id=3)
    want = pg.pack(a, b, cfg)
    assert want["input_ids"].shape == (6, 14) and int(want["attention_mask"][2].sum()) == 7 and want["input_ids"][0].tolist().count(3) == 0
    assert [int((want["token_type_ids"][0] == t).sum()) for t in (0, 1)] == [8, 6]   # budget 11, n1 = 9 > n2 = 8: A keeps 6, B keeps 5
    _same(P(cfg, a, b), want, np.int64, "left and left")
    assert "row=14 tokens=" in _ffi.last_kernel() and "dropped=" + str(sum(map(len, a + b)) - int((want["special_tokens_mask"] == 0).sum())) in _ffi.last_kernel()
    for mult, L in ((7, 14), (14, 14), (8, 16), (1, 14)):
        c = {**cfg, "pad_to_multiple_of": mult}
        want = pg.pack(a, b, c)
        assert want["input_ids"].shape == (6, L)
        _same(P(c, a, b), want, np.int64, ("multiple", mult))
    c = {**cfg, "padding": 10, "max_length": None}   # a row longer than the fixed length widens L
    want = pg.pack(a, b, c)
    assert want["input_ids"].shape == (6, 43)
    _same(P(c, a, b), want, np.int64, "fixed below the longest row")
    # ids above 2^31 are zero-extended into int64
    big = [[(0xFFFFFFFE, 0, 1), (0x80000000, 1, 2)]]
    assert P(pg.config(), big)["input_ids"].tolist() == [[0xFFFFFFFE, 0x80000000]]


# ----------------------------------------------------------------------------------------------------------- 3. the refusals
class _Raw:
    """daac_tokens_pack over device tensors, with every out-pointer set to a value the call has to clear"""

    def __init__(self, packer, a, b=None):
        self.p = packer
        self.keep = [[torch.from_numpy(x.view(np.int32 if x.dtype.itemsize == 4 else np.int64).copy()).cuda() for x in pg.flatten(s)] for s in ((a,) if b is None else (a, b))]
        self.tokens = [sum(map(len, s)) for s in ((a,) if b is None else (a, b))]
        self.n = len(a)
        self.outs = [C.c_void_p(5) for _ in range(6)]
        self.L, self.slots = C.c_uint64(5), C.c_uint64(5)

    def run(self, stream=None):
        ptr = lambda t: t.data_ptr() if t.numel() else None
        seq = [(ptr(k[0]), ptr(k[1]), k[2].data_ptr(), t) for k, t in zip(self.keep, self.tokens)] + [(None, None, None, 0)]
        return _ffi.lib().daac_tokens_pack(C.byref(self.p.params), *seq[0], *seq[1], self.n, stream, *[C.byref(o) for o in self.outs], C.byref(self.L), C.byref(self.slots))

    def cleared(self):
        return all(o.value is None for o in self.outs) and (self.L.value, self.slots.value) == (0, 0)


def test_the_failing_document_is_named_and_nothing_is_handed_over():
    n = 700   # several workgroups: the first failing document of all is the answer, whichever wave finds it
    la, lb = np.full(n, 9), np.full(n, 9)
    la[[311, 650, 699]], lb[[311, 650, 699]] = 1, 20   # budget 10: only_first would have to take 11 tokens from a sequence of 1
    a, b = _seeded(8, la.tolist()), _seeded(9, lb.tolist())
    for padding in ("longest", None):
        r = _Raw(_packer(pg.config(single=BERT_SINGLE, pair=BERT_PAIR, max_length=13, strategy="only_first", padding=padding)), a, b)
        assert r.run() == 1 and r.cleared()
        msg = _ffi.lib().daac_last_error().decode()
        assert msg.startswith("document 311: only_first"), msg
    r = _Raw(_packer(pg.config(single=BERT_SINGLE, pair=BERT_PAIR, max_length=13, strategy="only_second")), b, a)
    assert r.run() == 1 and r.cleared() and _ffi.lib().daac_last_error().decode().startswith("document 311: only_second")
    with pytest.raises(pg.PackError) as ei:
        pg.pack(a, b, pg.config(single=BERT_SINGLE, pair=BERT_PAIR, max_length=13, strategy="only_first"))
    assert ei.value.doc == 311
    # offsets that leave the token list or decrease are a document in error too, in front of one that cannot be truncated
    r = _Raw(_packer(pg.config(single=BERT_SINGLE, pair=BERT_PAIR, max_length=13, strategy="only_first")), a, b)
    off = r.keep[1][2]
    off[401] = off[-1] + 1
    assert r.run() == 1 and r.cleared() and _ffi.lib().daac_last_error().decode().startswith("document 311: only_first")
    off[100] = 0
    assert r.run() == 1 and r.cleared()
    msg = _ffi.lib().daac_last_error().decode()
    assert msg.startswith("document 99: its token offsets"), msg
    # the same batch with longest_first is served
    r = _Raw(_packer(pg.config(single=BERT_SINGLE, pair=BERT_PAIR, max_length=13)), a, b)
    assert r.run() == 0 and (r.L.value, r.slots.value) == (13, 13 * n) and all(o.value for o in r.outs[:5]) and r.outs[5].value is None
    for o in r.outs[:5]:
        _ffi.lib().daac_device_free(o)


def test_max_result_bytes_is_answered_before_the_planes_are_allocated():
    a = _seeded(10, [5, 6, 7, 8])   # rows of 10 slots at the most: 4 x 10 x (4 planes x 8 + 16) = 1920 bytes, CSR 34 x (3 x 8 + 16) = 1360
    for cfg, need in ((pg.config(single=BERT_SINGLE), 1920), (pg.config(single=BERT_SINGLE, padding=None), 1360)):
        want = pg.pack(a, None, cfg)
        for limit, ok in ((need - 1, False), (need, True)):
            da.set_option("max_result_bytes", limit)
            try:
                if ok:
                    _same(_packer(cfg).pack(pg.flatten(a)), want, np.int64, limit)
                else:
                    r = _Raw(_packer(cfg), a)
                    assert r.run() == 2 and r.cleared() and "max_result_bytes" in _ffi.lib().daac_last_error().decode()
            finally:
                da.set_option("max_result_bytes", 8 << 30)
    da.set_option("max_result_bytes", 1 << 20)   # a fixed length that would take 2^40 slots a row is refused, not allocated
    try:
        r = _Raw(_packer(pg.config(padding=1 << 40)), a)
        assert r.run() == 2 and r.cleared()
    finally:
        da.set_option("max_result_bytes", 8 << 30)


# ---------------------------------------------------------------------------------------------------------- 4. end to end
def test_wordpiece_docs_with_pack_equal_tokenizers_bert_pipeline():
    """raw documents in device memory -> BERT's normalizer, the special-token cut, Split.Bert, WordPiece, splice and pack: the planes
    `tokenizers` gives for [CLS] A [SEP], max_length 16 and padding longest, raw-text offsets included"""
    block = pg.load()["bert"]
    want = pg.pipeline_planes(block)
    spec = {t: i for t, i in block["specials"]}
    cfg = block["config"]
    assert cfg["single"] == [["special", spec["[CLS]"], 0], ["A", 0, 0], ["special", spec["[SEP]"], 0]] and cfg["pad_id"] == spec["[PAD]"]
    patterns, first, cont = da.wordpiece_tables(wg.load("vocab")["vocab"])
    _, unk_id, max_chars, _ = wg.model()
    pma = da.DoubleArrayAhoCorasick.new(patterns)
    docs = ng.docs()
    off = np.zeros(len(docs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(d) for d in docs])
    batch = (torch.from_numpy(np.frombuffer(b"".join(docs), dtype=np.uint8).copy()).cuda(), torch.from_numpy(off).cuda())
    st, nz = da.SpecialTokens(spec), da.bert_normalizer()
    packer = da.Packer(da.bert_template(spec["[CLS]"], spec["[SEP]"]), max_length=16, pad_id=spec["[PAD]"])
    got = pma.tokenize_wordpiece_docs(batch, first, cont, unk_id, max_chars, spans=True, normalizer=nz, special=st, pack=packer)
    _same(got, want, np.int64, "device documents")
    assert _ffi.last_kernel().startswith(f"pack docs={len(docs)} pair=0 row=16 ")
    _same(pma.tokenize_wordpiece_docs(docs, first, cont, unk_id, max_chars, normalizer=nz, special=st, pack=packer), _without_offsets(want), np.int64, "host documents, no spans")
    out = pma.tokenize_wordpiece_docs(batch, first, cont, unk_id, max_chars, spans=True, normalizer=nz, pack=da.Packer(da.bert_template(spec["[CLS]"], spec["[SEP]"]), max_length=16, pad_id=spec["[PAD]"], dtype=np.int32), device=True)
    assert out["input_ids"].shape == (len(docs), 16) and out["offsets"].shape == (len(docs), 16, 2)
    got = {k: v.to_numpy().reshape(v.shape) for k, v in out.items()}
    for v in out.values():
        v.free()
    _same(got, want, np.int32, "without special=, int32, device results")   # no document of the list holds a special token's text


def test_bpe_docs_with_pack_equal_tokenizers_roberta_pipeline():
    """byte-level BPE behind the GPT-2 split, then <s> A </s> with max_length 16 cut on the left and padding longest"""
    block = pg.load()["roberta"]
    spec = {t: i for t, i in block["specials"]}
    docs = ng.docs()[:block["n_docs"]]
    pieces = tg.bpe_pieces()
    token_offsets = []   # the pieces tile the document: the kept tokens are its last ones
    for d, ids in zip(docs, block["ids"]):
        toks, end, spans = [i for i in ids if i < len(pieces)], len(d), []
        for i in reversed(toks):
            spans.append((end - len(pieces[i]), end))
            end -= len(pieces[i])
        assert end >= 0 and (end == 0 or len(toks) == 14)
        token_offsets.append(spans[::-1])
    want = pg.pipeline_planes(block, token_offsets)
    assert want["input_ids"].shape == (len(docs), 16) and sum(s[0][0] > 0 for s in token_offsets if s) >= 20
    o = orc.OraclePma.build(pieces, values=np.arange(len(pieces), dtype=np.uint32))
    pma, rest = da.DoubleArrayAhoCorasick.deserialize(o.serialize())
    assert rest == b""
    packer = da.Packer(da.roberta_template(spec["<s>"], spec["</s>"]), max_length=16, truncation_side="left", pad_id=spec["<pad>"])
    got = pma.tokenize_bpe_docs(docs, split=Split.Gpt2, gap=Gap.Bytes, gap_id=1 << 20, spans=True, special=da.SpecialTokens(spec), pack=packer)
    _same(got, want, np.int64, "tokenize_bpe_docs(pack=)")
    _same(pma.tokenize_bpe_docs(docs, gap_id=1 << 20, pack=packer), _without_offsets(want), np.int64, "no spans, no specials")
