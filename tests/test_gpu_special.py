"""Special tokens in raw text on the MI355X (daac_cut_batch / daac_tokens_splice; SpecialTokens, splice_special and
tokenize_bpe_docs / tokenize_wordpiece_docs with special=..).  The expected segments and tokens come from the pure-Python definition
(tests/special_golden.py) and from `tokenizers`' own ids and spans in tests/golden/special_tokens_cases.json (make_special_golden.py
writes them and test_special_host.py ties the two together); nothing here reads the library under test for its expectations, and every
comparison is exact.

Shapes are the smallest that cross the kernels' boundaries: a wave of 64, a workgroup of 256 lanes, a scan chunk of 2048 items (one
workgroup sums up to 8192 counts, the chunked sum takes over above), a document beyond batch_lane_max."""
import numpy as np
import pytest
import torch

import special_golden as sg
import tokenizer_golden as tg
import wordpiece_golden as wg
from oracle import oracle as orc
from test_gpu_streams import _Delay, _h, _no_collection

pytestmark = pytest.mark.gpu

import daachorse_amd as da
from daachorse_amd import Engine, Gap, Split

GID = 1 << 20
EOT = b"<|endoftext|>"


def _device_batch(docs, front=b"", tail=b""):
    """(hay, offsets) on the device: `front`, the documents, `tail`; offsets[0] = len(front)"""
    off = np.full(len(docs) + 1, len(front), dtype=np.int64)
    off[1:] += np.cumsum([len(d) for d in docs], dtype=np.int64)
    hay = np.frombuffer(front + b"".join(docs) + tail or b"\0", dtype=np.uint8)
    return torch.from_numpy(hay.copy()).cuda(), torch.from_numpy(off).cuda()


def _same(got, want, what):
    assert len(got) == len(want), what
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), what


def _flat(ids, spans):
    return (np.array([i for a in ids for i in a], dtype=np.uint32), np.array([s for b in spans for s in b], dtype=np.uint64).reshape(-1, 2),
            np.cumsum([0] + [len(a) for a in ids]).astype(np.uint64))


@pytest.fixture(scope="module")
def specials():
    """-> {name: (SpecialTokens, [(bytes, id)])}: both lists of the fixture, bytewise, and the BPE list on a charwise handle"""
    out = {w: (da.SpecialTokens(sg.specials(w)), sg.specials(w)) for w in ("bpe", "wordpiece")}
    spec = sg.specials("bpe")
    cw = da.CharwiseDoubleArrayAhoCorasickBuilder().match_kind(da.MatchKind.LeftmostLongest).build_with_values([(t.decode(), i) for t, i in spec])
    out["charwise"] = (da.SpecialTokens(cw), spec)
    return out


def _want_cut(docs, spec, base=0):
    return sg.cut(docs, lambda d: sg.leftmost(d, spec), base)


# ------------------------------------------------------------------------------------------------------------- 1. the fixture
@pytest.mark.parametrize("which", ["bpe", "wordpiece", "charwise"])
@pytest.mark.parametrize("engine", [Engine.Auto, Engine.DArray])
def test_cut_batch_on_the_fixture(specials, which, engine):
    st, spec = specials[which]
    docs = sg.docs()
    _same(st.cut_batch(docs, engine=engine), _want_cut(docs, spec), "host list")
    assert "cut docs=%d matches=" % len(docs) in da.last_kernel() and "batch " in da.last_kernel()
    # a device batch with offsets[0] != 0; the bytes in front of it and behind it hold a special and complete one across either end
    front, tail = b"zz<|a|>[CLS]<|endof", b"|><|a|>[SEP]"
    ends = [b"text|>x"] + docs + [b"y<|a"]
    out = st.cut_batch(_device_batch(ends, front, tail), engine=engine, device=True)
    assert isinstance(out[0], da.bytewise.DeviceOffsets) and isinstance(out[2], da.bytewise.DeviceMatches) and out[2].dtype == np.uint32
    want = _want_cut(ends, spec, base=len(front))
    assert out[2].n_special == int((want[2] != sg.TEXT).sum())
    _same([o.to_numpy() for o in out], want, "device batch")
    for o in out:
        o.free()


# ---------------------------------------------------------------------------------------------------------- 2. the boundaries
def test_a_special_across_a_document_boundary_is_none(specials):
    st, spec = specials["bpe"]
    docs = [b"text|>" + b"ab"[: 1 + i % 2] + b"<|endof" for i in range(300)]
    so, ds, sv = st.cut_batch(docs)
    assert sv.tolist() == [sg.TEXT] * 300 and ds.tolist() == list(range(301))
    _same((so, ds, sv), _want_cut(docs, spec), "300 documents")
    _same(st.cut_batch(_device_batch(docs, b"<|endof", b"text|>")), _want_cut(docs, spec, base=7), "device")


def test_one_document_of_2500_adjacent_specials(specials):
    st, spec = specials["bpe"]
    docs = [b"x", b"<|a|>" * 2500, b"", b"<|a|>y"]
    so, ds, sv = st.cut_batch(docs)
    assert ds.tolist() == [0, 1, 2501, 2501, 2503] and (sv[1:2501] == dict(spec)[b"<|a|>"]).all()
    _same((so, ds, sv), _want_cut(docs, spec), "2500 specials")


@pytest.mark.parametrize("n", [63, 64, 65, 256, 257, 2047, 2048, 2049, 2500, 8193])
def test_one_byte_documents_without_a_special(specials, n):
    st, spec = specials["bpe"]
    docs = [b"<|a|>"[i % 5: i % 5 + 1] for i in range(n)]
    _same(st.cut_batch(docs), (np.arange(n + 1, dtype=np.uint64), np.arange(n + 1, dtype=np.uint64), np.full(n, sg.TEXT, dtype=np.uint32)), n)


@pytest.mark.parametrize("n", [64, 2048, 8192])
def test_items_at_the_edges_of_the_sums(specials, n):
    """n items exactly, one more and one fewer: documents of one special each, so a document is two items and two or three segments"""
    st, spec = specials["bpe"]
    for items in (n - 1, n, n + 1):
        docs = [(b"<|a|>", b"<|a|>z", b"q<|a|>z")[i % 3] for i in range(items // 2)] + [b"w"] * (items % 2)
        _same(st.cut_batch(docs), _want_cut(docs, spec), items)


def test_a_document_beyond_batch_lane_max(specials):
    st, spec = specials["bpe"]
    word = b"lorem ipsum "
    long_doc = b"<|a|>" + word * 1364 + EOT + b"x" + b"<|a|><|b|>" + word * 40 + b"the" + EOT   # the second special starts at 16 373, ends at 16 386
    assert len(long_doc) > 16384 + 400 and long_doc.index(EOT) < 16384 < long_doc.index(EOT) + len(EOT)
    docs = [b"a<|a|>", long_doc, b"", b"<|a|>b"]
    _same(st.cut_batch(docs), _want_cut(docs, spec), "host")
    assert "long_docs=1" in da.last_kernel()
    _same(st.cut_batch(_device_batch(docs, b"<|a", b"|>")), _want_cut(docs, spec, base=3), "device")


def test_no_document_and_only_empty_documents(specials):
    for which in ("bpe", "charwise"):
        st, _ = specials[which]
        so, ds, sv = st.cut_batch([])
        assert so.tolist() == [0] and ds.tolist() == [0] and sv.tolist() == [] and sv.dtype == np.uint32
        assert da.last_kernel().startswith("cut docs=0 matches=0 segs=0")
        so, ds, sv = st.cut_batch([b"", b"", b""])
        assert so.tolist() == [0] and ds.tolist() == [0, 0, 0, 0] and sv.tolist() == []
        so, ds, sv = st.cut_batch(_device_batch([b"", b""], b"<|a|>", b"<|a|>"))
        assert so.tolist() == [5] and ds.tolist() == [0, 0, 0] and sv.tolist() == []


# ------------------------------------------------------------------------------------------------------------ 3. the splice
@pytest.fixture(scope="module")
def csr():
    """random CSR inputs of the splice: 3 000 segments in 700 documents (some empty), a third of them special with 0, 1 or 5 garbage
    tokens under them, text segments with 0 .. 6 tokens, one with 5 000; and what the definition makes of them (computed once)"""
    rng = np.random.default_rng(20261021)
    n_segs, n_docs = 3000, 700
    seg_len = rng.integers(1, 30, n_segs)
    values = np.where(rng.integers(0, 3, n_segs) == 0, rng.integers(0, 0xFFFFFFFF, n_segs), sg.TEXT).astype(np.uint32)
    cuts = np.sort(rng.choice(np.arange(n_segs + 1), n_docs - 1))   # with repeats: empty documents
    doc_segs = np.concatenate([[0], cuts, [n_segs]]).astype(np.uint64)
    base = 11
    seg_offsets = (base + np.concatenate([[0], np.cumsum(seg_len)])).astype(np.uint64)
    doc_offsets = seg_offsets[doc_segs.astype(np.int64)]
    counts = np.where(values == sg.TEXT, rng.integers(0, 7, n_segs), rng.choice([0, 1, 5], n_segs))
    big = int(np.flatnonzero(values == sg.TEXT)[1500 // 3])
    counts[big] = 5000
    seg_tok = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    t = int(seg_tok[-1])
    ids = rng.integers(0, 1 << 32, t, dtype=np.uint64).astype(np.uint32)
    starts = rng.integers(0, 40, t)
    spans = np.stack([starts, starts + rng.integers(0, 9, t)], axis=1).astype(np.uint64)
    want = sg.splice(ids, spans, seg_tok, values, seg_offsets, doc_segs, doc_offsets)
    assert (np.diff(doc_segs.astype(np.int64)) == 0).sum() > 20 and (counts[values == sg.TEXT] == 0).sum() > 100
    return dict(ids=ids, spans=spans, seg_tok=seg_tok, values=values, seg_offsets=seg_offsets, doc_segs=doc_segs, doc_offsets=doc_offsets, want=want,
                hay_len=int(seg_offsets[-1]) + 3)


def _dev(a):
    view = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}[a.dtype]
    return torch.from_numpy(np.ascontiguousarray(a).view(view).copy()).cuda()


def _splice_args(c):
    docs = (torch.zeros(c["hay_len"], dtype=torch.uint8, device="cuda"), _dev(c["doc_offsets"]))
    return _dev(c["ids"]), _dev(c["spans"]), _dev(c["seg_tok"]), (_dev(c["seg_offsets"]), _dev(c["doc_segs"]), _dev(c["values"])), docs


@pytest.mark.parametrize("with_spans", [True, False])
def test_splice_special_on_random_csr_inputs(csr, with_spans):
    ids, spans, seg_tok, cut, docs = _splice_args(csr)
    want = csr["want"] if with_spans else (csr["want"][0], csr["want"][2])
    _same(da.splice_special(ids, spans if with_spans else None, seg_tok, cut, docs), want, "numpy results")
    assert da.last_kernel() == "splice docs=700 segs=3000 tokens=%d" % len(want[0])
    out = da.splice_special(ids, spans if with_spans else None, seg_tok, cut, docs, device=True)
    _same([o.to_numpy() for o in out], want, "device results")
    for o in out:
        o.free()


def test_splice_special_without_segments_or_tokens():
    zero = torch.zeros(1, dtype=torch.int64, device="cuda")
    none32 = torch.zeros(0, dtype=torch.int32, device="cuda")
    ids, off = da.splice_special(None, None, zero, (zero, zero, none32), [])
    assert ids.tolist() == [] and ids.dtype == np.uint32 and off.tolist() == [0]
    ids, spans, off = da.splice_special(none32, torch.zeros((0, 2), dtype=torch.int64, device="cuda"), zero, (zero, torch.zeros(4, dtype=torch.int64, device="cuda"), none32),
                                        [b"", b"", b""])
    assert ids.tolist() == [] and spans.shape == (0, 2) and off.tolist() == [0, 0, 0, 0]
    # specials alone: no token comes in, one a segment goes out
    so, ds = _dev(np.array([0, 5, 10], dtype=np.uint64)), _dev(np.array([0, 2], dtype=np.uint64))
    ids, spans, off = da.splice_special(None, torch.zeros((0, 2), dtype=torch.int64, device="cuda"), torch.zeros(3, dtype=torch.int64, device="cuda"),
                                        (so, ds, _dev(np.array([7, 8], dtype=np.uint32))), [b"<|a|><|a|>"])
    assert ids.tolist() == [7, 8] and spans.tolist() == [[0, 5], [5, 10]] and off.tolist() == [0, 2]


def test_splice_special_behind_tokenize_batch_chained_by_the_caller(specials):
    """cut_batch(device=True), tokenize_batch over (hay, seg_offsets) and splice_special, nothing on the host in between: the words of
    a small dictionary and Gap.Bytes between them, against the same three steps of the definition"""
    st, spec = specials["bpe"]
    words = [b"he", b"hello", b"world", b" ", b"o", b"<|", b"a"]
    o = orc.OraclePma.build(words, kind=orc.LEFTMOST_LONGEST)
    p, _ = da.DoubleArrayAhoCorasick.deserialize(o.serialize())
    docs = sg.docs()
    batch = _device_batch(docs, b"<|a|>he", b"llo")

    def text(seg):   # tokenize_batch's definition: the leftmost matches' values, a token of GID + byte for every byte between them
        ids, spans, pos = [], [], 0
        for s, e, v in [(int(m["start"]), int(m["end"]), int(m["value"])) for m in o.leftmost_find_iter(seg)] + [(len(seg), len(seg), None)]:
            for q in range(pos, s):
                ids.append(GID + seg[q])
                spans.append((q, q + 1))
            if v is not None:
                ids.append(v)
                spans.append((s, e))
            pos = e
        return ids, spans

    per_doc = sg.tokenize_docs(docs, lambda d: sg.leftmost(d, spec), text)
    want = _flat([i for i, _ in per_doc], [s for _, s in per_doc])
    cut = st.cut_batch(batch, device=True)
    ids, spans, seg_tok = p.tokenize_batch((batch[0], cut[0]), gap=Gap.Bytes, gap_id=GID, spans=True, device=True)
    _same(da.splice_special(ids, spans, seg_tok, cut, batch), want, "tokenize_batch behind the cut")
    for x in (ids, spans, seg_tok) + tuple(cut):
        x.free()


# ------------------------------------------------------------------------------------------------------------------ 4. BPE
@pytest.fixture(scope="module")
def bpe():
    pieces = tg.bpe_pieces()
    o = orc.OraclePma.build(pieces, values=np.arange(len(pieces), dtype=np.uint32))
    p, rest = da.DoubleArrayAhoCorasick.deserialize(o.serialize())
    assert rest == b""
    return p, pieces


def test_bpe_docs_with_specials_equal_tokenizers(bpe, specials):
    p, pieces = bpe
    st, spec = specials["bpe"]
    docs, case = sg.docs(), sg.load()
    want_spans = sg.bpe_spans([len(x) for x in pieces], {i: len(t) for t, i in spec})
    for d, spans in zip(docs, want_spans):
        assert (spans[-1][1] if spans else 0) == len(d)
    want = _flat(case["bpe_ids"], want_spans)
    got = p.tokenize_bpe_docs(docs, split=Split.Gpt2, gap=Gap.Bytes, gap_id=GID, spans=True, special=st)
    _same(got, want, "host documents")
    _same(p.tokenize_bpe_docs(docs, gap_id=GID, special=st), (want[0], want[2]), "no spans")
    out = p.tokenize_bpe_docs(_device_batch(docs, b"zz<|a|>", b"<|a|>"), gap_id=GID, spans=True, special=st, device=True)
    assert out[0].n_matches > len(want[0])   # the tokenizer scan's count: every piece that occurs in a segment
    _same([o.to_numpy() for o in out], want, "device batch, device results")
    for o in out:
        o.free()
    _same(p.tokenize_bpe_docs([], spans=True, special=st), _flat([], []), "no document")
    _same(p.tokenize_bpe_docs([b"", b""], spans=True, special=st), _flat([[], []], [[], []]), "empty documents")
    with pytest.raises(da.DaachorseError) as ei:
        p.tokenize_bpe_docs(docs, special="<|a|>")
    assert ei.value.code == 1 and "SpecialTokens" in str(ei.value)


def test_bpe_docs_without_specials_are_the_direct_chain(bpe):
    p, _ = bpe
    docs = sg.docs()
    got = p.tokenize_bpe_docs(docs, gap_id=GID, spans=True, special=None)
    _same(got, p.tokenize_bpe_docs(docs, gap_id=GID, spans=True), "special=None is the default")
    batch = _device_batch(docs)
    wo, dw = da.split_batch(batch, Split.Gpt2, device=True)
    ids, word_tok = p.tokenize_bpe_batch((batch[0], torch.from_numpy(wo.to_numpy().astype(np.int64)).cuda()), gap=Gap.Bytes, gap_id=GID, device=True)
    doc_tok = da.offsets_compose(word_tok, dw)
    _same((got[0], got[2]), (ids.to_numpy(), doc_tok), "split_batch, tokenize_bpe_batch, offsets_compose")
    per_doc = [got[0][int(a):int(b)].tolist() for a, b in zip(got[2], got[2][1:])]
    ignored = sum(x != y for x, y in zip(per_doc, sg.load()["bpe_ids"]))
    assert ignored >= 30   # the text is ordinary characters there: what the fixture's maker counted
    for o in (wo, dw, ids, word_tok):
        o.free()


# ------------------------------------------------------------------------------------------------------------ 5. WordPiece
@pytest.fixture(scope="module")
def wordpiece():
    patterns, first, cont = da.wordpiece_tables(wg.load("vocab")["vocab"])
    _, unk_id, max_chars, _ = wg.model()
    return da.DoubleArrayAhoCorasick.new(patterns), first, cont, unk_id, max_chars


def test_wordpiece_docs_with_specials_and_the_normalizer_equal_tokenizers(wordpiece, specials):
    p, first, cont, unk_id, max_chars = wordpiece
    st, _ = specials["wordpiece"]
    docs, case = sg.docs(), sg.load()
    want = _flat(case["wordpiece_ids"], sg.wordpiece_spans())
    nz = da.bert_normalizer()
    _same(p.tokenize_wordpiece_docs(docs, first, cont, unk_id, max_chars, spans=True, normalizer=nz, special=st), want, "host documents")
    _same(p.tokenize_wordpiece_docs(docs, first, cont, unk_id, max_chars, normalizer=nz, special=st), (want[0], want[2]), "no spans")
    out = p.tokenize_wordpiece_docs(_device_batch(docs, b"[CLS]x", b"[SEP]"), first, cont, unk_id, max_chars, spans=True, device=True, normalizer=nz, special=st)
    _same([o.to_numpy() for o in out], want, "device batch, device results")
    for o in out:
        o.free()
    _same(p.tokenize_wordpiece_docs([], first, cont, unk_id, max_chars, spans=True, normalizer=nz, special=st), _flat([], []), "no document")


def test_wordpiece_docs_with_specials_on_normalized_documents(wordpiece, specials):
    """without the normalizer: the documents whose text segments were normalized beforehand (the specials stay as they are) give the
    ids of BertPreTokenizer + WordPiece — the fixture's, as its maker asserted on every document"""
    import normalize_golden as ng
    p, first, cont, unk_id, max_chars = wordpiece
    st, spec = specials["wordpiece"]
    docs, case = sg.docs(), sg.load()
    normalized = []
    for d in docs:
        so, _, sv = _want_cut([d], spec)
        normalized.append(b"".join(d[int(a):int(b)] if v != sg.TEXT else ng.bert_scan(d[int(a):int(b)], ng.OPTIONS["default"])[0] for a, b, v in zip(so, so[1:], sv)))
    assert sum(a != b for a, b in zip(docs, normalized)) > 50
    ids, off = p.tokenize_wordpiece_docs(normalized, first, cont, unk_id, max_chars, special=st)
    want = _flat(case["wordpiece_ids"], [[]] * len(docs))
    _same((ids, off), (want[0], want[2]), "normalized documents")


# ------------------------------------------------------------------------------------------------------- 6. a caller's stream
@pytest.fixture(scope="module")
def delay():
    return _Delay()


def _behind_a_delay(delay, real, decoy, call):
    """`call(batch, stream)` on a fresh stream on which a delay and, behind it, the copies of the real inputs over the decoys are queued"""
    s = torch.cuda.Stream()
    dev = [torch.from_numpy(a.copy()).cuda() for a in decoy]
    src = [torch.from_numpy(a.copy()).pin_memory() for a in real]
    torch.cuda.synchronize()
    with _no_collection():
        with torch.cuda.stream(s):
            delay.queue()
            for d, r in zip(dev, src):
                d.copy_(r, non_blocking=True)
        return call(dev, _h(s))


def test_the_new_calls_on_a_busy_callers_stream(delay, bpe, specials, csr):
    p, _ = bpe
    st, spec = specials["bpe"]
    docs = sg.docs()[:200]
    other = [d.replace(b"<|a|>", b"<|x|>").replace(b"the", b"teh") for d in docs[100:] + docs[:100]]
    hay_r, off_r = (t.cpu().numpy() for t in _device_batch(docs, b"<|a", b"|>"))
    hay_d, off_d = (t.cpu().numpy() for t in _device_batch(other, b"<|a", b"|>"))
    hay_d = np.resize(hay_d, hay_r.shape)
    off_d = np.minimum(off_d, off_r[-1])
    off_d[-1] = off_r[-1]
    assert not np.array_equal(off_r, off_d) and np.all(np.diff(off_d) >= 0)
    want_cut = st.cut_batch((torch.from_numpy(hay_r).cuda(), torch.from_numpy(off_r).cuda()))
    _same(want_cut, _want_cut(docs, spec, base=3), "the default stream")
    got = _behind_a_delay(delay, (hay_r, off_r), (hay_d, off_d), lambda dev, s: st.cut_batch((dev[0], dev[1]), stream=s))
    _same(got, want_cut, "cut_batch on a busy stream")
    want_tok = p.tokenize_bpe_docs((torch.from_numpy(hay_r).cuda(), torch.from_numpy(off_r).cuda()), gap_id=GID, spans=True, special=st)
    got = _behind_a_delay(delay, (hay_r, off_r), (hay_d, off_d), lambda dev, s: p.tokenize_bpe_docs((dev[0], dev[1]), gap_id=GID, spans=True, special=st, stream=s))
    _same(got, want_tok, "tokenize_bpe_docs(special=) on a busy stream")
    # the splice: every input is a decoy (zeros) until the copies behind the delay have run
    names = ("ids", "spans", "seg_tok", "seg_offsets", "doc_segs", "values", "doc_offsets")
    real = [csr[k].view({4: np.int32, 8: np.int64}[csr[k].dtype.itemsize]) for k in names]
    decoy = [np.zeros_like(a) for a in real]
    hay = torch.zeros(csr["hay_len"], dtype=torch.uint8, device="cuda")
    got = _behind_a_delay(delay, real, decoy, lambda dev, s: da.splice_special(dev[0], dev[1], dev[2], (dev[3], dev[4], dev[5]), (hay, dev[6]), stream=s))
    _same(got, csr["want"], "splice_special on a busy stream")
