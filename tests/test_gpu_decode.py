"""Token ids back to text on the MI355X (daac_tokens_decode; Decoder.decode_batch / decode).  The expected texts come from `tokenizers`'
own results in tests/golden/decode_cases.json (make_decode_golden.py writes them) and from the pure-Python definition
(tests/decode_golden.py), which test_decode_host.py ties to the fixture; nothing here reads the library under test for its
expectations, and every comparison is exact.

Shapes are the smallest that cross the copy kernel's boundaries: a lane owns 16 output bytes and a workgroup a tile of 4 096, so texts
of 0, 1, 15, 16, 17, 4 095, 4 096, 4 097 and 8 193 bytes, an image across a lane's and a tile's edge, one of 5 000 bytes over whole
tiles, tiles of 1-byte tokens (the 4 096 starts the LDS stage holds) and of empty images besides (more), 6 000 skipped tokens in a row, batches of 1, 2, 257
and 1 031 documents, no document at all, and one text just above 4 GiB.  The call on a caller's busy stream is
tests/test_gpu_tokens_decode_stream.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import decode_golden as dg
import normalize_golden as ng
import tokenizer_golden as tg
import wordpiece_golden as wg
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

import daachorse_amd as da
from daachorse_amd import Gap, Split, _ffi, synth

TILE = 4096


def _flat(docs, dtype=np.uint32):
    return np.array([i for d in docs for i in d], dtype=dtype), np.cumsum([0] + [len(d) for d in docs]).astype(np.uint64)


_decoders = {}


def _decoder(name):
    if name not in _decoders:
        _decoders[name] = dg.library_decoder(name)
    return _decoders[name]


# ------------------------------------------------------------------------------------------------------------- 1. the fixture
@pytest.mark.parametrize("dtype", [np.int32, np.int64], ids=["int32", "int64"])
@pytest.mark.parametrize("form", ["csr", "right", "left"])
@pytest.mark.parametrize("skip", [True, False], ids=["skip_special", "all_tokens"])
@pytest.mark.parametrize("name", dg.NAMES)
def test_decode_on_the_fixture(name, skip, form, dtype):
    """every case of the fixture, one batch per tokenizer: `tokenizers`' recorded text where the case is not lossy and the form holds the
    case's own tokens only (CSR, or padding that is skipped); the definition otherwise"""
    mine = [c for c in dg.cases() if c[0] == name]
    docs = [c[1] for c in mine]
    rows = docs if form == "csr" else dg.padded(docs, dg.pad_id(name), left=form == "left")
    tokens = _flat(rows, dtype) if form == "csr" else np.array(rows, dtype=dtype)
    got = _decoder(name).decode_batch(tokens, skip_special_tokens=skip)
    want = dg.decode_batch(dg.table(name), rows, skip_special=skip)[0]
    assert got == want, (name, skip, form)
    if form == "csr" or skip:
        for c, g in zip(mine, got):
            assert c[3] or g == c[2][skip].encode(), (name, c[1])
    assert _ffi.last_kernel().startswith(f"decode docs={len(docs)} tokens={sum(len(r) for r in rows)} kept=")
    if form == "csr":
        assert _decoder(name).decode(docs[0], skip_special_tokens=skip) == want[0]


# ---------------------------------------------------------------------------------------------------------- 2. boundaries
N_SEEDED, ONE, BIG, SKIP = 64, 64, 65, 66   # ids 0 .. 63: seeded images of 0 .. 40 bytes; a 1-byte image; 5 000 bytes; a special


def _seeded_table():
    rng = np.random.default_rng(20261021)
    rest = [bytes(rng.integers(0, 256, size=int(n), dtype=np.uint8)) for n in rng.integers(0, 41, size=N_SEEDED)]
    rest[3], rest[7], rest[40] = b"", b"", bytes(range(100, 140))   # empty images for sure, and one of 40 bytes
    first = {i: bytes(rng.integers(0, 256, size=int(n), dtype=np.uint8)) for i, n in zip(range(0, N_SEEDED, 2), rng.integers(0, 9, size=N_SEEDED // 2))}
    rest += [b"\x2a", bytes((i * 7 + (i >> 8)) & 0xFF for i in range(5000)), b"<skipped>"]
    table = ({i: r for i, r in enumerate(rest)}, {i: first.get(i, r) for i, r in enumerate(rest)}, {SKIP})
    return da.Decoder(rest, first, special=[SKIP]), table


@pytest.fixture(scope="module")
def seeded():
    return _seeded_table()


def _check(dec, table, docs, dense=None, dtype=np.uint32, **kw):
    """decode_batch with token_starts over CSR (dense=None) or a plane padded with SKIP on the given side, against the definition"""
    rows = docs if dense is None else dg.padded(docs, SKIP, left=dense == "left")
    tokens = _flat(rows, dtype) if dense is None else np.array(rows, dtype=dtype).reshape(len(rows), -1)
    got, starts = dec.decode_batch(tokens, token_starts=True, **kw)
    want, want_starts = dg.decode_batch(table, rows, skip_special=kw.get("skip_special_tokens", True), unknown=kw.get("unknown", "error"))
    assert got == want, [(i, len(g), len(w)) for i, (g, w) in enumerate(zip(got, want)) if g != w][:5]
    assert starts.dtype == np.uint64 and starts.tolist() == want_starts
    return got


def _doc_of_bytes(table, total, seed):
    """a seeded document whose text has exactly `total` bytes: seeded tokens while they fit, then 1-byte tokens"""
    rng = np.random.default_rng(seed)
    doc, size = [], 0
    while True:
        i = int(rng.integers(0, N_SEEDED))
        n = len(table[0][i] if doc else table[1][i])
        if size + n > total:
            break
        doc.append(i)
        size += n
        if len(doc) > 4 * total + 8:
            break
    if not doc and total:
        doc, size = [ONE], len(table[1][ONE])
    return doc + [ONE] * (total - size)


@pytest.mark.parametrize("total", [0, 1, 15, 16, 17, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_texts_around_a_lane_and_a_tile(seeded, total):
    dec, table = seeded
    doc = _doc_of_bytes(table, total, total)
    got = _check(dec, table, [doc])
    assert len(got[0]) == total
    _check(dec, table, [doc], dense="right", dtype=np.int64)
    _check(dec, table, [[SKIP], doc, [], doc[::-1]], dense="left", dtype=np.int32)


def test_images_across_edges_long_images_and_crowded_tiles(seeded):
    dec, table = seeded
    docs = [[ONE] * (TILE - 6) + [40, 40, 5],                    # a 40-byte image across the tile's edge (and across lanes' edges)
            [ONE] * 10 + [BIG, BIG, 3, 5],                        # 5 000 bytes: whole tiles of one image, twice
            [ONE] * 5000,                                         # a tile of 4 096 tokens: as many starts as the stage holds
            [3, 7] * 3000 + [9] + [3] * 2500 + [ONE] * 3000,      # empty images in runs among them: more starts than the stage holds
            [BIG]]
    got = _check(dec, table, docs)
    assert len(got[2]) == 5000 and got[4] == table[1][BIG]
    _check(dec, table, docs[:2], dense="right", dtype=np.int64)


def test_six_thousand_skipped_tokens_in_a_row(seeded):
    """in the middle of a document, at its end and as a whole document, whose text is empty between non-empty neighbours"""
    dec, table = seeded
    docs = [[ONE, 2] + [SKIP] * 6000 + [5, 6], [ONE, 9] + [SKIP] * 6000, [SKIP] * 6000, [SKIP] * 6000 + [ONE], [12]]
    got = _check(dec, table, docs)
    assert got[2] == b"" and got[1].startswith(b"\x2a") and got[3] == b"\x2a"
    _check(dec, table, docs, skip_special_tokens=False)
    _check(dec, table, docs, dense="right", dtype=np.int64)


@pytest.mark.parametrize("n", [1, 2, 257, 1031])
def test_batches_across_workgroups(seeded, n):
    dec, table = seeded
    rng = np.random.default_rng(n)
    docs = [rng.integers(0, SKIP + 1, size=int(k)).tolist() for k in rng.integers(0, 13, size=n)]
    _check(dec, table, docs)
    _check(dec, table, docs, dense="left", dtype=np.int32, skip_special_tokens=False)
    _check(dec, table, docs, dense="right", dtype=np.int64)


def test_no_document(seeded):
    dec, _ = seeded
    assert dec.decode_batch((np.zeros(0, dtype=np.uint32), np.zeros(1, dtype=np.uint64))) == []
    assert dec.decode_batch(np.zeros((0, 5), dtype=np.int64)) == [] and _ffi.last_kernel() == "decode docs=0 tokens=0 kept=0 bytes=0"
    out, off = dec.decode_batch((np.zeros(0, dtype=np.uint32), np.zeros(1, dtype=np.uint64)), device=True)
    assert (out.ptr, out.count, off.to_numpy().tolist()) == (None, 0, [0])
    off.free()
    assert dec.decode_batch(([], [0, 0, 0])) == [b"", b""] and dec.decode([]) == b""   # documents, none with a token


# --------------------------------------------------------------------------------------------------------------- 3. errors
class _Raw:
    """daac_tokens_decode over device tensors, with its out-pointers in hand"""

    def __init__(self, dec, ids, off=None):
        self.dec = dec
        self.ids = torch.from_numpy(np.ascontiguousarray(ids).view(np.int32 if ids.dtype.itemsize == 4 else np.int64).copy()).cuda()
        self.off = None if off is None else torch.from_numpy(np.asarray(off).astype(np.int64)).cuda()
        self.shape = ids.shape
        self.outs = [C.c_void_p(1), C.c_void_p(1), C.c_void_p(1)]
        self.bytes = C.c_uint64(1)

    def run(self, unknown_skip=0, starts=True):
        csr = self.off is not None
        return _ffi.lib().daac_tokens_decode(self.dec._h, self.ids.data_ptr(), self.ids.dtype.itemsize, self.off.data_ptr() if csr else None, self.ids.numel() if csr else 0,
                                             self.off.numel() - 1 if csr else self.shape[0], 0 if csr else self.shape[1], 1, unknown_skip, None,
                                             C.byref(self.outs[0]), C.byref(self.outs[1]), C.byref(self.outs[2]) if starts else None, C.byref(self.bytes))

    def cleared(self, starts=True):
        return all(o.value is None for o in self.outs[:3 if starts else 2]) and self.bytes.value == 0


def test_the_lowest_unknown_token_is_named_and_nothing_is_handed_over(seeded):
    dec, table = seeded
    rng = np.random.default_rng(5)
    docs = [rng.integers(0, N_SEEDED, size=int(k)).tolist() for k in rng.integers(1, 9, size=700)]   # several workgroups
    for d, k in ((311, 0), (650, 0), (699, 0)):
        docs[d][k] = 9999
    ids, off = _flat(docs)
    r = _Raw(dec, ids, off)
    assert r.run() == 1 and r.cleared()
    msg = _ffi.lib().daac_last_error().decode()
    assert msg.startswith(f"document 311, token {int(off[311])}:"), msg
    with pytest.raises(dg.DecodeError) as ei:
        dg.decode_batch(table, docs)
    assert ei.value.token == int(off[311])
    with pytest.raises(da.DaachorseError) as ei:
        dec.decode_batch((ids, off))
    assert ei.value.code == 1 and "document 311" in str(ei.value)
    _check(dec, table, docs, unknown="skip")
    # an empty document in front of the token shares its offset: the document that holds the token is named
    docs2 = [[1], [], [], [9999, 2], [3]]
    with pytest.raises(da.DaachorseError) as ei:
        dec.decode_batch(_flat(docs2))
    assert "document 3, token 1:" in str(ei.value)
    # -100 and 2^32 in an int64 plane, an absent id in an int32 one
    plane = np.array(dg.padded(docs[:400], SKIP), dtype=np.int64)
    L = plane.shape[1]
    plane[200, 1], plane[100, 0], plane[399, 0] = -100, 1 << 32, (1 << 32) + 5
    r = _Raw(dec, plane)
    assert r.run() == 1 and r.cleared()
    msg = _ffi.lib().daac_last_error().decode()
    assert msg.startswith(f"document 100, token {100 * L} (column 0):"), msg
    plane[100, 0] = 5
    with pytest.raises(da.DaachorseError) as ei:
        dec.decode_batch(plane)
    assert f"document 200, token {200 * L + 1} (column 1)" in str(ei.value)
    got = dec.decode_batch(plane, unknown="skip")
    assert got == dg.decode_batch(table, plane.tolist(), unknown="skip")[0]
    holes = da.Decoder(["a", None, "c"])
    with pytest.raises(da.DaachorseError) as ei:
        holes.decode_batch(np.array([[0, 2], [1, 0]], dtype=np.int32))
    assert "document 1, token 2 (column 0)" in str(ei.value)
    assert holes.decode_batch(np.array([[0, 2], [1, 0]], dtype=np.uint32), unknown="skip") == [b"ac", b"a"]


def test_offsets_in_error_name_the_first_bad_document(seeded):
    dec, table = seeded
    rng = np.random.default_rng(6)
    docs = [rng.integers(0, N_SEEDED, size=int(k)).tolist() for k in rng.integers(1, 9, size=700)]
    docs[50][0] = 9999   # an unknown token too: the offsets are answered first
    ids, off = _flat(docs)
    bad = off.copy()
    bad[401] = off[-1] + 1
    bad[100] = 0
    r = _Raw(dec, ids, bad)
    assert r.run() == 1 and r.cleared()
    msg = _ffi.lib().daac_last_error().decode()
    assert msg.startswith("document 99: its token offsets"), msg
    bad[100] = off[100]
    assert _Raw(dec, ids, bad).run() == 1 and _ffi.lib().daac_last_error().decode().startswith("document 400: its token offsets")
    with pytest.raises(da.DaachorseError) as ei:
        dec.decode_batch((ids, bad))
    assert ei.value.code == 1 and "document 400" in str(ei.value)


def test_max_result_bytes_and_what_a_call_leaves_behind(seeded):
    dec, table = seeded
    docs = [_doc_of_bytes(table, 700, 1), [], _doc_of_bytes(table, 300, 2)]
    ids, off = _flat(docs)
    want = dg.decode_batch(table, docs)[0]
    for limit, ok in ((999, False), (1000, True)):
        da.set_option("max_result_bytes", limit)
        try:
            if ok:
                assert dec.decode_batch((ids, off)) == want
            else:
                r = _Raw(dec, ids, off)
                assert r.run(starts=False) == 2 and r.cleared(starts=False) and "max_result_bytes" in _ffi.lib().daac_last_error().decode()
        finally:
            da.set_option("max_result_bytes", 8 << 30)
    # nothing leaks: device results are the caller's to free, a refused call hands out nothing.  A round's text has 64 MB, so that
    # twenty rounds that kept theirs would take 1.3 GB; the margin of 256 MB is for whoever else allocates on the card meanwhile
    docs = [[BIG] * 6400, [], [BIG] * 6400]
    ids, off = _flat(docs)
    d_ids, d_off = torch.from_numpy(ids.view(np.int32).copy()).cuda(), torch.from_numpy(off.astype(np.int64)).cuda()
    bad = d_ids.clone()
    bad[2] = 9999

    def round_():
        out = dec.decode_batch((d_ids, d_off), token_starts=True, device=True)
        assert out[0].count == 12800 * 5000 and out[1].count == 4 and out[2].count == len(ids) + 1
        for o in out:
            o.free()
            assert o.ptr is None
        with pytest.raises(da.DaachorseError):
            dec.decode_batch((bad, d_off), device=True)

    round_()
    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info()[0]
    for _ in range(20):
        round_()
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] >= free_before - (256 << 20)


# ----------------------------------------------------------------------------------------------------------- 4. round trips
def _soup_batch(n_docs, seed):
    """seeded word soup cut into documents of seeded lengths (0 .. 200 bytes) -> (bytes, offsets)"""
    words = synth.patterns_cfg3(2000)
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 201, size=n_docs)
    lens[::97] = 0
    off = np.zeros(n_docs + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    hay = synth.wordsoup_haystack(int(off[-1]), synth.SEEDS["cfg3_dense"], words, 20)
    return np.array(hay, dtype=np.uint8), off


def _bpe_pma():
    pieces = tg.bpe_pieces()
    o = orc.OraclePma.build(pieces, values=np.arange(len(pieces), dtype=np.uint32))
    pma, rest = da.DoubleArrayAhoCorasick.deserialize(o.serialize())
    assert rest == b""
    return pma, pieces


def test_byte_level_round_trip_gives_the_input_batch_back():
    """tokenize_bpe_docs(device=True) and back: bytes and offsets equal the input, with no library involved"""
    pma, pieces = _bpe_pma()
    hay, off = _soup_batch(3000, 7)
    batch = (torch.from_numpy(hay).cuda(), torch.from_numpy(off).cuda())
    dec = da.Decoder.byte_level(pieces)
    toks = pma.tokenize_bpe_docs(batch, split=Split.Gpt2, gap=Gap.Bytes, gap_id=1 << 20, device=True)
    out, out_off = dec.decode_batch(toks, device=True)
    assert out.count == len(hay) and np.array_equal(out.to_numpy(), hay) and np.array_equal(out_off.to_numpy(), off.astype(np.uint64))
    # the result is a batch again: it goes straight back into the tokenizer
    again = pma.tokenize_bpe_docs((_as_tensor(out), out_off), split=Split.Gpt2, gap_id=1 << 20, device=True)
    assert np.array_equal(again[0].to_numpy(), toks[0].to_numpy()) and np.array_equal(again[-1].to_numpy(), toks[-1].to_numpy())
    for o in (out, out_off) + tuple(toks) + tuple(again):
        o.free()
    # the same through pack=: <s> A </s>, rows padded to the longest, the template's ids flagged special
    n = len(pieces)
    spec = da.SpecialTokens({"<s>": n, "</s>": n + 1, "<pad>": n + 2})
    dec = da.Decoder.byte_level(pieces, special=spec)
    for dtype in (np.int64, np.int32):
        x = pma.tokenize_bpe_docs(batch, split=Split.Gpt2, gap_id=1 << 20, pack=da.Packer(da.roberta_template(n, n + 1), padding="longest", pad_id=n + 2, dtype=dtype), device=True)
        got = dec.decode_batch(x["input_ids"], skip_special_tokens=True)
        assert got == [hay[off[d]:off[d + 1]].tobytes() for d in range(len(off) - 1)]
        first = dec.decode_batch(x["input_ids"], skip_special_tokens=False)[0]
        assert first.startswith(b"<s>" + got[0] + b"</s>") and first.endswith(b"<pad>")
        for v in x.values():
            v.free()


def _as_tensor(m):
    """a DeviceMatches of bytes as a CUDA tensor of its own (a copy through the host: the test's plumbing, not the library's)"""
    return torch.from_numpy(m.to_numpy()).cuda()


def test_wordpiece_pipeline_and_back_equals_tokenizers_decode():
    """normalize, split, WordPiece and pack on the device, then decode: the strings `tokenizers` gives for exactly that pipeline"""
    pipe = dg.load()["bert_pipeline"]
    spec = {t: i for t, i in pipe["specials"]}
    vocab = wg.load("vocab")["vocab"]
    patterns, first, cont = da.wordpiece_tables(vocab)
    _, unk_id, max_chars, _ = wg.model()
    pma = da.DoubleArrayAhoCorasick.new(patterns)
    docs = ng.docs()
    packer = da.Packer(da.bert_template(spec["[CLS]"], spec["[SEP]"]), max_length=pipe["max_length"], pad_id=spec["[PAD]"])
    x = pma.tokenize_wordpiece_docs(docs, first, cont, unk_id, max_chars, normalizer=da.bert_normalizer(), pack=packer, device=True)
    assert x["input_ids"].shape == (len(docs), pipe["row_length"])
    dec = da.Decoder.wordpiece(vocab, special=da.SpecialTokens(spec))
    got = dec.decode_batch(x["input_ids"])
    for v in x.values():
        v.free()
    assert got == [t.encode() for t in pipe["text"]]


# ------------------------------------------------------------------------------------------------------------ 5. past 2^32
def test_a_text_just_above_four_gib():
    """one 1 100-byte image whose bytes depend on their position and a few short ones; the text crosses 2^32 inside a document.  64 KiB
    windows around byte 2^32, around every document's edge and at the end against the definition evaluated there; out_offsets exact"""
    long_img = bytes((i * 13 + (i >> 8) * 7 + (i >> 4)) & 0xFF for i in range(1100))
    rest = [long_img, b"ab", b"", b"xyz", b"<s>"]
    first = {0: long_img[1:], 1: b"B", 3: b"yz"}
    dec = da.Decoder(rest, first, special=[4])
    imgs_rest = [np.frombuffer(r, dtype=np.uint8) for r in rest]
    imgs_first = [np.frombuffer(first.get(i, r), dtype=np.uint8) for i, r in enumerate(rest)]
    rng = np.random.default_rng(32)
    T = (1 << 32) // 1100 + 200_000   # (a fiftieth of the tokens is short: the rest still passes 2^32)
    ids = np.zeros(T, dtype=np.uint32)
    at = rng.integers(0, T, size=T // 50)
    ids[at] = rng.integers(1, 5, size=len(at))
    doc_off = np.array([0, 5, 5, T // 3, T - 40_000, T - 40_000 + 1, T], dtype=np.uint64)
    ids[[0, 5, T // 3]] = [4, 1, 3]   # a special first: the document's first KEPT token is the next one
    n = len(doc_off) - 1
    # the definition, in numpy: every token's length and start
    kept = ids != 4
    is_first = np.zeros(T, dtype=bool)
    for d in range(n):
        t0, t1 = int(doc_off[d]), int(doc_off[d + 1])
        k = np.flatnonzero(kept[t0:t1])
        if len(k):
            is_first[t0 + k[0]] = True
    len_rest, len_first = np.array([len(r) for r in imgs_rest], dtype=np.uint64), np.array([len(r) for r in imgs_first], dtype=np.uint64)
    lens = np.where(is_first, len_first[ids], len_rest[ids]) * kept
    starts = np.zeros(T + 1, dtype=np.uint64)
    starts[1:] = np.cumsum(lens, dtype=np.uint64)
    total = int(starts[-1])
    assert total > (1 << 32) + (1 << 20) and int(starts[int(doc_off[3])]) < (1 << 32) < int(starts[int(doc_off[4])])

    def window(lo, size):
        q = np.arange(lo, lo + size, dtype=np.uint64)
        tok = np.searchsorted(starts, q, side="right") - 1
        d = (q - starts[tok]).astype(np.int64)
        out = np.zeros(size, dtype=np.uint8)
        for i in range(len(rest)):
            for table, sel in ((imgs_rest, ~is_first[tok]), (imgs_first, is_first[tok])):
                m = (ids[tok] == i) & sel
                if m.any():
                    out[m] = table[i][d[m]]
        return out

    d_ids, d_off = torch.from_numpy(ids.view(np.int32)).cuda(), torch.from_numpy(doc_off.astype(np.int64)).cuda()
    out, out_off = dec.decode_batch((d_ids, d_off), device=True)
    try:
        assert out.count == total and out_off.to_numpy().tolist() == [int(starts[int(t)]) for t in doc_off]
        W = 64 * 1024
        edges = [1 << 32] + [int(starts[int(t)]) for t in doc_off[1:-1]]
        for lo in [0] + [max(0, e - W // 2) for e in edges] + [total - W]:
            lo = min(lo, total - W)
            assert np.array_equal(out.to_numpy(lo, W), window(lo, W)), lo
    finally:
        out.free()
        out_off.free()
