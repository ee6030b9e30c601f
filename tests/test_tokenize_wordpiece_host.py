"""tokenize_wordpiece (daac_tokenize_wordpiece / daac_tokenize_wordpiece_batch) on the host side: the exports, every answer the C ABI and
the Python wrappers give before they touch a device, wordpiece_tables, the fixtures of tests/golden/ against the pure-Python definition
(tests/wordpiece_golden.py), and the kernel file's per-lane bodies run on the CPU under ASan and UBSan (tests/native/wordpiece_check.cpp,
a stand-alone program) over the fixture words and over hostile tuple lists.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as orc
import wordpiece_golden as wg

import daachorse_amd as da
from daachorse_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF


def _pair(patterns, kind=0, charwise=False, values=None):
    if charwise:
        o = orc.OracleCharwisePma.build(patterns, values=values, kind=kind)
        p, rest = da.CharwiseDoubleArrayAhoCorasick.deserialize(o.serialize())
    else:
        o = orc.OraclePma.build(patterns, values=values, kind=kind)
        p, rest = da.DoubleArrayAhoCorasick.deserialize(o.serialize())
    assert rest == b""
    return p


class _Call:
    """the raw arguments of the two calls; the pointers named in `null` go as NULL"""

    def __init__(self, p, batch=False, hay=b"abab", offsets=(0, 2, 4), first=(0, 1), cont=(2, 3), unk_id=9, max_chars=100):
        self.p, self.batch, self.unk_id, self.max_chars = p, batch, unk_id, max_chars
        self.hay = np.frombuffer(hay, dtype=np.uint8)
        self.offsets = None if offsets is None else np.asarray(offsets, dtype=np.uint64)
        self.n = 0 if offsets is None else len(offsets) - 1
        self.first, self.cont = np.asarray(first, dtype=np.uint32), np.asarray(cont, dtype=np.uint32)
        self.n_ids = len(self.first)
        self.ids, self.spans, self.tok_off = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self.n_tokens, self.n_matches = C.c_uint64(), C.c_uint64()
        self.null = set()

    def run(self, engine=0):
        ptr = lambda name, a: None if a is None or name in self.null else a.ctypes.data
        ref = lambda name, v: None if name in self.null else C.byref(v)
        L = _ffi.lib()
        model = (ptr("first", self.first), ptr("cont", self.cont), self.n_ids, self.unk_id, self.max_chars)
        if self.batch:
            return L.daac_tokenize_wordpiece_batch(self.p._h, int(engine), ptr("hay", self.hay), ptr("offsets", self.offsets), self.n, 0, None, *model, None,
                                                   ref("ids", self.ids), ref("spans", self.spans), ref("tok_off", self.tok_off), ref("n_tokens", self.n_tokens),
                                                   ref("n_matches", self.n_matches))
        return L.daac_tokenize_wordpiece(self.p._h, int(engine), ptr("hay", self.hay), len(self.hay), 0, None, *model, ref("ids", self.ids),
                                         ref("spans", self.spans), ref("n_tokens", self.n_tokens), ref("n_matches", self.n_matches))


def _err():
    return _ffi.lib().daac_last_error().decode()


def _wrapper(p, batch, first=(0, 1), cont=(2, 3), unk_id=9, **kw):
    """the Python wrapper on the same text as _Call -> (the status it raises, the message)"""
    with pytest.raises(da.DaachorseError) as ei:
        p.tokenize_wordpiece_batch([b"ab", b"ab"], first, cont, unk_id, **kw) if batch else p.tokenize_wordpiece(b"abab", first, cont, unk_id, **kw)
    return ei.value.code, str(ei.value)


def test_wordpiece_symbols_are_exported():
    lib = C.CDLL(_ffi._build.LIB_PATH)
    for name in ("daac_tokenize_wordpiece", "daac_tokenize_wordpiece_batch", "daac_split_words_space"):
        assert hasattr(lib, name), name
    p = _pair(["ab"])
    for name in ("tokenize_wordpiece", "tokenize_wordpiece_batch", "tokenize_wordpiece_docs"):
        assert callable(getattr(p, name)), name
        assert callable(getattr(da.DoubleArrayAhoCorasick, name)), name
        assert callable(getattr(da.CharwiseDoubleArrayAhoCorasick, name)), name
    assert callable(da.wordpiece_tables) and callable(da.bert_char_classes)
    assert _ffi.lib().daac_abi_version() == 6 == _ffi.ABI_VERSION


@pytest.mark.parametrize("batch", [False, True])
def test_wordpiece_bad_arguments_answer_1_without_a_device(batch):
    p = _pair(["ab", "b"])   # values 0 and 1
    # a NULL required pointer (spans may be NULL: they are not wanted then)
    for name in ("ids", "n_tokens", "n_matches") + (("tok_off",) if batch else ()):
        c = _Call(p, batch)
        c.null.add(name)
        assert c.run() == 1, name
        assert "null" in _err()
    # max_chars: 1 .. 0xFFFFFFFF
    assert _Call(p, batch, max_chars=0).run() == 1 and "max_chars" in _err()
    for bad in (0, -1, 1 << 32):
        code, msg = _wrapper(p, batch, max_chars=bad)
        assert code == 1 and "max_chars" in msg, bad
    # the two id tables
    for name, word in (("first", "first_ids"), ("cont", "cont_ids")):
        c = _Call(p, batch)
        c.null.add(name)
        assert c.run() == 1 and word in _err(), name
    code, msg = _wrapper(p, batch, first=None)
    assert code == 1 and "first_ids" in msg
    code, msg = _wrapper(p, batch, cont=None)
    assert code == 1 and "cont_ids" in msg
    for bad in ([[0, 1]], [0.5, 1.0], [-1, 0], [0, 1 << 32]):   # what the wrapper itself refuses as a table
        assert _wrapper(p, batch, first=bad)[0] == 1 and "first_ids" in _wrapper(p, batch, first=bad)[1], bad
        assert _wrapper(p, batch, cont=bad)[0] == 1 and "cont_ids" in _wrapper(p, batch, cont=bad)[1], bad
    code, msg = _wrapper(p, batch, first=(0, 1, 2))
    assert code == 1 and "first_ids" in msg and "cont_ids" in msg   # two lengths
    for bad in (-1, 1 << 32):
        code, msg = _wrapper(p, batch, unk_id=bad)
        assert code == 1 and "unk_id" in msg
    # the tables must reach the largest value among the outputs
    assert _Call(p, batch, first=(5,), cont=(6,)).run() == 1 and "n_ids" in _err()
    code, msg = _wrapper(p, batch, first=[5], cont=[6])
    assert code == 1 and "n_ids" in msg
    big = _pair(["ab", "b"], values=[3, 1000])
    assert _Call(big, batch, first=[0] * 1000, cont=[0] * 1000).run() == 1 and "1000" in _err()
    code, msg = _wrapper(big, batch, first=[0] * 1000, cont=[0] * 1000)
    assert code == 1 and "n_ids" in msg
    if batch:   # the batch calls' own offset rules
        assert _Call(p, True, offsets=(0, 3, 2)).run() == 1
        assert "document 1" in _err()
        c = _Call(p, True)
        c.null.add("offsets")
        assert c.run() == 1 and "offsets" in _err()
        c = _Call(p, True)
        c.null.add("hay")
        assert c.run() == 1 and "hay" in _err()
    else:
        c = _Call(p, False)
        c.null.add("hay")
        assert c.run() == 1 and "hay" in _err()


@pytest.mark.parametrize("batch", [False, True])
def test_wordpiece_leftmost_automata_answer_5_without_a_device(batch):
    lefts = [_pair(["ab", "b"], kind=1), _pair(["ab", "b"], kind=2), _pair(["世界", "界"], kind=1, charwise=True), _pair(["世界", "界"], kind=2, charwise=True)]
    for p in lefts:
        assert _Call(p, batch).run() == 5
        assert "standard" in _err()
        assert _wrapper(p, batch)[0] == 5
        assert _wrapper(p, batch, spans=True, max_chars=1)[0] == 5
        # every status-1 family is answered before 5 is looked at
        c = _Call(p, batch)
        c.null.add("n_tokens")
        assert c.run() == 1
        assert _Call(p, batch, max_chars=0).run() == 1
        c = _Call(p, batch)
        c.null.add("cont")
        assert c.run() == 1
        assert _Call(p, batch, first=(0,), cont=(0,)).run() == 1
        if batch:
            assert _Call(p, True, offsets=(0, 3, 2)).run() == 1


def test_wordpiece_documents_of_2_32_minus_1_bytes_answer_6_without_a_device():
    """positions are kept in 32 bits: the length alone decides, before the text is looked at"""
    p = _pair(["ab", "b"])
    c = _Call(p, True, offsets=(0, 2, 2 + 0xFFFFFFFF))
    assert c.run() == 6 and "document 1" in _err() and "4294967295 bytes" in _err()
    L = _ffi.lib()
    first, cont = np.array([0, 1], dtype=np.uint32), np.array([2, 3], dtype=np.uint32)
    ids, n, k = C.c_void_p(), C.c_uint64(), C.c_uint64()
    for length, want in ((0xFFFFFFFF, 6), (0x100000000, 6)):
        assert L.daac_tokenize_wordpiece(p._h, 0, c.hay.ctypes.data, length, 0, None, first.ctypes.data, cont.ctypes.data, 2, 9, 100, C.byref(ids), None,
                                         C.byref(n), C.byref(k)) == want, length
        assert "document 0" in _err()
    # a leftmost automaton answers 5 whatever the length
    q = _pair(["ab", "b"], kind=1)
    assert _Call(q, True, offsets=(0, 2, 2 + 0xFFFFFFFF)).run() == 5


def test_wordpiece_tables_on_a_hand_vocabulary():
    vocab = {"[UNK]": 0, "un": 1, "##able": 2, "able": 3, "##s": 4, "##": 5, "a": 6, "##a": 7, "##ing": 8}
    patterns, first, cont = da.wordpiece_tables(vocab)
    want = sorted([b"[UNK]", b"un", b"##able", b"able", b"##s", b"##", b"a", b"##a", b"##ing", b"s", b"ing"])
    assert patterns == want and first.dtype == cont.dtype == np.uint32 and len(first) == len(cont) == len(want)
    f, c = dict(zip(patterns, first.tolist())), dict(zip(patterns, cont.tolist()))
    assert f[b"able"] == 3 and c[b"able"] == 2          # both roles
    assert f[b"ing"] == NONE and c[b"ing"] == 8         # a continuation only
    assert f[b"un"] == 1 and c[b"un"] == NONE           # an initial piece only
    assert f[b"##s"] == 4 and c[b"##s"] == NONE         # a key with the prefix is also an initial piece of the literal word "##s"
    assert f[b"##"] == 5 and c[b"##"] == NONE and b"" not in patterns   # a key equal to the prefix: no empty pattern
    assert f[b"a"] == 6 and c[b"a"] == 7 and f[b"##a"] == 7 and c[b"##a"] == NONE
    # bytes keys and another prefix
    p2, f2, c2 = da.wordpiece_tables({b"x": 0, b"@@y": 1, b"@@": 2}, prefix="@@")
    assert p2 == [b"@@", b"@@y", b"x", b"y"] and f2.tolist() == [2, 1, 0, NONE] and c2.tolist() == [NONE, NONE, NONE, 1]
    # it is tokenizers' lookup: the pure-Python definition over the tables gives the definition over the vocabulary
    v = {k.encode(): i for k, i in vocab.items()}
    for w in (b"unable", b"ables", b"##s", b"as", b"aa", b"unx", b"ingun", b"a##"):
        out, pos = [], 0
        while pos < len(w):
            for e in range(len(w), pos, -1):
                i = (c if pos else f).get(w[pos:e], NONE)
                if i != NONE:
                    out.append((i, pos, e))
                    pos = e
                    break
            else:
                out = [(0, 0, len(w))]
                break
        assert out == wg.wordpiece(w, v, 0, 100), w
    for bad in ({"a": -1}, {"a": NONE}, {"": 1}):
        with pytest.raises(da.DaachorseError) as ei:
            da.wordpiece_tables(bad)
        assert ei.value.code == 1
    with pytest.raises(da.DaachorseError):
        da.wordpiece_tables({"a": 0}, prefix="")


def test_wordpiece_fixtures_against_the_definition():
    """the committed cases say what `tokenizers` gave; the pure-Python definition gives the same on every document"""
    for name in ("vocab", "cases"):
        f = wg.load(name)
        assert set(f["versions"]) == {"tokenizers", "unidata_version"}, name
        assert os.path.getsize(os.path.join(wg.GOLDEN, f"tokenizer_wordpiece_{name}.json")) <= 64 * 1024
    vocab, unk_id, max_chars, prefix = wg.model()
    docs, ids, tok_spans, word_spans = wg.cases()
    assert max_chars == 16 and prefix == "##" and 1000 <= len(vocab) <= 1200 and len(docs) >= 257 and len(docs) == len(ids) == len(tok_spans) == len(word_spans)
    s = wg.load("cases")["sensitivity"]
    assert s["words_with_two_or_more_pieces"] >= 200 and s["distinct_words_changed_by_ignoring_roles"] >= 10
    assert s["distinct_words_with_a_first_piece_that_fail_later"] >= 10 and s["words_above_max_chars"] >= 5
    assert s["words_within_max_chars_but_more_bytes"] >= 5 and s["distinct_words_changed_by_shortest_first"] >= 10
    assert s["words_unk"] * 10 <= s["words"]
    table = wg.class_table(da.bert_char_classes())
    n_words = n_unk = 0
    for d, want_ids, want_spans, ws in zip(docs, ids, tok_spans, word_spans):
        assert not any(b < 0x20 and b not in (9, 10, 11, 12, 13) for b in d)
        assert [(s_, e) for s_, e, sp in wg.bert_scan(d, table) if not sp] == ws, d
        got_ids, got_spans = wg.wordpiece_doc(d, table, vocab, unk_id, max_chars, prefix.encode())
        assert got_ids == want_ids and got_spans == want_spans, d
        n_words += len(ws)
        n_unk += sum(wg.wordpiece(d[a:b], vocab, unk_id, max_chars) == [(unk_id, 0, b - a)] for a, b in ws)
    assert (n_words, n_unk) == (s["words"], s["words_unk"])
    # the tables of the fixture vocabulary give the same pieces as the vocabulary itself
    patterns, first, cont = da.wordpiece_tables(wg.load("vocab")["vocab"])
    assert len(set(patterns)) == len(patterns) and all(patterns) and int((first != NONE).sum()) == len(vocab)
    assert int((cont != NONE).sum()) == sum(k.startswith(b"##") and len(k) > 2 for k in vocab)


def _exe(tmp_path):
    exe = str(tmp_path / "wordpiece_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-o", exe, os.path.join(ROOT, "tests", "native", "wordpiece_check.cpp")])
    return exe


def test_wordpiece_lane_bodies_on_the_host_under_sanitizers(tmp_path):
    """the count and write bodies of wordpiece_kernels.hip as plain C++: every word of every fixture document (and an empty one) as one
    batch, ids and spans equal to the fixture's; then 2 x 2000 rounds of random words with hostile tuple lists against the definition"""
    exe = _exe(tmp_path)
    vocab, unk_id, max_chars, prefix = wg.model()
    docs, ids, tok_spans, word_spans = wg.cases()
    patterns, first, cont = da.wordpiece_tables(wg.load("vocab")["vocab"])
    lines = [f"M {unk_id} {max_chars}"] + [f"P {p.hex()} {f} {c}" for p, f, c in zip(patterns, first.tolist(), cont.tolist())]
    lines.append("W -")
    for d, ws in zip(docs, word_spans):
        lines += [f"W {d[s:e].hex()}" for s, e in ws]
    path = tmp_path / "words.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, "words", str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.stdout[-2000:], r.stderr[-2000:])
    out = r.stdout.split("\n")[:-1]
    assert out[0] == "" and len(out) == 1 + sum(map(len, word_spans))
    k = 1
    for d, want_ids, want_spans, ws in zip(docs, ids, tok_spans, word_spans):
        got_ids, got_spans = [], []
        for s, _ in ws:
            for tok in out[k].split():
                i, a, b = map(int, tok.split(":"))
                got_ids.append(i)
                got_spans.append((s + a, s + b))
            k += 1
        assert got_ids == want_ids and got_spans == want_spans, d
    for seed in (1, 2):
        r = subprocess.run([exe, "hostile", "2000", str(seed)], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.startswith("OK 2000 rounds") and r.stderr == "", (r.stdout, r.stderr)
