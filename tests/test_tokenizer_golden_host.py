"""The tokenizer fixtures of tests/golden/ (make_tokenizer_golden.py: `tokenizers`' byte-level BPE and sentencepiece's unigram model on
synthetic text) on the host: the fixtures are consistent in themselves, `tokenizers` models rebuilt from the committed lists give the
committed ids again, and the three references that the GPU suites compare the device with (`_bpe` of test_gpu_tokenize_bpe.py,
`_viterbi` of test_gpu_tokenize_unigram.py, `scan_batch` of test_split_host.py) reproduce the libraries' results exactly when they are
fed the CPU oracle's find_overlapping_iter matches.  Every comparison is exact.  No GPU."""
import importlib.util
import os
import unicodedata

import numpy as np
import pytest

from oracle import oracle as orc
from test_gpu_tokenize_bpe import _bpe
from test_gpu_tokenize_unigram import _viterbi
from test_split_host import GPT2_PATTERN, scan_batch
import tokenizer_golden as tg

import daachorse_amd as da
from daachorse_amd import Gap, Split

GID = 1 << 20   # above every id: no token of a byte-level vocabulary may reach it


# ------------------------------------------------------------------------------------------------------ 1. the fixtures themselves
def test_fixture_files_are_small_and_say_where_they_come_from():
    for name in ("bpe_vocab", "bpe_cases", "unigram_vocab", "unigram_cases"):
        f = tg.load(name)
        assert set(f["versions"]) == {"sentencepiece", "tokenizers", "regex", "unidata_version"}, name
    for name in ("bpe_cases", "unigram_cases"):
        assert len(tg.load(name)["docs"]) >= 257 and len(tg.load(name)["docs"]) == len(tg.load(name)["ids"])
    s = {**tg.load("bpe_cases")["sensitivity"], **tg.load("unigram_cases")["sensitivity"]}
    assert s["words_changed_by_rightmost_ties"] >= 10 and s["docs_changed_by_greedy_longest_match"] >= 10
    assert s["docs_with_an_unknown_run"] >= 20 and s["docs_with_an_isolated_unknown"] >= 20
    # the split's classes are the running Python's: the documents hold no code point whose class is younger than Unicode 6.1
    assert tuple(map(int, unicodedata.unidata_version.split("."))) >= (6, 1)


def test_bpe_fixture_is_consistent():
    pieces = tg.bpe_pieces()
    c = tg.load("bpe_cases")
    assert sorted(pieces[:256]) == [bytes([b]) for b in range(256)] and len(set(pieces)) == len(pieces)
    merges = tg.load("bpe_vocab")["merges"]
    assert len(merges) == len(pieces) - 256 >= 1000
    for i, (a, b) in enumerate(merges):   # merge i produces id 256 + i out of two earlier ids: id = rank
        assert a < 256 + i and b < 256 + i and pieces[a] + pieces[b] == pieces[256 + i], i
    words, word_ids = tg.bpe_words()
    assert len(set(words)) == len(words) == len(word_ids)
    of_word = dict(zip(words, word_ids))
    for w, ids in of_word.items():
        assert w and b"".join(pieces[i] for i in ids) == w
    seen = set()
    for d, ids, bounds in zip(c["docs"], c["ids"], c["word_bounds"]):
        raw = d.encode()
        assert all(0 <= i < len(pieces) for i in ids) and b"".join(pieces[i] for i in ids) == raw
        assert bounds[0] == 0 and bounds[-1] == len(raw) and all(x < y for x, y in zip(bounds, bounds[1:]))
        ws = [raw[s:e] for s, e in zip(bounds, bounds[1:])]
        assert sum((of_word[w] for w in ws), []) == ids
        seen.update(ws)
    assert seen == set(words)
    assert c["docs"].count("") >= 2 and c["docs"][-1] == "" and "" in c["docs"][1:-1]


def _follows(text, ids, pieces, unk_id, known_chars):
    """ids spell `text` (a str): a piece is itself, an unk_id is a run of one or more code points that are no piece"""
    at = 0
    for i in ids:
        if i != unk_id:
            if not text.startswith(pieces[i], at):
                return False
            at += len(pieces[i])
        else:
            to = at
            while to < len(text) and text[to] not in known_chars:
                to += 1
            if to == at:
                return False
            at = to
    return at == len(text)


def test_unigram_fixture_is_consistent():
    v, c = tg.load("unigram_vocab"), tg.load("unigram_cases")
    pieces, unk_id = v["pieces"], v["unk_id"]
    pats, values, scores, unk_id2, unk_score = tg.unigram_model()
    assert unk_id == unk_id2 and len(pieces) == len(scores) == len(set(pieces)) and len(pats) == len(pieces) - 1
    assert unk_score.dtype == np.float32 and unk_score == np.float32(min(s for i, s in enumerate(v["scores"]) if i != unk_id)) - np.float32(10)
    assert all(s < 0 for i, s in enumerate(v["scores"]) if i != unk_id) and "▁" in pieces and " " not in "".join(pieces)
    known = {p for i, p in enumerate(pieces) if len(p) == 1 and i != unk_id}
    for docs, all_ids in ((c["docs"], c["ids"]), (c["tie_docs"], c["tie_ids"])):
        assert len(docs) == len(all_ids)
        for d, ids in zip(docs, all_ids):
            assert "▁" not in d and all(0 <= i < len(pieces) for i in ids)
            assert all(a != unk_id or b != unk_id for a, b in zip(ids, ids[1:]))   # runs of unknowns come collapsed
            assert _follows(d.replace(" ", "▁"), ids, pieces, unk_id, known), d
    assert c["docs"].count("") >= 2 and c["docs"][-1] == "" and "" in c["docs"][1:-1]


def test_generator_writes_the_committed_fixtures_again():
    """make_tokenizer_golden.py trains both models again, passes all its own assertions (its docstring lists them) and produces the
    committed bytes; with other versions of the libraries than the recorded ones the trained models may differ, and the test is skipped"""
    versions = tg.load("bpe_vocab")["versions"]
    for name in ("sentencepiece", "tokenizers", "regex"):
        if pytest.importorskip(name).__version__ != versions[name]:
            pytest.skip(f"the fixtures were written with {name} {versions[name]}")
    if unicodedata.unidata_version != versions["unidata_version"]:
        pytest.skip(f"the fixtures were written with Unicode {versions['unidata_version']}")
    spec = importlib.util.spec_from_file_location("make_tokenizer_golden", os.path.join(tg.GOLDEN, "make_tokenizer_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    files, stats = gen.generate()
    assert sorted(files) == sorted(f"tokenizer_{n}.json" for n in ("bpe_vocab", "bpe_cases", "unigram_vocab", "unigram_cases"))
    for name, blob in files.items():
        with open(os.path.join(tg.GOLDEN, name), "rb") as f:
            assert f.read() == blob, name
        assert len(blob) < 64 * 1024
    print("sensitivity:", {k: v for k, v in stats.items() if "changed" in k or "unknown" in k})


# ------------------------------------------------------------------------- 2. a second implementation, rebuilt from the committed lists
def test_rebuilt_tokenizers_bpe_gives_the_committed_ids_and_words():
    tokenizers = pytest.importorskip("tokenizers")
    pieces, c = tg.bpe_pieces(), tg.load("bpe_cases")
    b2u = tg.byte_alphabet()
    name = [("".join(b2u[b] for b in p)) for p in pieces]
    merges = [(name[a], name[b]) for a, b in tg.load("bpe_vocab")["merges"]]
    tok = tokenizers.Tokenizer(tokenizers.models.BPE({s: i for i, s in enumerate(name)}, merges))
    tok.pre_tokenizer = tokenizers.pre_tokenizers.ByteLevel(add_prefix_space=False, use_regex=True)
    for d, ids, bounds in zip(c["docs"], c["ids"], c["word_bounds"]):
        assert tok.encode(d, add_special_tokens=False).ids == ids, d
        got = [0]
        for w, _ in tok.pre_tokenizer.pre_tokenize_str(d):
            got.append(got[-1] + len(w))   # one stand-in character per byte
        assert got == bounds, d
    words, word_ids = tg.bpe_words()
    for w, ids in zip(words, word_ids):
        assert tok.encode(w.decode(), add_special_tokens=False).ids == ids, w


def test_rebuilt_tokenizers_unigram_gives_sentencepieces_ids():
    tokenizers = pytest.importorskip("tokenizers")
    v, c = tg.load("unigram_vocab"), tg.load("unigram_cases")
    tok = tokenizers.Tokenizer(tokenizers.models.Unigram(vocab=list(zip(v["pieces"], v["scores"])), unk_id=v["unk_id"]))
    for d, ids in zip(c["docs"] + c["tie_docs"], c["ids"] + c["tie_ids"]):
        assert tok.encode(d.replace(" ", "▁"), add_special_tokens=False).ids == ids, d


def test_regex_module_gives_the_committed_words():
    regex = pytest.importorskip("regex")
    c = tg.load("bpe_cases")
    pat = regex.compile(GPT2_PATTERN)
    for d, bounds in zip(c["docs"], c["word_bounds"]):
        raw = d.encode()
        assert [w.encode() for w in pat.findall(d)] == [raw[s:e] for s, e in zip(bounds, bounds[1:])], d


# ----------------------------------------------------------------------------- 3. the GPU suites' references against the libraries
@pytest.fixture(scope="module")
def bpe_oracle():
    pieces = tg.bpe_pieces()
    return orc.OraclePma.build(pieces, values=np.arange(len(pieces), dtype=np.uint32))


def test_bpe_reference_gives_tokenizers_ids(bpe_oracle):
    words, word_ids = tg.bpe_words()
    pi, ranks = tg.permutation(len(tg.bpe_pieces()))
    po = orc.OraclePma.build(tg.bpe_pieces(), values=pi)
    inv = np.argsort(pi)
    for w, ids in zip(words, word_ids):
        toks = _bpe(w, bpe_oracle.find_overlapping_iter(w), None, Gap.Bytes, GID)
        assert [t[0] for t in toks] == ids, w
        assert [w[s:e] for _, s, e in toks] == [tg.bpe_pieces()[i] for i in ids]
        toks = _bpe(w, po.find_overlapping_iter(w), ranks, Gap.Bytes, GID)   # value = pi(id), ranks[pi(id)] = id
        assert [int(inv[t[0]]) for t in toks] == ids, w


def test_bpe_reference_behind_the_split_gives_tokenizers_document_ids(bpe_oracle):
    c = tg.load("bpe_cases")
    cc = da.char_classes()
    for d, ids, bounds in zip(c["docs"], c["ids"], c["word_bounds"]):
        raw = d.encode()
        wo, dw = scan_batch([raw], Split.Gpt2, cc)
        assert wo.tolist() == (bounds if raw else [0]) and dw.tolist() == [0, len(bounds) - 1], d
        got = []
        for s, e in zip(bounds, bounds[1:]):
            got += [t[0] for t in _bpe(raw[s:e], bpe_oracle.find_overlapping_iter(raw[s:e]), None, Gap.Bytes, GID)]
        assert got == ids, d
    # the batch form, as daac_split_batch defines it
    raws = [d.encode() for d in c["docs"]]
    wo, dw = scan_batch(raws, Split.Gpt2, cc, 7)
    want, at = [], 7
    for raw, bounds in zip(raws, c["word_bounds"]):
        want += [at + b for b in bounds[:-1]]
        at += len(raw)
    assert wo.tolist() == want + [at] and dw.tolist() == np.cumsum([0] + [len(b) - 1 for b in c["word_bounds"]]).tolist()


def test_unigram_reference_gives_sentencepieces_ids():
    pats, values, scores, unk_id, unk_score = tg.unigram_model()
    o = orc.OraclePma.build(pats, values=values)
    c = tg.load("unigram_cases")
    pieces = tg.load("unigram_vocab")["pieces"]
    for d, ids in zip(c["docs"] + c["tie_docs"], c["ids"] + c["tie_ids"]):
        raw = tg.sp_text(d)
        toks, score = _viterbi(raw, o.find_overlapping_iter(raw), scores, unk_score, Gap.Chars, unk_id)
        assert tg.collapse([t[0] for t in toks], unk_id) == ids, d
        assert all(raw[s:e] == pieces[i].encode() for i, s, e in toks if i != unk_id)
        assert type(score) is np.float32 and (score < 0 or not raw)
