#!/usr/bin/env python3
"""Writes tests/golden/special_tokens_cases.json (data only): a few hundred noisy documents with special tokens written into them and
what `tokenizers` makes of them with those tokens added as AddedToken(.., special=True) — the ids of the byte-level BPE tokenizer
(ByteLevel, add_prefix_space=False, over the committed tokenizer_bpe_vocab.json) and the ids and byte spans of the BERT tokenizer
(BertNormalizer + BertPreTokenizer + WordPiece over the committed tokenizer_wordpiece_vocab.json).

    python tests/golden/make_special_golden.py            # writes the file
    python tests/golden/make_special_golden.py --check    # regenerates in memory and compares with the committed bytes

Needs `tokenizers` and `regex`, no GPU, and nothing of the library's kernels: from this repository it takes bert_char_classes() (pure
Python; importing it needs the package built), the pure-Python definitions of tests/special_golden.py, tests/normalize_golden.py and
tests/wordpiece_golden.py and the documents of make_tokenizer_golden.py.  All text is synthetic and every seed is fixed.

Each list of specials holds one that is a prefix of another (<|a|> and <|a|><|b|>, [MASK] and [MASK][SEP]), one that overlaps another's
tail (|><|, K][) and an ordinary word (the).  An added token that the vocabulary already holds keeps the vocabulary's id (the); the
others get the ids above the vocabulary.  The hand-written documents have a special at the start, at the end and alone, two and three
adjacent, inside a word, cut short, wrongly cased, with whitespace runs around it, next to multi-byte text, and empty documents.

Before anything is written the generator asserts, on every document (none is excluded):
  a. the definition — cut at the matches of a leftmost-longest scan over the raw text (special_golden.cut), every text segment
     tokenized as a string of its own by the definitions the other fixtures were checked with (the GPT-2 pattern and a rank merge; the
     BERT normalizer, Split.Bert and WordPiece, spans_to_source), splice (special_golden.splice) — gives `tokenizers`' ids, and for the
     BERT tokenizer its byte spans;
  b. the BPE tokens tile the document: a piece's length is its bytes and a special's is its text;
  c. the BERT tokenizer without its normalizer, on the document whose text segments were normalized beforehand, gives the same ids;
  d. the cases discriminate.  For each tokenizer at least 100 documents hold a special, and at least 30 of those change their ids when
     the specials are ignored; at least 10 documents change when the stretches between specials are not split independently but the
     text is split whole, with the specials masked out; at least 5 change under leftmost-first in list order instead of
     leftmost-longest.
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)                                     # make_tokenizer_golden: the documents
sys.path.insert(0, os.path.dirname(HERE))                    # tests/: special_golden, normalize_golden, wordpiece_golden
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))   # the repository: daachorse_amd

import make_tokenizer_golden as base  # noqa: E402
import normalize_golden as ng  # noqa: E402
import special_golden as sg  # noqa: E402
import wordpiece_golden as wg  # noqa: E402

SEED = 20261021
N_SEEDED = 250
MAX_FILE = 64 * 1024
# list order is what leftmost-first would go by: the shorter of two that share a start comes first
BPE_SPECIALS = ["<|endoftext|>", "<|a|>", "<|a|><|b|>", "|><|", "the", "<|im_start|>", "<|eot_id|>"]
WP_SPECIALS = ["[CLS]", "[SEP]", "[MASK]", "[MASK][SEP]", "K][", "the", "[PAD]"]
HAND = ["<|endoftext|>hello", "hello<|endoftext|>", "<|endoftext|>", "[CLS]hello world[SEP]", "[MASK]", "[CLS]",
        "<|endoftext|><|endoftext|>", "<|im_start|><|eot_id|><|endoftext|>x", "[CLS][MASK][SEP]", "[SEP][SEP]", "a[PAD][PAD][PAD]",
        "other", "bro<|a|>ther", "un[MASK]ed", "mother then", "x<|a|><|c|>",
        "<|endoftext", "<|endoftext|", "|endoftext|>", "[MASK", "MASK]", "<|a|", "<|a|><|b|",
        "[cls] [Mask]", "[CLS] [mask] [MASK]", "<|EndOfText|>", "The THE the", "[Sep]x[SEP]",
        "hello  <|endoftext|>world", "hello  world", "hello   [SEP]   world", "<|a|>  \n x", "a \n\n<|eot_id|>\n b", "  [MASK]  ", "\t<|endoftext|>\t",
        "a  <|a|>  b  <|a|>", "we'll <|a|>'ll", "it<|a|>'s", "12<|a|>34 5  [CLS]  6",
        "世界<|endoftext|>日本語", "café[MASK]naïve", "привет[SEP]мир", "<|a|>é", "é<|a|>", "ありがとう[CLS]こんにちは", "한국어<|eot_id|>사람", base.EMOJI + "<|a|>" + base.EMOJI,
        "", "",
        "x|><|y", "<|a|><|b|>", "<|a|><|b|><|a|>", "<|a|>|><|b|>", "[MASK][SEP]", "[MASK][SEP][MASK]", "[MAS K][ x", "K][", "[MASK][CLS]", "[MASK][SEPx",
        "[MASK]the[SEP]", "<|a|><|b|>the<|a|>", "bathe[MASK][SEP]K]["]


def documents():
    """the hand-written documents and N_SEEDED of make_tokenizer_golden's with specials of either list written in at seeded positions, some
    behind a whitespace run and some in front of a contraction (<|a|>'s: split whole, the apostrophe belongs to the punctuation in front of it)"""
    rng = random.Random(SEED)
    pool = BPE_SPECIALS + WP_SPECIALS + ["<|a|><|b|>", "[MASK][SEP]"]
    docs = []
    for d in base.documents(SEED)[:N_SEEDED]:
        if d and rng.random() < 0.75:
            for _ in range(rng.randrange(1, 4)):
                at = rng.randrange(len(d) + 1)
                pad = rng.choice(["  ", " \n", "   "]) if rng.random() < 0.15 else ""   # a whitespace run that ends at the special
                tail = rng.choice(["'s", "'ll", "'re", "'t"]) if rng.random() < 0.2 else ""   # a contraction that begins behind the special
                d = d[:at] + pad + rng.choice(pool) + tail + d[at:]
        docs.append(d)
    return HAND + docs


def bpe_tokenizer():
    from tokenizers import Tokenizer, models, pre_tokenizers

    with open(os.path.join(HERE, "tokenizer_bpe_vocab.json"), encoding="utf-8") as f:
        v = json.load(f)
    pieces = [bytes.fromhex(h) for h in v["pieces_hex"]]
    mapped = ["".join(base.B2U[b] for b in p) for p in pieces]
    tok = Tokenizer(models.BPE(vocab={m: i for i, m in enumerate(mapped)}, merges=[(mapped[a], mapped[b]) for a, b in v["merges"]]))
    tok.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False, use_regex=True)
    return tok, pieces


def wordpiece_tokenizer(normalizer):
    from tokenizers import Tokenizer, models, normalizers, pre_tokenizers

    v = wg.load("vocab")
    tok = Tokenizer(models.WordPiece(vocab=v["vocab"], unk_token="[UNK]", max_input_chars_per_word=v["max_input_chars_per_word"],
                                     continuing_subword_prefix=v["prefix"]))
    if normalizer:
        tok.normalizer = normalizers.BertNormalizer()
    tok.pre_tokenizer = pre_tokenizers.BertPreTokenizer()
    return tok


def add_specials(tok, texts, vocab_size):
    """-> [[text, id]] in list order; a text the vocabulary holds keeps its id, the others follow the vocabulary"""
    from tokenizers import AddedToken

    tok.add_special_tokens([AddedToken(t, special=True) for t in texts])
    out = [[t, tok.token_to_id(t)] for t in texts]
    new = [i for _, i in out if i >= vocab_size]
    assert new == list(range(vocab_size, vocab_size + len(new))) and len(new) >= len(texts) - 1, out
    return out


def generate():
    os.environ["TOKENIZERS_PARALLELISM"] = "false"
    import regex
    import tokenizers

    from daachorse_amd import bert_char_classes

    versions = {"tokenizers": tokenizers.__version__, "regex": regex.__version__}
    docs = documents()
    raws = [d.encode() for d in docs]

    # ---- byte-level BPE
    bpe, pieces = bpe_tokenizer()
    bpe_plain, _ = bpe_tokenizer()
    bpe_spec = add_specials(bpe, BPE_SPECIALS, len(pieces))
    spec_b = [(t.encode(), i) for t, i in bpe_spec]
    rank_of = {p: i for i, p in enumerate(pieces)}
    gpt2 = regex.compile(base.GPT2_PATTERN)

    def bpe_words(words):
        ids, spans, pos = [], [], 0
        for w in words:
            for i in base.rank_merge(w, rank_of):
                ids.append(i)
                spans.append((pos, pos + len(pieces[i])))
                pos += len(pieces[i])
        return ids, spans

    def bpe_text(seg):
        return bpe_words([w.encode() for w in gpt2.findall(seg.decode())])

    bpe_ids = [bpe.encode(d, add_special_tokens=False).ids for d in docs]
    special_len = {i: len(t) for t, i in spec_b}
    mine = sg.tokenize_docs(raws, lambda d: sg.leftmost(d, spec_b), bpe_text)
    first = sg.tokenize_docs(raws, lambda d: sg.leftmost(d, spec_b, longest=False), bpe_text)
    n_hold_b = n_ignored_b = n_whole = 0
    by_first = set()
    for k, (d, raw) in enumerate(zip(docs, raws)):
        assert mine[k][0] == bpe_ids[k], ("a: bpe", d, mine[k][0], bpe_ids[k])
        pos = 0
        for i, (s, e) in zip(*mine[k]):   # b. the tiling
            assert s == pos and e - s == (special_len[i] if i in special_len else len(pieces[i])), ("b", d)
            pos = e
        assert pos == len(raw), ("b", d)
        matches = sg.leftmost(raw, spec_b)
        n_hold_b += bool(matches)
        n_ignored_b += bool(matches) and bpe_plain.encode(d, add_special_tokens=False).ids != bpe_ids[k]
        # the wrong way: the whole text split once, the words then cut at the specials' ends
        cuts = {0, len(raw)} | {x for s, e, _ in matches for x in (s, e)}
        at = 0
        for w in gpt2.findall(d):
            cuts.add(at)
            at += len(w.encode())
        cuts = sorted(c for c in cuts if not any(s < c < e for s, e, _ in matches))
        whole, inside = [], {s: (e, v) for s, e, v in matches}
        for s, e in zip(cuts, cuts[1:]):
            whole += [inside[s][1]] if s in inside and inside[s][0] == e else bpe_words([raw[s:e]])[0]
        n_whole += whole != bpe_ids[k]
        if first[k][0] != bpe_ids[k]:
            by_first.add(k)

    # ---- BERT: normalizer, pre-tokenizer, WordPiece
    wp, wp_plain, wp_bare = wordpiece_tokenizer(True), wordpiece_tokenizer(True), wordpiece_tokenizer(False)
    vocab_file = wg.load("vocab")
    assert vocab_file["versions"]["tokenizers"] == tokenizers.__version__, "the committed vocabulary was trained by another version"
    wp_spec = add_specials(wp, WP_SPECIALS, len(vocab_file["vocab"]))
    assert add_specials(wp_bare, WP_SPECIALS, len(vocab_file["vocab"])) == wp_spec
    spec_w = [(t.encode(), i) for t, i in wp_spec]
    vocab, unk_id, max_chars, prefix = wg.model()
    table = wg.class_table(bert_char_classes())

    def wp_text(seg):
        out, src = ng.bert_scan(seg, ng.OPTIONS["default"])
        ids, spans = wg.wordpiece_doc(out, table, vocab, unk_id, max_chars, prefix.encode())
        return ids, ng.spans_to_source(spans, src, seg)

    mine = sg.tokenize_docs(raws, lambda d: sg.leftmost(d, spec_w), wp_text)
    first = sg.tokenize_docs(raws, lambda d: sg.leftmost(d, spec_w, longest=False), wp_text)
    wp_ids, wp_spans = [], []
    n_hold_w = n_ignored_w = 0
    for k, (d, raw) in enumerate(zip(docs, raws)):
        enc = wp.encode(d, add_special_tokens=False)
        ids, spans = enc.ids, base_byte_spans(d, enc.offsets)
        assert (mine[k][0], [tuple(x) for x in mine[k][1]]) == (ids, spans), ("a: wordpiece", d, mine[k], ids, spans)
        matches = sg.leftmost(raw, spec_w)
        normalized = "".join(raw[s:e].decode() if v != sg.TEXT else ng.bert_scan(raw[s:e], ng.OPTIONS["default"])[0].decode()
                             for s, e, v in segments(raw, matches))
        assert wp_bare.encode(normalized, add_special_tokens=False).ids == ids, ("c", d)
        n_hold_w += bool(matches)
        n_ignored_w += bool(matches) and wp_plain.encode(d, add_special_tokens=False).ids != ids
        if first[k][0] != ids:
            by_first.add(k)
        wp_ids.append(ids)
        wp_spans.append(wg.pack_spans(spans) if all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) else {"raw": spans})

    n_first = len(by_first)
    sens = {"docs_with_a_bpe_special": n_hold_b, "bpe_docs_changed_when_ignored": n_ignored_b, "docs_with_a_wordpiece_special": n_hold_w,
            "wordpiece_docs_changed_when_ignored": n_ignored_w, "docs_changed_by_splitting_the_text_whole": n_whole, "docs_changed_by_leftmost_first": n_first}
    assert n_hold_b >= 100 and n_hold_w >= 100 and n_ignored_b >= 30 and n_ignored_w >= 30 and n_whole >= 10 and n_first >= 5, ("d", sens)
    cases = {"about": "tokenizers' ids per document with the specials added as AddedToken(special=True): byte-level BPE over tokenizer_bpe_vocab.json "
                      "(ByteLevel, add_prefix_space=False) and BertNormalizer + BertPreTokenizer + WordPiece over tokenizer_wordpiece_vocab.json, the "
                      "latter with byte spans packed as [gap, length, ..] or, where tokens share a source character, {raw: [[start, end], ..]}; "
                      "specials as [text, id] in the order they were added",
             "versions": versions, "sensitivity": sens, "bpe_specials": bpe_spec, "wordpiece_specials": wp_spec, "docs": docs, "bpe_ids": bpe_ids,
             "wordpiece_ids": wp_ids, "wordpiece_spans": wp_spans}
    blob = (json.dumps(cases, ensure_ascii=False, separators=(",", ":")) + "\n").encode()
    assert len(blob) < MAX_FILE, len(blob)
    assert json.loads(blob) == json.loads(json.dumps(cases))
    stats = {"docs": len(docs), "bytes": sum(map(len, raws)), **sens, "file_bytes": len(blob)}
    return {"special_tokens_cases.json": blob}, stats


def base_byte_spans(text, spans):
    """character spans of a str -> byte spans of its UTF-8"""
    at = [0]
    for ch in text:
        at.append(at[-1] + len(ch.encode()))
    return [(at[s], at[e]) for s, e in spans]


def segments(raw, matches):
    """-> [(start, end, value or TEXT)] of one document: special_golden.cut on it"""
    so, _, sv = sg.cut([raw], lambda d: matches)
    return [(int(s), int(e), int(v)) for s, e, v in zip(so, so[1:], sv)]


def main():
    check = "--check" in sys.argv[1:]
    files, stats = generate()
    for name, blob in files.items():
        path = os.path.join(HERE, name)
        if check:
            with open(path, "rb") as f:
                assert f.read() == blob, f"{name} differs from what this run generates"
        else:
            with open(path, "wb") as f:
                f.write(blob)
    print(("checked " if check else "wrote ") + json.dumps(stats))


if __name__ == "__main__":
    main()
