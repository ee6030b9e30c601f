#!/usr/bin/env python3
"""Writes tests/golden/normalize_cases.json (data only): a few hundred multi-script documents and what `tokenizers` makes of them — the
bytes of normalizers.BertNormalizer.normalize_str under three sets of options and, for the default options, the ids and byte offsets of
the full Tokenizer (BertNormalizer + BertPreTokenizer + models.WordPiece over the committed tokenizer_wordpiece_vocab.json, no special
tokens).

    python tests/golden/make_normalize_golden.py            # writes the file
    python tests/golden/make_normalize_golden.py --check    # regenerates in memory and compares with the committed bytes

Needs `tokenizers`, no GPU, and nothing of the library's kernels: from this repository it takes bert_char_classes() (pure Python;
importing it needs the package built), the pure-Python definitions of tests/normalize_golden.py and tests/wordpiece_golden.py and the word
lists of make_tokenizer_golden.py.  All text is synthetic and every seed is fixed.

The text holds mixed-case Latin with precomposed and combining accents, Greek and Cyrillic capitals, İ, ẞ and ǅ, Hangul, CJK with
compatibility ideographs, tabs, newlines, NBSP and U+3000, NUL, U+FFFD, U+200D and a private-use character.

Before anything is written the generator asserts:
  a. what the issue behind this fixture states about BertNormalizer, on every scalar value: the substitution per code point
     (normalize_golden.bert_image) equals normalize_str("a" + c + "b")[1:-1] but for code points assigned after the older of the two
     libraries' Unicode tables — 379 under the default options, 11 with strip_accents and lowercase off — and its longest image has 12
     bytes;
  b. every character of the documents is one on which the two agree under all three option sets, and none of the 23 that canonical
     reordering could move;
  c. on every document (none is excluded) and under every option set, the sequential scanner over that substitution gives
     normalize_str's bytes;
  d. on every document, the scanner, then the Split.Bert and WordPiece definitions over its output, then spans_to_source give the full
     Tokenizer's ids and offsets;
  e. the cases discriminate: the documents that change under each of the four steps alone, and those whose ids differ with and without
     the normalizer, are counted, and no count is zero.
"""
import json
import os
import random
import sys
import unicodedata

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)                                     # make_tokenizer_golden: the word lists
sys.path.insert(0, os.path.dirname(HERE))                    # tests/: normalize_golden, wordpiece_golden
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))   # the repository: daachorse_amd

import make_tokenizer_golden as base  # noqa: E402
import normalize_golden as ng  # noqa: E402
import wordpiece_golden as wg  # noqa: E402

SEED = 20261020
N_DOCS = 300
MAX_FILE = 160 * 1024
COMBINING = ["é", "à", "ö", "ñ", "û", "ç", "Å", "Ẹ́", "ό", "й"]
SPECIAL = ["İ", "ẞ", "ǅ", "İstanbul", "STRAẞE", "ǅungla", "Σ", "ΟΔΟΣ", "ſ", "Å", "Ǆ"]
CAPITALS = ["ΛΟΓΟΣ", "Ελλάδα", "ΆΝΘΡΩΠΟΣ", "Москва", "ПРИВЕТ", "Человек", "ЁЛКА", "Йод", "ÉLÈVE", "Zürich", "ÜBER", "SMÖRGÅSBORD", "Ångström", "ŒUVRE"]
COMPAT = ["豈", "欄", "﨎", "\U0002f800", "\U0002f9d4"]   # compatibility ideographs: two decompose, one does not, two beyond the BMP
WIDE_CJK = ["㐀", "\U00020000", "\U0002a700", "\U0002b820"]       # extensions A, B and C; U+2B820 lies in none of BERT's blocks
SPACES = ["\t", "\n", "\r\n", " ", "　", " ", " ", " \t ", "  "]
REMOVED = ["\0", "�", "‍", "", "\x07", "\x7f", "­", "\U000f0000", "\x0b", "\u0085"]


def documents(seed):
    rng = random.Random(seed)
    pools = ([base.ENGLISH] * 4 + [base.ACCENTED] * 2 + [base.GREEK, base.CYRILLIC, base.CJK, base.KANA, base.HANGUL, base.ARABIC, base.NUMBERS, base.PUNCT,
                                                          COMBINING, SPECIAL, CAPITALS, COMPAT, WIDE_CJK, base.CONTRACTIONS])
    docs = []
    for k in range(N_DOCS):
        if k in (5, 151, N_DOCS - 1):
            docs.append("")
            continue
        if k in (9, 152):
            docs.append(rng.choice(REMOVED) * 3)   # normalizes to nothing
            continue
        if k == 10:
            docs.append(" \t ")
            continue
        parts = []
        for _ in range(rng.randrange(1, 8)):
            w = rng.choice(rng.choice(pools))
            r = rng.random()
            if r < 0.25:
                w = w.upper()
            elif r < 0.45:
                w = w[:1].upper() + w[1:]
            elif r < 0.55:
                w = "".join(ch.upper() if rng.random() < 0.5 else ch for ch in w)
            if rng.random() < 0.15:   # a removed character inside, in front of or behind the word
                i = rng.choice((0, len(w) // 2, len(w)))
                w = w[:i] + rng.choice(REMOVED) + w[i:]
            if rng.random() < 0.1:    # an ideograph glued to the word
                w = w + rng.choice(base.CJK + COMPAT + WIDE_CJK)[:1]
            if rng.random() < 0.08:
                w = w + rng.choice(["́", "̈", "̧́"])
            r = rng.random()
            sep = "" if r < 0.06 else rng.choice(SPACES) if r < 0.3 else rng.choice(base.PUNCT) if r < 0.36 else " "
            parts += [w, sep]
        if rng.random() < 0.1:
            parts.insert(0, rng.choice(SPACES + REMOVED))
        if rng.random() < 0.6:
            parts.pop()
        docs.append("".join(parts))
    return docs


def byte_spans(text, spans):
    """character spans of a str -> byte spans of its UTF-8"""
    at = [0]
    for ch in text:
        at.append(at[-1] + len(ch.encode()))
    return [(at[s], at[e]) for s, e in spans]


def check_every_scalar(normalizers):
    """a. -> the code points on which the substitution and `tokenizers` differ, per option set"""
    differ, longest = {}, 0
    for name, opts in ng.OPTIONS.items():
        cps = [cp for cp in range(0x110000) if not 0xD800 <= cp <= 0xDFFF]
        want = [ng.bert_image(cp, *opts) for cp in cps]
        f = normalizers[name].normalize_str
        got = [f("a" + chr(cp) + "b")[1:-1] for cp in cps]
        differ[name] = {cp for cp, w, g in zip(cps, want, got) if w != g}
        if name == "default":
            longest = max(len(w.encode()) for w in want)
    return differ, longest


def generate():
    os.environ["TOKENIZERS_PARALLELISM"] = "false"
    import tokenizers
    from tokenizers import Tokenizer, models, normalizers, pre_tokenizers

    from daachorse_amd import bert_char_classes

    versions = {"tokenizers": tokenizers.__version__, "unidata_version": unicodedata.unidata_version}
    norm = {name: normalizers.BertNormalizer(clean_text=o[0], handle_chinese_chars=o[1], strip_accents=o[2], lowercase=o[3]) for name, o in ng.OPTIONS.items()}
    differ, longest = check_every_scalar(norm)
    assert longest == 12, longest
    assert len(differ["default"]) == 379 and len(differ["clean_only"]) == 11, {k: len(v) for k, v in differ.items()}
    # every one of them was assigned after the older table: the running Python's table is the older or does not know it differently
    off_limits = set().union(*differ.values()) | ng.REORDERED

    vocab_file = wg.load("vocab")
    vocab_str, unk_id, max_chars, prefix = vocab_file["vocab"], vocab_file["unk_id"], vocab_file["max_input_chars_per_word"], vocab_file["prefix"]
    assert vocab_file["versions"]["tokenizers"] == tokenizers.__version__, "the committed vocabulary was trained by another version"
    model = models.WordPiece(vocab=vocab_str, unk_token="[UNK]", max_input_chars_per_word=max_chars, continuing_subword_prefix=prefix)
    tok = Tokenizer(model)
    tok.normalizer = norm["default"]
    tok.pre_tokenizer = pre_tokenizers.BertPreTokenizer()
    plain = Tokenizer(models.WordPiece(vocab=vocab_str, unk_token="[UNK]", max_input_chars_per_word=max_chars, continuing_subword_prefix=prefix))
    plain.pre_tokenizer = pre_tokenizers.BertPreTokenizer()
    vocab = {k.encode(): i for k, i in vocab_str.items()}
    table = wg.class_table(bert_char_classes())

    docs = documents(SEED)
    for d in docs:
        for ch in d:
            assert ord(ch) not in off_limits, ("b", d, hex(ord(ch)))
    have = set("".join(docs))
    for need in "İẞǅ\t\n 　\0�‍豈":
        assert need in have, hex(ord(need))
    normalized = {name: [] for name in ng.OPTIONS}
    doc_ids, doc_spans = [], []
    steps = {"clean_text": (True, False, False, False), "handle_chinese_chars": (False, True, False, False), "strip_accents": (False, False, True, False),
             "lowercase": (False, False, False, True)}
    changed = {k: 0 for k in steps}
    ids_differ = n_unk = n_tok = 0
    for d in docs:
        raw = d.encode()
        for name, opts in ng.OPTIONS.items():
            want = norm[name].normalize_str(d).encode()
            got, _ = ng.bert_scan(raw, opts)
            assert got == want, ("c", name, d)
            normalized[name].append(want.decode())
        for k, opts in steps.items():
            changed[k] += ng.bert_scan(raw, opts)[0] != raw
        enc = tok.encode(d, add_special_tokens=False)
        ids, spans = enc.ids, byte_spans(d, enc.offsets)
        out, src = ng.bert_scan(raw, ng.OPTIONS["default"])
        my_ids, my_spans = wg.wordpiece_doc(out, table, vocab, unk_id, max_chars, prefix.encode())
        assert (my_ids, ng.spans_to_source(my_spans, src, raw)) == (ids, spans), ("d", d, my_ids, ids, ng.spans_to_source(my_spans, src, raw), spans)
        ids_differ += plain.encode(d, add_special_tokens=False).ids != ids
        n_unk += ids.count(unk_id)
        n_tok += len(ids)
        doc_ids.append(ids)
        doc_spans.append(wg.pack_spans(spans) if all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) else None)
    # offsets of tokens that share a source character (a Hangul syllable's jamo) overlap: such a document keeps its spans unpacked
    flat_spans = [p if p is not None else {"raw": byte_spans(d, tok.encode(d, add_special_tokens=False).offsets)} for p, d in zip(doc_spans, docs)]
    sens = {"docs_changed_by_" + k: v for k, v in changed.items()}
    sens.update({"docs_whose_ids_differ_without_the_normalizer": ids_differ, "tokens": n_tok, "tokens_unk": n_unk})
    assert all(v > 0 for v in changed.values()) and ids_differ > 0, ("e", sens)
    assert n_unk * 4 <= n_tok, ("at most a quarter [UNK]", sens)
    cases = {"about": "tokenizers' BertNormalizer.normalize_str per option set (clean_text, handle_chinese_chars, strip_accents, lowercase) and, for the "
                      "default options, the ids and byte offsets of BertNormalizer + BertPreTokenizer + WordPiece over tokenizer_wordpiece_vocab.json; "
                      "spans packed as [gap, length, ..] or, where tokens share a source character, {raw: [[start, end], ..]}",
             "versions": versions, "options": {k: list(v) for k, v in ng.OPTIONS.items()}, "sensitivity": sens,
             "code_points_that_differ_from_tokenizers": {k: len(v) for k, v in differ.items()}, "docs": docs, "normalized": normalized, "ids": doc_ids,
             "tok_spans": flat_spans}
    blob = (json.dumps(cases, ensure_ascii=False, separators=(",", ":")) + "\n").encode()
    assert len(blob) <= MAX_FILE, len(blob)
    assert json.loads(blob) == json.loads(json.dumps(cases))
    stats = {"docs": len(docs), "bytes": sum(len(d.encode()) for d in docs), **sens, "file_bytes": len(blob)}
    return {"normalize_cases.json": blob}, stats


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
