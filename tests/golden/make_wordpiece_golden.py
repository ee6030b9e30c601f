#!/usr/bin/env python3
"""Writes the WordPiece fixtures under tests/golden/ (data only): a WordPiece vocabulary trained by `tokenizers` on synthetic multi-script
text, and what `tokenizers` (models.WordPiece behind pre_tokenizers.BertPreTokenizer, no normalizer, no special tokens) makes of a few
hundred noisy documents.

    python tests/golden/make_wordpiece_golden.py            # writes the cases from the committed vocabulary (trains one if there is none)
    python tests/golden/make_wordpiece_golden.py --train    # trains a new vocabulary and writes both files
    python tests/golden/make_wordpiece_golden.py --check    # regenerates in memory and compares with the committed bytes

Needs `tokenizers`, no GPU, and nothing of the library's kernels: from this repository it takes bert_char_classes() (pure Python;
importing it needs the package built), the two pure-Python definitions of tests/wordpiece_golden.py and the word lists of
make_tokenizer_golden.py.  All text is synthetic and every seed is fixed.  The trainer breaks ties between equally frequent pairs in the
order of a hash table that is seeded per process, so two trainings give two vocabularies: the committed vocabulary file is the record,
a run without --train reads it back, and from it a second run writes the same bytes.

    tokenizer_wordpiece_vocab.json   the vocabulary {piece: id}, the "##" prefix, unk_id, max_input_chars_per_word
    tokenizer_wordpiece_cases.json   documents; per document `tokenizers`' ids, its token spans and BertPreTokenizer's word spans, both in
                                     bytes (converted from character offsets) and packed as [gap, length, ..] (wordpiece_golden.unpack_spans)

The documents hold no ASCII control characters besides whitespace.  Before anything is written the generator asserts, on every document
(none is excluded):
  a. the sequential Split.Bert scanner with bert_char_classes() gives BertPreTokenizer's words once the whitespace words are dropped;
  b. the definition of daac_tokenize_wordpiece in pure Python (greedy longest-match-first with an initial and a continuation piece set,
     whole-word [UNK], the character cap) gives `tokenizers`' ids and spans;
  c. the cases can tell a wrong tokenizer from a right one: >= 200 words have two or more pieces; >= 10 distinct words change when the
     roles are ignored (initial and continuation pieces merged); >= 10 distinct words have a piece at 0 but fail later, so whole-word
     [UNK] differs from a partial output; >= 5 words are above 16 characters; >= 5 words have at most 16 characters but more than 16
     bytes; >= 10 words differ under shortest-match-first;
  and at most 10 % of all words are [UNK], so parity is not carried by [UNK].
"""
import json
import os
import random
import sys
import unicodedata

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)                                     # make_tokenizer_golden: the word lists
sys.path.insert(0, os.path.dirname(HERE))                    # tests/: wordpiece_golden
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))   # the repository: daachorse_amd

import make_tokenizer_golden as base  # noqa: E402
import wordpiece_golden as wg  # noqa: E402

SEED = 20261019
N_DOCS = 300
VOCAB_SIZE = 1200
MAX_CHARS = 16
PREFIX = "##"
MAX_FILE = 64 * 1024
# non-ASCII punctuation (P*: words of their own) and symbols (S*: BERT leaves them inside words)
WIDE_PUNCT = ["。", "、", "¿", "«", "»", "—", "…", "「", "」", "·", "！"]
SYMBOLS = ["€", "°", "±", "→", "©"]
SPACES = base.SPACES + [" ", " ", "　 "]
# never seen by the trainer: a word that holds one of them has no segmentation
UNSEEN = base.HANGUL + base.HEBREW + [base.EMOJI, "ξ", "ӂ", "ў"]
KNOWN = [w for w in base.KNOWN_WORDS if w not in base.UNSEEN_BY_UNIGRAM]
LONG = ["internationalization", "counterrevolutionaries", "thethethethethethe", "importantimportant", "somethingsomethingsomething",
        "человекчеловекработа", "こんにちはありがとうカタカナひらがな", "mississippimississippi"]
WIDE = ["человекработа", "спасибохорошо", "φιλοσοφίαΕλλάδα", "ありがとうこんにちは", "привет" + "мир" * 3, "時間大学中国今日世界日本語", "άνθρωποςκόσμος", "مدينةكتابسلام"]


def documents(seed):
    rng = random.Random(seed)
    pools = ([base.ENGLISH] * 6 + [base.REPEATED] * 2 + [base.ACCENTED, base.GREEK, base.CYRILLIC, base.CJK, base.KANA, base.ARABIC, base.CONTRACTIONS,
                                                          base.NUMBERS, base.PUNCT, WIDE_PUNCT, SYMBOLS, LONG + WIDE])
    docs = []
    for k in range(N_DOCS):
        if k in (3, 150, N_DOCS - 1):
            docs.append("")
            continue
        if k in (7, 151):
            docs.append(rng.choice(SPACES) * 2)   # whitespace only
            continue
        parts = []
        for _ in range(rng.randrange(1, 8)):
            w = rng.choice(rng.choice(pools))
            r = rng.random()
            if r < 0.2:
                w = base._mutate(rng, w, False)
            elif r < 0.32 and len(w) <= 8:   # two words glued: pieces in the continuation role
                w = w + rng.choice(rng.choice(pools[:14]))
            elif 0.32 <= r < 0.36:   # an unseen character behind, inside or in front of a word
                u = rng.choice(UNSEEN)
                i = rng.choice((0, len(w) // 2, len(w), len(w)))
                w = w[:i] + u + w[i:]
            r = rng.random()
            sep = "" if r < 0.08 else rng.choice(SPACES) if r < 0.22 else rng.choice(base.PUNCT + WIDE_PUNCT) if r < 0.3 else " "
            parts += [w, sep]
        if rng.random() < 0.1:
            parts.insert(0, rng.choice([" ", "  ", "\n"]))
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


def generate(train=False):
    """-> ({file name: bytes}, stats); `train`: a new vocabulary, not the committed one"""
    os.environ["TOKENIZERS_PARALLELISM"] = "false"
    import tokenizers
    from tokenizers import Tokenizer, models, pre_tokenizers, trainers

    from daachorse_amd import bert_char_classes

    versions = {"tokenizers": tokenizers.__version__, "unidata_version": unicodedata.unidata_version}
    vocab_path = os.path.join(HERE, "tokenizer_wordpiece_vocab.json")
    if train or not os.path.exists(vocab_path):
        trainer_tok = Tokenizer(models.WordPiece(unk_token="[UNK]", max_input_chars_per_word=MAX_CHARS))
        trainer_tok.pre_tokenizer = pre_tokenizers.BertPreTokenizer()
        trainer = trainers.WordPieceTrainer(vocab_size=VOCAB_SIZE, min_frequency=1, special_tokens=["[UNK]"], show_progress=False, continuing_subword_prefix=PREFIX)
        corpus = base.training_corpus(KNOWN + WIDE_PUNCT + SYMBOLS + LONG + WIDE, 6000, SEED + 1)
        trainer_tok.train_from_iterator(corpus, trainer)
        vocab_str = json.loads(trainer_tok.to_str())["model"]["vocab"]
    else:
        with open(vocab_path, encoding="utf-8") as f:
            committed = json.load(f)
        assert (committed["prefix"], committed["max_input_chars_per_word"]) == (PREFIX, MAX_CHARS)
        vocab_str, versions = committed["vocab"], {**versions, "tokenizers": committed["versions"]["tokenizers"]}
        assert versions["tokenizers"] == tokenizers.__version__, "the committed vocabulary was trained by another version: --train"
    assert sorted(vocab_str.values()) == list(range(len(vocab_str))) and 1000 <= len(vocab_str) <= VOCAB_SIZE, len(vocab_str)
    unk_id = vocab_str["[UNK]"]
    tok = Tokenizer(models.WordPiece(vocab=vocab_str, unk_token="[UNK]", max_input_chars_per_word=MAX_CHARS, continuing_subword_prefix=PREFIX))
    tok.pre_tokenizer = pre_tokenizers.BertPreTokenizer()
    pre = pre_tokenizers.BertPreTokenizer()
    vocab = {k.encode(): i for k, i in vocab_str.items()}
    table = wg.class_table(bert_char_classes())

    docs = documents(SEED)
    for d in docs:
        for ch in d:
            assert ord(ch) >= 0x20 or ch in "\t\n\r\x0b\x0c", (d, hex(ord(ch)))
            assert unicodedata.category(ch) != "Cn", hex(ord(ch))
    doc_ids, doc_tok, doc_words = [], [], []
    n_words = n_unk = n_multi = n_long = n_wide = 0
    by_roles, by_partial, by_shortest = set(), set(), set()
    for d in docs:
        raw = d.encode()
        enc = tok.encode(d, add_special_tokens=False)
        ids, spans = enc.ids, byte_spans(d, enc.offsets)
        ws = byte_spans(d, [o for _, o in pre.pre_tokenize_str(d)])
        scan = wg.bert_scan(raw, table)
        assert [(s, e) for s, e, sp in scan if not sp] == ws, ("a: Split.Bert", d)
        assert all(raw[s:e].decode().isspace() for s, e, sp in scan if sp), ("a: the words dropped are whitespace", d)
        want = wg.wordpiece_doc(raw, table, vocab, unk_id, MAX_CHARS, PREFIX.encode())
        assert (ids, spans) == want, ("b: the definition", d)
        for s, e in ws:
            w = raw[s:e]
            right = wg.wordpiece(w, vocab, unk_id, MAX_CHARS, PREFIX.encode())
            chars = len(w.decode())
            n_words += 1
            n_unk += right == [(unk_id, 0, len(w))]
            n_multi += len(right) >= 2
            n_long += chars > MAX_CHARS
            n_wide += chars <= MAX_CHARS < len(w)
            if wg.wordpiece(w, vocab, unk_id, MAX_CHARS, PREFIX.encode(), roles=False) != right:
                by_roles.add(w)
            if wg.wordpiece(w, vocab, unk_id, MAX_CHARS, PREFIX.encode(), shortest=True) != right:
                by_shortest.add(w)
            if chars <= MAX_CHARS and right == [(unk_id, 0, len(w))] and any(w[:e] in vocab for e in range(1, len(w) + 1)):
                by_partial.add(w)
        doc_ids.append(ids)
        doc_tok.append(wg.pack_spans(spans))
        doc_words.append(wg.pack_spans(ws))
    sens = {"words": n_words, "words_unk": n_unk, "words_with_two_or_more_pieces": n_multi, "distinct_words_changed_by_ignoring_roles": len(by_roles),
            "distinct_words_with_a_first_piece_that_fail_later": len(by_partial), "words_above_max_chars": n_long,
            "words_within_max_chars_but_more_bytes": n_wide, "distinct_words_changed_by_shortest_first": len(by_shortest)}
    assert n_multi >= 200 and len(by_roles) >= 10 and len(by_partial) >= 10 and n_long >= 5 and n_wide >= 5 and len(by_shortest) >= 10, ("c", sens)
    assert n_unk * 10 <= n_words, ("at most 10 % [UNK]", sens)
    vocab_file = {"about": "WordPiece vocabulary trained by tokenizers.trainers.WordPieceTrainer on synthetic text; a key with the prefix is a "
                           "continuation piece", "versions": versions, "prefix": PREFIX, "unk_id": unk_id, "max_input_chars_per_word": MAX_CHARS,
                  "vocab": dict(sorted(vocab_str.items(), key=lambda kv: kv[1]))}
    cases_file = {"about": "tokenizers' ids (models.WordPiece behind BertPreTokenizer, no normalizer, no special tokens), token spans and "
                           "BertPreTokenizer's word spans per document, in bytes, packed as [gap, length, ..]",
                  "versions": versions, "sensitivity": sens, "docs": docs, "ids": doc_ids, "tok_spans": doc_tok, "word_spans": doc_words}
    files = {}
    for name, obj in (("tokenizer_wordpiece_vocab.json", vocab_file), ("tokenizer_wordpiece_cases.json", cases_file)):
        blob = (json.dumps(obj, ensure_ascii=False, separators=(",", ":")) + "\n").encode()
        assert len(blob) <= MAX_FILE, (name, len(blob))
        assert json.loads(blob) == obj
        files[name] = blob
    stats = {"docs": len(docs), "bytes": sum(len(d.encode()) for d in docs), "pieces": len(vocab_str), "tokens": sum(map(len, doc_ids)), **sens,
             "file_bytes": {k: len(v) for k, v in files.items()}}
    return files, stats


def main():
    check = "--check" in sys.argv[1:]
    files, stats = generate(train="--train" in sys.argv[1:] and not check)
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
