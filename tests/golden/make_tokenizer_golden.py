#!/usr/bin/env python3
"""Writes the tokenizer fixtures under tests/golden/ (data only): a byte-level BPE vocabulary trained by `tokenizers`, a unigram
vocabulary trained by `sentencepiece`, and what the two libraries make of a few hundred noisy documents.

    python tests/golden/make_tokenizer_golden.py            # writes the four files
    python tests/golden/make_tokenizer_golden.py --check    # regenerates in memory and compares with the committed bytes

Needs `sentencepiece`, `tokenizers` and `regex`, no GPU, and nothing of the library's kernels: from this repository it takes only the
sequential scanner of tests/test_split_host.py with char_classes() (pure Python; importing them needs the package built).  All text is
synthetic and every seed is fixed, so a second run writes the same bytes.

    tokenizer_bpe_vocab.json       pieces (hex of their bytes, id order; id = rank), the merges as pairs of ids
    tokenizer_bpe_cases.json       documents, per document `tokenizers`' ids and the word boundaries in bytes, per distinct word its ids
    tokenizer_unigram_vocab.json   pieces, float32 scores, unk_id
    tokenizer_unigram_cases.json   documents (as given to sentencepiece: with " ", not "▁"), per document sp.encode's ids; the same for
                                   a few documents whose best path is not unique (tie_docs)

Before anything is written the generator asserts, on every document (none is excluded):
  a. the words of `tokenizers`' ByteLevel pre-tokenizer == scan_batch(doc, Split.Gpt2, char_classes()) == the `regex` module's GPT-2
     pattern;
  b. a tiktoken-style rank merge (ranks looked up by the concatenated bytes, ties to the left) == `tokenizers` on every distinct word;
     a float32 Viterbi with one unknown edge per code point at min score - 10 == sentencepiece once runs of unk_id are collapsed, with
     the candidates into a position tried longest-first and shortest-first (the tie_docs: longest-first, which is the order of
     find_overlapping_iter and the one sentencepiece agrees with); `tokenizers`' Unigram rebuilt from the piece list == sentencepiece;
  c. the cases can tell a subtly wrong tokenizer from a right one: >= 10 distinct words change under a rightmost-tie rank merge, >= 10
     documents change under greedy longest-match instead of Viterbi, >= 20 documents hold a run of two or more unknown code points and
     >= 20 an isolated one.
"""
import io
import json
import os
import random
import sys
import unicodedata

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                    # tests/: test_split_host
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))   # the repository: daachorse_amd

SEED = 20261018
N_DOCS = 330
BPE_MERGES = 1500
UNIGRAM_PIECES = 1200
MAX_FILE = 64 * 1024
GPT2_PATTERN = r"'s|'t|'re|'ve|'m|'ll|'d| ?\p{L}+| ?\p{N}+| ?[^\s\p{L}\p{N}]+|\s+(?!\S)|\s+"
F = np.float32

# ------------------------------------------------------------------------------------------------------------------- the text
ENGLISH = """the of and to in is that it was for on are as with his they at be this from have or by one had not but what all were when
we there can an your which their said if do will each about how up out them then she many some so these would other into has more her
two like him see time could no make than first been its who now people my made over did down only way find use may water long little very
after words called just where most know get through back much before go good new write our used me man too any day same right look think
also around another came come work three word must because does part even place well such here take why things help put years different
away again off went old number great tell men say small every found still between name should home big give air line set own under read
last never us left end along while might next sound below saw something thought both few those always looked show large often together
asked house world going want school important until form food keep children feet land side without boy once animals life enough took""".split()
REPEATED = ["aaa", "aaaa", "aaaaa", "haha", "hahaha", "hahahaha", "ththth", "eeee", "eeeee", "ooo", "ooooo", "zzz", "zzzzz", "mmm", "hmmm", "lololol", "nanana",
            "banana", "bananana", "xoxoxo", "ababab", "abababa", "mississippi", "sisisi", "tototo", "ininin", "ererer", "ananan", "lalala", "nonono", "sss",
            "ааа", "хахаха", "ははは", "ááá", "ωωω"]
ACCENTED = ["café", "naïve", "über", "señor", "façade", "smörgåsbord", "crème", "piñata", "Zürich", "élève", "niño", "garçon", "fiancée", "søster", "mañana",
            "português", "français", "straße", "œuvre", "Ångström"]
GREEK = ["λόγος", "και", "το", "άλφα", "θεός", "άνθρωπος", "κόσμος", "είναι", "από", "φιλοσοφία", "Ελλάδα", "νερό"]
CYRILLIC = ["привет", "мир", "это", "как", "что", "хорошо", "спасибо", "да", "нет", "человек", "время", "Москва", "работа", "слово"]
CJK = ["世界", "日本語", "中文", "你好", "東京", "学生", "我们", "時間", "大学", "中国", "今日", "人", "水"]
KANA = ["こんにちは", "ありがとう", "カタカナ", "ひらがな", "です", "ます", "これ", "ラーメン", "さくら"]
HANGUL = ["한국어", "안녕", "사람", "감사", "서울"]
HEBREW = ["שלום", "עולם", "תודה", "ספר"]
ARABIC = ["سلام", "عالم", "كتاب", "شكرا", "مدينة"]
CONTRACTIONS = ["it's", "we'll", "don't", "I'm", "they've", "you're", "he'd", "that's", "can't", "she'll", "we've", "I'd", "let's", "who're"]
NUMBERS = ["1", "7", "42", "123", "2024", "3.14", "1000000", "0", "99", "１２３", "４５", "２０２４", "٣٤", "½"]
PUNCT = [".", ",", "!", "?", "...", "!!!", "???", "--", "-----", ":", ";", "(", ")", "\"", "'", "/", "&", "#1", "@", "%"]
SPACES = ["  ", "   ", "\n", "\n\n", "\t", " \n ", "　", "　　", " ", "    "]
EMOJI = "\U0001f600"   # one emoji, Unicode 6.1
# seen by the BPE trainer (it has every byte anyway) and kept from the unigram trainer, so that sentencepiece meets unknown code points
UNSEEN_BY_UNIGRAM = HANGUL + HEBREW + [EMOJI, EMOJI + EMOJI, "１２３", "４５", "２０２４", "ωωω", "½", "œuvre", "Ångström", "٣٤"]
KNOWN_WORDS = ENGLISH + REPEATED + ACCENTED + GREEK + CYRILLIC + CJK + KANA + ARABIC + CONTRACTIONS + NUMBERS
ALL_WORDS = KNOWN_WORDS + HANGUL + HEBREW + [EMOJI]
# documents with several best unigram segmentations of one score (-|--|-- and --|--|-): kept apart from the unigram documents, whose
# result must not depend on the order in which the candidates into a position are tried
TIE_DOCS = ["-----", "ssss", "we'lll", "aaaa", "1000000", "-----of 1000000 ", "ooooo zzzzz", "hahahaha lll", "eeeee mmm!!!", "ááá ааа"]


def _assigned_long_ago():
    """every code point of the corpus has had its category since Unicode 6.1 or earlier (the oldest this check can see is the running
    Python's own table; the word lists above were chosen by hand from blocks of Unicode 1.1 .. 6.1)"""
    for w in ALL_WORDS + PUNCT + SPACES:
        for ch in w:
            assert unicodedata.category(ch) != "Cn" and (ord(ch) < 0x3100 or 0x4E00 <= ord(ch) < 0xD7A4 or 0xFF00 <= ord(ch) < 0xFFF0 or ch == EMOJI), hex(ord(ch))


def _repeats(w):
    """a character or a pair of characters comes twice in a row"""
    return any(w[i] == w[i + 1] for i in range(len(w) - 1)) or any(w[i:i + 2] == w[i + 2:i + 4] for i in range(len(w) - 3))


def _weights(rng, words):
    return [1.0 / (1 + i) ** 0.7 for i in range(len(words))]


def _sentence(rng, words, weights, n):
    out = []
    for w in rng.choices(words, weights, k=n):
        out.append(w)
        if rng.random() < 0.12:
            out.append(rng.choice(PUNCT))
    return " ".join(out)


def training_corpus(words, n, seed):
    rng = random.Random(seed)
    order = words[:]
    rng.shuffle(order)
    order = ENGLISH[:60] + [w for w in order if w not in ENGLISH[:60]]
    weights = _weights(rng, order)
    rep = [w for w in REPEATED if w in words]
    return [_sentence(rng, order, weights, rng.randrange(3, 14)) for _ in range(n)] + [" ".join(rng.choices(rep, k=6)) for _ in range(n // 10)]


def _mutate(rng, w, plain):
    """a word the trainers have not seen: a character dropped, doubled (not with `plain`), swapped or replaced"""
    if len(w) < 2:
        return w + "e"
    i = rng.randrange(len(w))
    how = rng.randrange(4)
    if how == 0:
        return w[:i] + w[i + 1:]
    if how == 1 and not plain:
        return w[:i] + w[i] + w[i:]
    if how == 2 and i + 1 < len(w):
        return w[:i] + w[i + 1] + w[i] + w[i + 2:]
    return w[:i] + rng.choice("aeiostnжあ世é") + w[i + 1:]


def documents(seed, plain=False):
    """N_DOCS noisy documents; a few are empty, the rest hold up to 8 words from every list, some of them mutated.  `plain`: without the
    words that repeat a pair (aaa, -----, 1000000): they have several best segmentations of one score (a|aa, aa|a), which TIE_DOCS cover"""
    rng = random.Random(seed)
    pools = [ENGLISH] * 6 + [REPEATED] * 3 + [ACCENTED, GREEK, CYRILLIC, CJK, KANA, HANGUL, HEBREW, ARABIC, CONTRACTIONS, CONTRACTIONS, NUMBERS, PUNCT, [EMOJI]]
    if plain:
        pools = [[w for w in pool if not _repeats(w)] for pool in pools if pool is not REPEATED]
    docs = []
    for k in range(N_DOCS):
        if k in (5, 100, N_DOCS - 1):
            docs.append("")
            continue
        parts = []
        for _ in range(rng.randrange(1, 9)):
            w = rng.choice(rng.choice(pools))
            if rng.random() < 0.2:
                w = _mutate(rng, w, plain)
            r = rng.random()
            sep = "" if r < 0.08 else rng.choice(SPACES) if r < 0.22 else " "
            parts += [w, sep]
        if rng.random() < 0.1:
            parts.insert(0, rng.choice([" ", "  ", "\n"]))
        if rng.random() < 0.6:
            parts.pop()   # no trailing separator
        docs.append("".join(parts))
    return docs


# -------------------------------------------------------------------------------------------------------- GPT-2's byte alphabet
def bytes_to_unicode():
    """the printable stand-in of every byte, as GPT-2's encoder.py and the ByteLevel pre-tokenizer define it"""
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(0xA1, 0xAD)) + list(range(0xAE, 0x100))
    cs, n = bs[:], 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return {b: chr(c) for b, c in zip(bs, cs)}


B2U = bytes_to_unicode()
U2B = {u: b for b, u in B2U.items()}


def unmap(s):
    return bytes(U2B[ch] for ch in s)


# --------------------------------------------------------------------------------------------------------- the restatements
def rank_merge(word, rank_of, rightmost=False):
    """tiktoken's byte_pair_merge: parts start as single bytes; the neighbouring pair whose concatenated bytes have the lowest rank is
    merged, ties to the left (`rightmost`: to the right, the wrong rule), until no pair is in the vocabulary -> ids"""
    b = list(range(len(word) + 1))
    while True:
        best, at = None, None
        for i in range(len(b) - 2):
            r = rank_of.get(word[b[i]:b[i + 2]])
            if r is not None and (best is None or r < best or (rightmost and r == best)):
                best, at = r, i
        if at is None:
            break
        del b[at + 1]
    return [rank_of[word[s:e]] for s, e in zip(b, b[1:])]


def viterbi(doc, piece_id, scores, unk, unk_id, max_len, longest_first):
    """float32 Viterbi over the byte positions of doc (bytes): the pieces that end at q are tried longest-first or shortest-first, then
    the unknown edge of the code point that ends at q; a candidate replaces the incumbent only when strictly greater -> ids"""
    L = len(doc)
    ninf = F(-np.inf)
    best = [ninf] * (L + 1)
    best[0] = F(0.0)
    back = [None] * (L + 1)
    cuts = [p for p in range(L) if (doc[p] & 0xC0) != 0x80] + [L]
    prev = {c1: c0 for c0, c1 in zip(cuts, cuts[1:])}
    for q in range(1, L + 1):
        inc, edge = ninf, None
        starts = range(max(0, q - max_len), q)
        for s in (starts if longest_first else reversed(starts)):
            v = piece_id.get(doc[s:q])
            if v is None or best[s] == ninf:
                continue
            c = best[s] + scores[v]
            if c > inc:
                inc, edge = c, (v, s)
        if q in prev and best[prev[q]] != ninf:
            c = best[prev[q]] + unk
            if c > inc:
                inc, edge = c, (unk_id, prev[q])
        best[q], back[q] = inc, edge
    ids, q = [], L
    while q > 0:
        ids.append(back[q][0])
        q = back[q][1]
    return ids[::-1]


def greedy(doc, piece_id, unk_id, max_len):
    """longest match first, an unknown code point where nothing matches -> ids"""
    ids, p, L = [], 0, len(doc)
    while p < L:
        for e in range(min(L, p + max_len), p, -1):
            if doc[p:e] in piece_id:
                ids.append(piece_id[doc[p:e]])
                p = e
                break
        else:
            ids.append(unk_id)
            p += 1
            while p < L and (doc[p] & 0xC0) == 0x80:
                p += 1
    return ids


def collapse(ids, unk_id):
    return [v for i, v in enumerate(ids) if v != unk_id or i == 0 or ids[i - 1] != unk_id]


def unknown_runs(ids, unk_id):
    """the lengths of the runs of unk_id"""
    runs, n = [], 0
    for v in ids + [None]:
        if v == unk_id:
            n += 1
        elif n:
            runs.append(n)
            n = 0
    return runs


# ------------------------------------------------------------------------------------------------------------------------ BPE
def make_bpe(docs, versions):
    import regex
    from tokenizers import Tokenizer, models, pre_tokenizers, trainers

    from daachorse_amd import Split, char_classes
    from test_split_host import scan_batch

    tok = Tokenizer(models.BPE())
    tok.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False, use_regex=True)
    trainer = trainers.BpeTrainer(vocab_size=256 + BPE_MERGES, min_frequency=2, special_tokens=[], show_progress=False,
                                  initial_alphabet=sorted(pre_tokenizers.ByteLevel.alphabet()))
    tok.train_from_iterator(training_corpus(ALL_WORDS, 6000, SEED + 1), trainer)
    model = json.loads(tok.to_str())["model"]
    vocab = model["vocab"]
    pieces = [None] * len(vocab)
    for s, i in vocab.items():
        pieces[i] = unmap(s)
    assert None not in pieces and len(set(pieces)) == len(pieces)
    assert sorted(pieces[:256]) == [bytes([b]) for b in range(256)], "ids 0 .. 255 are the byte alphabet"
    merges = [m.split(" ") if isinstance(m, str) else m for m in model["merges"]]
    assert len(merges) == len(pieces) - 256 >= 1000, len(merges)
    pairs = []
    for i, (a, b) in enumerate(merges):
        assert vocab[a + b] == 256 + i, "merge i produces id 256 + i"
        pairs.append([vocab[a], vocab[b]])
    rank_of = {p: i for i, p in enumerate(pieces)}

    gpt2 = regex.compile(GPT2_PATTERN)
    cc = char_classes()
    doc_ids, doc_bounds, words = [], [], {}
    for d in docs:
        raw = d.encode()
        ws = [unmap(w) for w, _ in tok.pre_tokenizer.pre_tokenize_str(d)]
        assert b"".join(ws) == raw, d
        bounds = [0]
        for w in ws:
            bounds.append(bounds[-1] + len(w))
        assert [w.decode() for w in ws] == gpt2.findall(d), ("a: regex", d)
        wo, dw = scan_batch([raw], Split.Gpt2, cc)
        assert wo.tolist() == (bounds if raw else [0]) and dw.tolist() == [0, len(ws)], ("a: scan_batch", d)
        ids = tok.encode(d, add_special_tokens=False).ids
        per_word = []
        for w in ws:
            if w not in words:
                words[w] = tok.encode(w.decode(), add_special_tokens=False).ids
                assert rank_merge(w, rank_of) == words[w], ("b: rank merge", w)
                assert b"".join(pieces[i] for i in words[w]) == w
            per_word += words[w]
        assert per_word == ids, d
        doc_ids.append(ids)
        doc_bounds.append(bounds)
    changed = sorted(w for w in words if rank_merge(w, rank_of, rightmost=True) != words[w])
    assert len(changed) >= 10, ("c: rightmost ties", len(changed))
    assert max(len(w) for w in words) <= 64
    order = sorted(words)
    sens = {"words_changed_by_rightmost_ties": len(changed)}
    vocab_file = {"about": "byte-level BPE trained by tokenizers.trainers.BpeTrainer on synthetic text; id = rank; pieces are hex of their bytes",
                  "versions": versions, "pieces_hex": [p.hex() for p in pieces], "merges": pairs}
    cases_file = {"about": "tokenizers' ids (ByteLevel, add_prefix_space=False, use_regex=True, no special tokens) and byte word boundaries per "
                           "document; per distinct word its ids",
                  "versions": versions, "sensitivity": sens, "docs": docs, "ids": doc_ids, "word_bounds": doc_bounds,
                  "words": [w.decode() for w in order], "word_ids": [words[w] for w in order]}
    stats = {"bpe_pieces": len(pieces), "bpe_tokens": sum(map(len, doc_ids)), "distinct_words": len(words), "longest_word": max(len(w) for w in words), **sens}
    return vocab_file, cases_file, stats


# -------------------------------------------------------------------------------------------------------------------- unigram
def make_unigram(docs, versions):
    import sentencepiece as spm
    from tokenizers import Tokenizer, models

    known = [w for w in KNOWN_WORDS if w not in UNSEEN_BY_UNIGRAM]
    model = io.BytesIO()
    spm.SentencePieceTrainer.train(sentence_iterator=iter(training_corpus(known, 6000, SEED + 2)), model_writer=model, vocab_size=UNIGRAM_PIECES,
                                   model_type="unigram", normalization_rule_name="identity", add_dummy_prefix=False, remove_extra_whitespaces=False,
                                   bos_id=-1, eos_id=-1, hard_vocab_limit=False, character_coverage=1.0, num_threads=1, minloglevel=2)
    sp = spm.SentencePieceProcessor(model_proto=model.getvalue())
    n = sp.get_piece_size()
    unk_id = sp.unk_id()
    pieces = [sp.id_to_piece(i) for i in range(n)]
    scores = [sp.get_score(i) for i in range(n)]
    assert all(float(F(s)) == s for s in scores) and len(set(pieces)) == n
    assert all(sp.is_unknown(i) == (i == unk_id) and not sp.is_control(i) and not sp.is_unused(i) and not sp.is_byte(i) for i in range(n))
    sc = np.array(scores, dtype=np.float32)
    unk = F(min(s for i, s in enumerate(sc) if i != unk_id)) - F(10.0)
    piece_id = {p.encode(): i for i, p in enumerate(pieces) if i != unk_id}
    max_len = max(map(len, piece_id))

    hf = Tokenizer(models.Unigram(vocab=list(zip(pieces, scores)), unk_id=unk_id))
    tie_ids, n_order = [], 0
    for d in TIE_DOCS:   # several best paths of one score: sentencepiece takes the one that longest-first takes
        raw = d.replace(" ", "▁").encode()
        long_first = viterbi(raw, piece_id, sc, unk, unk_id, max_len, True)
        n_order += long_first != viterbi(raw, piece_id, sc, unk, unk_id, max_len, False)
        tie_ids.append(sp.encode(d))
        assert collapse(long_first, unk_id) == tie_ids[-1], ("b: viterbi, longest first", d)
        assert hf.encode(d.replace(" ", "▁"), add_special_tokens=False).ids == tie_ids[-1], ("b: tokenizers' Unigram", d)
    assert n_order >= 3, n_order
    doc_ids, n_greedy, n_run, n_single = [], 0, 0, 0
    for d in docs:
        want = sp.encode(d)
        raw = d.replace(" ", "▁").encode()
        long_first = viterbi(raw, piece_id, sc, unk, unk_id, max_len, True)
        short_first = viterbi(raw, piece_id, sc, unk, unk_id, max_len, False)
        assert long_first == short_first, ("b: the path depends on the candidate order: change the seed", d)
        assert collapse(long_first, unk_id) == want, ("b: viterbi", d)
        assert hf.encode(d.replace(" ", "▁"), add_special_tokens=False).ids == want, ("b: tokenizers' Unigram", d)
        n_greedy += collapse(greedy(raw, piece_id, unk_id, max_len), unk_id) != want
        runs = unknown_runs(long_first, unk_id)
        n_run += any(r >= 2 for r in runs)
        n_single += 1 in runs
        doc_ids.append(want)
    assert n_greedy >= 10 and n_run >= 20 and n_single >= 20, ("c", n_greedy, n_run, n_single)
    sens = {"docs_changed_by_greedy_longest_match": n_greedy, "docs_with_an_unknown_run": n_run, "docs_with_an_isolated_unknown": n_single,
            "tie_docs_changed_by_shortest_first": n_order}
    vocab_file = {"about": "unigram model trained by sentencepiece (identity normalization, no dummy prefix, extra whitespace kept, no bos/eos); "
                           "scores are float32 values; the piece at unk_id is no piece of the text",
                  "versions": versions, "unk_id": unk_id, "pieces": pieces, "scores": scores}
    cases_file = {"about": "sp.encode ids per document; documents as given to sentencepiece (the caller of a byte automaton replaces ' ' by U+2581)",
                  "versions": versions, "sensitivity": sens, "docs": docs, "ids": doc_ids, "tie_docs": TIE_DOCS, "tie_ids": tie_ids}
    stats = {"unigram_pieces": n, "unigram_tokens": sum(map(len, doc_ids)), **sens}
    return vocab_file, cases_file, stats


def generate():
    """-> ({file name: bytes}, stats)"""
    os.environ["TOKENIZERS_PARALLELISM"] = "false"
    import regex
    import sentencepiece
    import tokenizers

    _assigned_long_ago()
    versions = {"sentencepiece": sentencepiece.__version__, "tokenizers": tokenizers.__version__, "regex": regex.__version__,
                "unidata_version": unicodedata.unidata_version}
    docs = documents(SEED)
    assert len(docs) >= 257
    bv, bc, s1 = make_bpe(docs, versions)
    uv, uc, s2 = make_unigram(documents(SEED + 5, plain=True), versions)
    files = {}
    for name, obj in (("tokenizer_bpe_vocab.json", bv), ("tokenizer_bpe_cases.json", bc), ("tokenizer_unigram_vocab.json", uv), ("tokenizer_unigram_cases.json", uc)):
        blob = (json.dumps(obj, ensure_ascii=False, separators=(",", ":")) + "\n").encode()
        assert len(blob) < MAX_FILE, (name, len(blob))
        assert json.loads(blob) == obj   # (float32 scores included: a double holds them exactly)
        files[name] = blob
    stats = {"docs": len(docs), "bytes": sum(len(d.encode()) for d in docs), **s1, **s2, "file_bytes": {k: len(v) for k, v in files.items()}}
    return files, stats


def main():
    files, stats = generate()
    check = "--check" in sys.argv[1:]
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
