#!/usr/bin/env python3
"""Writes tests/golden/pack_cases.json (data only): what `tokenizers` makes of token lists with TemplateProcessing, enable_truncation
and enable_padding, in three blocks.

    python tests/golden/make_pack_golden.py            # writes the file
    python tests/golden/make_pack_golden.py --check    # regenerates in memory and compares with the committed bytes

Needs `tokenizers`, no GPU and nothing of the library: from this repository it takes the pure-Python definition tests/pack_golden.py,
the committed vocabularies and the documents of normalize_cases.json.  Every seed is fixed.

1. "cases": seeded token lists over a WordLevel vocabulary (word i is "w<i>", documents are words joined by single spaces, so a
   token's span is its word's), run as batches through three templates (none; BERT's [CLS] A [SEP] B [SEP] with type ids 0 / 1;
   RoBERTa's <s> A </s> </s> B </s>), every strategy and direction, and padding longest, fixed, to a multiple of 8 and none, on either
   side.  Pairs and singles.  A case holds its template's name, what its configuration changes of "defaults", the id lists and the
   recorded planes — the ids, the masks and type ids as one string of digits a row (an index into "table", the distinct rows) and the
   offsets of the slots that are tokens (a special's and a padding slot's are (0, 0), asserted here) —, or "error": the first pair
   that only_first / only_second cannot truncate, where `tokenizers` refuses the whole batch.
2. "bert": BertNormalizer + BertPreTokenizer + WordPiece over tokenizer_wordpiece_vocab.json with [CLS] A [SEP], max_length 16 and
   padding longest, over the documents of normalize_cases.json: the ids in front of the padding (which holds [PAD], asserted here), type
   ids, both masks and the offsets as byte spans of the raw document (packed as [gap, length, ..] over the row's tokens, or {raw: ..}
   where tokens share a source character).
3. "roberta": byte-level BPE over tokenizer_bpe_vocab.json with <s> A </s>, max_length 16 and truncation on the left, padding
   longest, over the first documents of the same list: ids, type ids and both masks.  The offsets are not recorded: the pieces tile
   the document (asserted here), so a token's span follows from the lengths of the pieces in front of it.

Before anything is written the generator asserts, on every case (none is excluded), that pack_golden.pack equals `tokenizers` on every
plane, and that the cases discriminate: at least 20 pairs reach the halving branch of longest_first with n1 > n2, at least 20
truncate only the longer sequence, at least 10 pairs hit the only_first / only_second error, and some cases have budget 0.  The one
deliberate difference that can show — a row longer than a fixed length, where `tokenizers` returns a ragged batch and the definition
widens L — is marked "definition_only", kept to at most 5 % of the cases and checked against the definition alone."""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))   # tests/: pack_golden, normalize_golden, wordpiece_golden

import make_tokenizer_golden as base  # noqa: E402
import normalize_golden as ng  # noqa: E402
import pack_golden as pg  # noqa: E402
import wordpiece_golden as wg  # noqa: E402

SEED = 20261022
MAX_FILE = 64 * 1024
N_WORDS = 40
CLS, SEP, BOS, EOS, PAD = 40, 41, 42, 43, 44
TEMPLATES = {
    "none": ([["A", 0, 0]], [["A", 0, 0], ["B", 0, 1]]),
    "bert": ([["special", CLS, 0], ["A", 0, 0], ["special", SEP, 0]],
             [["special", CLS, 0], ["A", 0, 0], ["special", SEP, 0], ["B", 0, 1], ["special", SEP, 1]]),
    "roberta": ([["special", BOS, 0], ["A", 0, 0], ["special", EOS, 0]],
                [["special", BOS, 0], ["A", 0, 0], ["special", EOS, 0], ["special", EOS, 0], ["B", 0, 0], ["special", EOS, 0]]),
}
PADDINGS = [("longest", None), (14, None), ("longest", 8), (None, None)]
N_ROBERTA_DOCS = 80


def wordlevel(template):
    from tokenizers import Tokenizer, models, pre_tokenizers, processors

    vocab = {pg.word(i): i for i in range(N_WORDS)}
    vocab.update({"[CLS]": CLS, "[SEP]": SEP, "<s>": BOS, "</s>": EOS, "[PAD]": PAD, "[UNK]": PAD + 1})
    tok = Tokenizer(models.WordLevel(vocab, unk_token="[UNK]"))
    tok.pre_tokenizer = pre_tokenizers.WhitespaceSplit()
    if template == "bert":
        tok.post_processor = processors.TemplateProcessing(single="[CLS] $A [SEP]", pair="[CLS] $A [SEP] $B:1 [SEP]:1", special_tokens=[("[CLS]", CLS), ("[SEP]", SEP)])
    elif template == "roberta":
        tok.post_processor = processors.TemplateProcessing(single="<s> $A </s>", pair="<s> $A </s> </s> $B </s>", special_tokens=[("<s>", BOS), ("</s>", EOS)])
    return tok


def configure(tok, cfg):
    if cfg["max_length"] is None:
        tok.no_truncation()
    else:
        tok.enable_truncation(cfg["max_length"], stride=0, strategy=cfg["strategy"], direction=cfg["truncation_side"])
    if cfg["padding"] is None:
        tok.no_padding()
    else:
        tok.enable_padding(direction=cfg["padding_side"], pad_id=cfg["pad_id"], pad_type_id=cfg["pad_type_id"], pad_token="[PAD]",
                           length=None if cfg["padding"] == "longest" else cfg["padding"], pad_to_multiple_of=cfg["pad_to_multiple_of"])


def text(ids):
    return " ".join(pg.word(i) for i in ids)


def encoded_rows(encs, byte_offsets=None):
    """`tokenizers`' encodings -> rows of (ids, types, attention, special, flat offsets)"""
    out = []
    for k, e in enumerate(encs):
        offs = e.offsets if byte_offsets is None else byte_offsets(k, e)
        out.append((list(e.ids), list(e.type_ids), list(e.attention_mask), list(e.special_tokens_mask), [x for s in offs for x in s]))
    return out


def same_as_definition(rows, planes, csr):
    """asserts `tokenizers`' rows equal the definition's planes"""
    import numpy as np
    names = ("input_ids", "token_type_ids", "attention_mask", "special_tokens_mask", "offsets")
    if csr:
        assert [len(r[0]) for r in rows] == np.diff(planes["row_offsets"].astype(np.int64)).tolist()
        for j, name in enumerate(names):
            if name == "attention_mask":
                assert all(x == 1 for r in rows for x in r[2])
                continue
            flat = [x for r in rows for x in r[j]]
            assert planes[name].reshape(-1).tolist() == flat, name
        return
    for j, name in enumerate(names):
        assert [planes[name][i].reshape(-1).tolist() for i in range(len(rows))] == [r[j] for r in rows], name


class Table:
    """the distinct digit rows of a plane, and a row's index among them"""

    def __init__(self):
        self.rows, self.at = [], {}

    def add(self, digits):
        s = "".join(str(x) for x in digits)
        assert all(0 <= x <= 9 for x in digits)
        if s not in self.at:
            self.at[s] = len(self.rows)
            self.rows.append(s)
        return self.at[s]


def lengths_for(rng, kind, budget):
    """(n1, n2) of a pair that takes the named way through truncation under `budget` (> 0)"""
    if kind == "halve":       # both above half the budget, n1 > n2
        n2 = rng.randrange(budget // 2 + 1, budget + 4)
        return n2 + rng.randrange(1, 4), n2
    if kind == "longer":      # the shorter fits beside a cut of the longer
        a = rng.randrange(0, max(1, budget // 2))
        b = budget - a + rng.randrange(1, 6)
        return (a, b) if rng.random() < 0.5 else (b, a)
    if kind == "fits":
        a = rng.randrange(0, budget + 1)
        return a, rng.randrange(0, budget - a + 1)
    if kind == "first_short":   # only_first cannot: n1 <= need
        n1 = rng.randrange(0, 3)
        return n1, budget + rng.randrange(0, 4)
    if kind == "second_short":
        n2 = rng.randrange(0, 3)
        return budget + rng.randrange(0, 4), n2
    return rng.randrange(0, 15), rng.randrange(0, 15)


def block_cases(stats):
    rng = random.Random(SEED)
    toks = {name: wordlevel(name) for name in TEMPLATES}
    cases, k = [], 0

    def ids(n):
        return [rng.randrange(N_WORDS) for _ in range(n)]

    def add(template, pair, lens, **kw):
        nonlocal k
        single, pair_t = TEMPLATES[template]
        pad, mult = PADDINGS[k % 4]
        side = "left" if (k // 4) % 2 else "right"
        k += 1
        cfg = pg.config(single=single, pair=pair_t, pad_id=PAD, pad_type_id=(k % 3 == 0) * 1, **{"padding": pad, "pad_to_multiple_of": mult, "padding_side": side, **kw})
        a = [ids(n1) for n1, _ in lens]
        b = [ids(n2) for _, n2 in lens] if pair else None
        cases.append(record(toks[template], template, cfg, a, b, stats))

    for template in TEMPLATES:
        n_added = sum(p[0] == "special" for p in TEMPLATES[template][1])
        for strategy in ("longest_first", "only_first", "only_second"):
            for side in ("right", "left"):
                max_length = n_added + rng.choice([7, 8, 9, 11])
                budget = max_length - n_added
                kw = dict(max_length=max_length, strategy=strategy, truncation_side=side)
                if strategy == "longest_first":
                    for _ in range(2):
                        add(template, True, [lengths_for(rng, w, budget) for w in ("halve", "longer", "halve", "longer")], **kw)
                else:
                    ok = []
                    while len(ok) < 4:   # pairs the strategy can truncate, and one that fits
                        n1, n2 = lengths_for(rng, rng.choice(["halve", "longer", "fits"]), budget)
                        if pg.truncate(n1, n2, True, budget, strategy) is not None:
                            ok.append((n1, n2))
                    add(template, True, ok, **kw)
                    short = "first_short" if strategy == "only_first" else "second_short"
                    add(template, True, [ok[0], lengths_for(rng, short, budget), ok[1], lengths_for(rng, short, budget)], **kw)
    for template in TEMPLATES:   # singles
        n_added = sum(p[0] == "special" for p in TEMPLATES[template][0])
        for side in ("right", "left"):
            add(template, False, [(rng.randrange(0, 16), 0) for _ in range(4)], max_length=n_added + rng.choice([5, 8]), truncation_side=side)
        add(template, False, [(rng.randrange(0, 9), 0) for _ in range(3)])
    for template in ("bert", "roberta"):   # budget 0
        for pair in (True, False):
            n_added = sum(p[0] == "special" for p in TEMPLATES[template][1 if pair else 0])
            add(template, pair, [(3, 2), (0, 5), (4, 0)], max_length=n_added, strategy=rng.choice(["longest_first", "only_first", "only_second"]) if pair else "longest_first")
    # a row longer than the fixed length: the definition widens L
    add("bert", True, [(9, 8), (1, 2)], padding=14, pad_to_multiple_of=None)
    add("none", False, [(17, 0), (3, 0)], padding=14, pad_to_multiple_of=None)
    return cases


def record(tok, template, cfg, a, b, stats):
    import numpy as np
    configure(tok, cfg)
    pair = b is not None
    inputs = [(text(x), text(y)) for x, y in zip(a, b)] if pair else [text(x) for x in a]
    seq_a, seq_b = pg.sequence(a), pg.sequence(b) if pair else None
    case = {"template": template, "config": {k: v for k, v in cfg.items() if k not in ("single", "pair") and v != pg.DEFAULTS[k]}, "a": a, "b": b}
    n_added = sum(p[0] == "special" for p in (cfg["pair"] if pair else cfg["single"]))
    if cfg["max_length"] is not None:
        budget = cfg["max_length"] - n_added
        stats["budget_0"] += budget == 0
        for x, y in zip(a, b if pair else [[]] * len(a)):
            n1, n2 = len(x), len(y)
            if pair and budget and n1 + n2 > budget:
                kept = pg.truncate(n1, n2, True, budget, cfg["strategy"])
                if cfg["strategy"] == "longest_first":
                    lo = min(n1, n2)
                    halved = (lo if lo > budget else max(lo, budget - lo)) + lo > budget
                    stats["halved_n1_above_n2"] += halved and n1 > n2
                    stats["only_the_longer_cut"] += (not halved) and min(kept) == lo
                stats["pairs_in_error"] += kept is None
    # what `tokenizers` says of every pair on its own: the first it refuses
    refused = None
    for i, x in enumerate(inputs):
        try:
            tok.encode(*x) if pair else tok.encode(x)
        except Exception:
            refused = i
            break
    try:
        want = pg.pack(seq_a, seq_b, cfg)
        assert refused is None, ("tokenizers refuses, the definition does not", cfg, a, b)
    except pg.PackError as e:
        assert e.doc is not None and e.doc == refused, (e, refused)
        try:
            tok.encode_batch(inputs)
            raise AssertionError("tokenizers takes the batch")
        except AssertionError:
            raise
        except Exception:
            pass
        case["error"] = refused
        stats["error_cases"] += 1
        return case
    csr = cfg["padding"] is None
    rows = encoded_rows(tok.encode_batch(inputs))
    ragged = not csr and len({len(r[0]) for r in rows}) > 1
    if ragged:
        assert cfg["padding"] != "longest" and max(len(r[0]) for r in rows) > cfg["padding"]
        case["definition_only"] = True
        stats["definition_only"] += 1
        n, L = want["input_ids"].shape
        rows = [tuple(want[name][i].reshape(-1).tolist() for name in ("input_ids", "token_type_ids", "attention_mask", "special_tokens_mask", "offsets")) for i in range(n)]
    else:
        same_as_definition(rows, want, csr)
    case["want"] = rows
    return case


def compact(cases):
    """the rows of every case with their digit planes out of one table"""
    table = Table()
    for c in cases:
        rows = c.pop("want", None)
        if rows is None:
            continue
        w = {"ids": [r[0] for r in rows], "types": [table.add(r[1]) for r in rows], "special": [table.add(r[3]) for r in rows],
             "token_offsets": [[x for j in range(len(r[0])) if not r[3][j] for x in r[4][2 * j:2 * j + 2]] for r in rows]}
        assert all(r[4][2 * j:2 * j + 2] == [0, 0] for r in rows for j in range(len(r[0])) if r[3][j])
        if c["config"].get("padding", "longest") is not None:
            w["attention"] = [table.add(r[2]) for r in rows]
        c["want"] = w
    return table.rows


def unpadded(rows, pad):
    """the ids of every row where attention is 1 (padding is on the right and holds `pad`)"""
    for r in rows:
        n = sum(r[2])
        assert r[2] == [1] * n + [0] * (len(r[0]) - n) and r[0][n:] == [pad] * (len(r[0]) - n)
    return [r[0][:sum(r[2])] for r in rows]


def base_byte_spans(text_, spans):
    at = [0]
    for ch in text_:
        at.append(at[-1] + len(ch.encode()))
    return [(at[s], at[e]) for s, e in spans]


def block_bert(docs):
    from tokenizers import AddedToken, Tokenizer, models, normalizers, pre_tokenizers, processors

    v = wg.load("vocab")
    tok = Tokenizer(models.WordPiece(vocab=v["vocab"], unk_token="[UNK]", max_input_chars_per_word=v["max_input_chars_per_word"], continuing_subword_prefix=v["prefix"]))
    tok.normalizer = normalizers.BertNormalizer()
    tok.pre_tokenizer = pre_tokenizers.BertPreTokenizer()
    names = ["[CLS]", "[SEP]", "[PAD]"]
    tok.add_special_tokens([AddedToken(t, special=True) for t in names])
    spec = [[t, tok.token_to_id(t)] for t in names]
    assert [i for _, i in spec] == list(range(len(v["vocab"]), len(v["vocab"]) + 3))
    cls, sep, pad = (i for _, i in spec)
    tok.post_processor = processors.TemplateProcessing(single="[CLS] $A [SEP]", pair="[CLS] $A [SEP] $B:1 [SEP]:1", special_tokens=[("[CLS]", cls), ("[SEP]", sep)])
    cfg = pg.config(single=[["special", cls, 0], ["A", 0, 0], ["special", sep, 0]], max_length=16, pad_id=pad)
    tok.enable_truncation(16)
    tok.enable_padding(pad_id=pad, pad_token="[PAD]")
    rows = encoded_rows(tok.encode_batch(docs), lambda k, e: base_byte_spans(docs[k], e.offsets))
    # the definition over the untruncated tokens the other fixture holds gives the same planes
    ids, spans = ng.tokens()
    seq = [[(i, s, e) for i, (s, e) in zip(a, b)] for a, b in zip(ids, spans)]
    same_as_definition(rows, pg.pack(seq, None, cfg), False)
    table = Table()
    offsets = []
    for r in rows:
        sp = [(r[4][2 * j], r[4][2 * j + 1]) for j in range(len(r[0])) if not r[3][j]]
        offsets.append(wg.pack_spans(sp) if all(x[1] <= y[0] for x, y in zip(sp, sp[1:])) else {"raw": sp})
    return {"specials": spec, "config": cfg, "row_length": len(rows[0][0]), "ids": unpadded(rows, pad), "types": [table.add(r[1]) for r in rows],
            "attention": [table.add(r[2]) for r in rows], "special": [table.add(r[3]) for r in rows], "token_offsets": offsets, "table": table.rows}


def block_roberta(docs):
    from tokenizers import AddedToken, Tokenizer, models, pre_tokenizers, processors

    with open(os.path.join(HERE, "tokenizer_bpe_vocab.json"), encoding="utf-8") as f:
        v = json.load(f)
    pieces = [bytes.fromhex(h) for h in v["pieces_hex"]]
    mapped = ["".join(base.B2U[b] for b in p) for p in pieces]
    tok = Tokenizer(models.BPE(vocab={m: i for i, m in enumerate(mapped)}, merges=[(mapped[a], mapped[b]) for a, b in v["merges"]]))
    tok.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False, use_regex=True)
    plain = [tok.encode(d, add_special_tokens=False).ids for d in docs]
    for d, p in zip(docs, plain):
        assert b"".join(pieces[i] for i in p) == d.encode(), "the pieces tile the document"
    names = ["<s>", "</s>", "<pad>"]
    tok.add_special_tokens([AddedToken(t, special=True) for t in names])
    spec = [[t, tok.token_to_id(t)] for t in names]
    assert [i for _, i in spec] == list(range(len(pieces), len(pieces) + 3))
    bos, eos, pad = (i for _, i in spec)
    tok.post_processor = processors.TemplateProcessing(single="<s> $A </s>", pair="<s> $A </s> </s> $B </s>", special_tokens=[("<s>", bos), ("</s>", eos)])
    cfg = pg.config(single=[["special", bos, 0], ["A", 0, 0], ["special", eos, 0]], max_length=16, truncation_side="left", pad_id=pad)
    tok.enable_truncation(16, direction="left")
    tok.enable_padding(pad_id=pad, pad_token="<pad>")
    rows = encoded_rows(tok.encode_batch(docs))
    seq = []
    for p in plain:
        doc, pos = [], 0
        for i in p:
            doc.append((i, pos, pos + len(pieces[i])))
            pos += len(pieces[i])
        seq.append(doc)
    want = pg.pack(seq, None, cfg)
    for j, name in enumerate(("input_ids", "token_type_ids", "attention_mask", "special_tokens_mask")):
        assert want[name].tolist() == [r[j] for r in rows], name
    assert sum(len(p) > 14 for p in plain) >= 20, "rows that left truncation cuts"
    table = Table()
    return {"specials": spec, "config": cfg, "n_docs": len(docs), "row_length": len(rows[0][0]), "ids": unpadded(rows, pad), "types": [table.add(r[1]) for r in rows],
            "attention": [table.add(r[2]) for r in rows], "special": [table.add(r[3]) for r in rows], "table": table.rows}


def generate():
    os.environ["TOKENIZERS_PARALLELISM"] = "false"
    import tokenizers

    stats = {"halved_n1_above_n2": 0, "only_the_longer_cut": 0, "pairs_in_error": 0, "budget_0": 0, "error_cases": 0, "definition_only": 0}
    cases = block_cases(stats)
    stats = {k: int(v) for k, v in stats.items()}
    assert stats["halved_n1_above_n2"] >= 20 and stats["only_the_longer_cut"] >= 20 and stats["pairs_in_error"] >= 10 and stats["budget_0"] >= 2, stats
    assert 0 < stats["definition_only"] <= 0.05 * len(cases), (stats, len(cases))
    table = compact(cases)
    docs = ng.load()["docs"]
    out = {"about": "tokenizers' TemplateProcessing + enable_truncation + enable_padding: cases over a WordLevel vocabulary (word i is w<i>, documents are "
                    "words joined by single spaces), the BERT pipeline over tokenizer_wordpiece_vocab.json and the byte-level BPE pipeline over "
                    "tokenizer_bpe_vocab.json with RoBERTa's template, both over the documents of normalize_cases.json; masks and type ids are indices "
                    "into a table of digit rows; make_pack_golden.py's docstring has the layout",
           "versions": {"tokenizers": tokenizers.__version__}, "sensitivity": stats, "table": table, "templates": {k: {"single": v[0], "pair": v[1]} for k, v in TEMPLATES.items()},
           "defaults": {k: v for k, v in pg.DEFAULTS.items() if k not in ("single", "pair")}, "cases": cases, "bert": block_bert(docs),
           "roberta": block_roberta(docs[:N_ROBERTA_DOCS])}
    blob = (json.dumps(out, ensure_ascii=False, separators=(",", ":")) + "\n").encode()
    assert len(blob) < MAX_FILE, len(blob)
    return {"pack_cases.json": blob}, {"cases": len(cases), **stats, "file_bytes": len(blob)}


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
