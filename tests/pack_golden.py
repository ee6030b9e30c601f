"""The pure-Python definition of daac_tokens_pack (include/daachorse_amd.h): a token result wrapped in a template, truncated and padded
into the planes a model reads — `tokenizers`' TemplateProcessing + enable_truncation + enable_padding, with the deliberate differences
the header names — and the readers of tests/golden/pack_cases.json.  tests/golden/make_pack_golden.py asserts on every case of the
fixture that pack() here equals `tokenizers`.

A sequence is a list of documents, a document a list of tokens (id, start, end).  A configuration is a dict:
    single, pair   templates: lists of [kind, id, type_id] with kind "special", "A" or "B"; pair None: there is none
    max_length     None: no truncation
    strategy       "longest_first" | "only_first" | "only_second";  truncation_side "right" | "left"
    padding        "longest" | an int (fixed) | None (the CSR form);  pad_to_multiple_of None | int;  padding_side "right" | "left"
    pad_id, pad_type_id
"""
import functools
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MAX_PIECES = 16
DEFAULTS = {"single": [["A", 0, 0]], "pair": None, "max_length": None, "strategy": "longest_first", "truncation_side": "right", "padding": "longest",
            "pad_to_multiple_of": None, "padding_side": "right", "pad_id": 0, "pad_type_id": 0}


class PackError(ValueError):
    """status 1; .doc: the first document in error, or None for a configuration that is refused before any document is looked at"""

    def __init__(self, msg, doc=None):
        super().__init__(msg if doc is None else f"document {doc}: {msg}")
        self.doc = doc


def config(**kw):
    assert set(kw) <= set(DEFAULTS), kw
    return {**DEFAULTS, **kw}


def check_config(cfg, pair):
    """the refusals that need no document, in the header's order -> the template in use and its n_added"""
    for name, is_pair in (("single", False), ("pair", True)):
        t = cfg[name]
        if t is None and is_pair:
            if pair:
                raise PackError("a pair batch without a pair template")
            continue
        kinds = [p[0] for p in t]
        if len(t) > MAX_PIECES or any(k not in ("special", "A", "B") for k in kinds):
            raise PackError(f"the {name} template: at most {MAX_PIECES} pieces of kind special, A or B")
        if kinds.count("A") != 1 or kinds.count("B") != (1 if is_pair else 0):
            raise PackError(f"the {name} template holds A exactly once and B {'exactly once' if is_pair else 'never'}")
    if cfg["padding"] is not None and cfg["pad_to_multiple_of"] == 0:
        raise PackError("pad_to_multiple_of is 0")
    if cfg["max_length"] is not None and cfg["strategy"] == "only_second" and not pair:
        raise PackError("only_second without B")
    template = cfg["pair"] if pair else cfg["single"]
    n_added = sum(p[0] == "special" for p in template)
    if cfg["max_length"] is not None and cfg["max_length"] < n_added:
        raise PackError("max_length is below the template's special tokens")
    return template, n_added


def truncate(n1, n2, pair, budget, strategy):
    """-> (kept of A, kept of B), or None where only_first / only_second cannot take `need` tokens from their sequence"""
    if budget == 0:
        return 0, 0
    if not pair:
        return min(n1, budget), 0
    if n1 + n2 <= budget:
        return n1, n2
    need = n1 + n2 - budget
    if strategy == "longest_first":
        a, b = min(n1, n2), max(n1, n2)
        b = a if a > budget else max(a, budget - a)
        if a + b > budget:
            a = budget // 2
            b = a + budget % 2
        return (b, a) if n1 > n2 else (a, b)
    if strategy == "only_first":
        return (n1 - need, n2) if n1 - need > 0 else None
    return (n1, n2 - need) if n2 - need > 0 else None


def rows(a, b, cfg):
    """-> the rows before padding: per document a list of slots (id, type_id, special, start, end)"""
    pair = b is not None
    template, n_added = check_config(cfg, pair)
    assert not pair or len(a) == len(b)
    out = []
    for d, doc_a in enumerate(a):
        doc_b = b[d] if pair else []
        keep = (len(doc_a), len(doc_b))
        if cfg["max_length"] is not None:
            keep = truncate(len(doc_a), len(doc_b), pair, cfg["max_length"] - n_added, cfg["strategy"])
            if keep is None:
                raise PackError(f"{cfg['strategy']} cannot take the tokens above max_length from a sequence this short", d)
        left = cfg["truncation_side"] == "left"
        kept = {"A": doc_a[len(doc_a) - keep[0]:] if left else doc_a[:keep[0]], "B": doc_b[len(doc_b) - keep[1]:] if left else doc_b[:keep[1]]}
        row = []
        for kind, tok, type_id in template:
            row += [(tok, type_id, 1, 0, 0)] if kind == "special" else [(i, type_id, 0, s, e) for i, s, e in kept[kind]]
        out.append(row)
    return out


def row_length(lengths, cfg):
    """L of a padded batch (0 for no document)"""
    if not lengths:
        return 0
    L = max(lengths)
    if cfg["padding"] != "longest":
        L = max(L, cfg["padding"])
    m = cfg["pad_to_multiple_of"] or 1
    return (L + m - 1) // m * m


def pack(a, b, cfg):
    """-> {plane: np.int64 array}: dense [n, L] input_ids, token_type_ids, attention_mask, special_tokens_mask and offsets [n, L, 2]
    (np.uint64); or, with padding None, the same flat [R] without attention_mask and row_offsets (np.uint64[n + 1])"""
    rs = rows(a, b, cfg)
    if cfg["padding"] is None:
        flat = [s for r in rs for s in r]
        cols = np.array(flat, dtype=np.int64).reshape(len(flat), 5)
        return {"input_ids": cols[:, 0].copy(), "token_type_ids": cols[:, 1].copy(), "special_tokens_mask": cols[:, 2].copy(),
                "offsets": cols[:, 3:].astype(np.uint64), "row_offsets": np.cumsum([0] + [len(r) for r in rs]).astype(np.uint64)}
    L = row_length([len(r) for r in rs], cfg)
    pad = (cfg["pad_id"], cfg["pad_type_id"], 1, 0, 0, 0)
    full = []
    for r in rs:
        fill = [pad] * (L - len(r))
        body = [s + (1,) for s in r]
        full.append(fill + body if cfg["padding_side"] == "left" else body + fill)
    cube = np.array(full, dtype=np.int64).reshape(len(rs), L, 6)
    return {"input_ids": cube[:, :, 0].copy(), "token_type_ids": cube[:, :, 1].copy(), "attention_mask": cube[:, :, 5].copy(),
            "special_tokens_mask": cube[:, :, 2].copy(), "offsets": cube[:, :, 3:5].astype(np.uint64)}


def packer_kwargs(cfg):
    """the configuration as the keyword arguments of daachorse_amd.Packer (dtype is the caller's)"""
    return {k: ([tuple(p) for p in v] if k in ("single", "pair") and v is not None else v) for k, v in cfg.items()}


def flatten(seq, with_spans=True):
    """a sequence -> (ids np.uint32[T], spans np.uint64[T, 2], offsets np.uint64[n + 1]), or (ids, offsets)"""
    ids = np.array([t[0] for d in seq for t in d], dtype=np.uint32)
    spans = np.array([t[1:] for d in seq for t in d], dtype=np.uint64).reshape(-1, 2)
    off = np.cumsum([0] + [len(d) for d in seq]).astype(np.uint64)
    return (ids, spans, off) if with_spans else (ids, off)


# ------------------------------------------------------------------------------------------------------------- the fixture
@functools.lru_cache(maxsize=None)
def load():
    with open(os.path.join(GOLDEN, "pack_cases.json"), encoding="utf-8") as f:
        return json.load(f)


def word(i):
    """the WordLevel vocabulary of the fixture's first block: token i is this word"""
    return f"w{i}"


def sequence(ids_per_doc):
    """the fixture's id lists -> a sequence: the documents are the words joined by single spaces, a token's span is its word's"""
    out = []
    for ids in ids_per_doc:
        doc, pos = [], 0
        for i in ids:
            n = len(word(i))
            doc.append((i, pos, pos + n))
            pos += n + 1
        out.append(doc)
    return out


def case_config(case):
    """a case of the first block -> its full configuration"""
    c = load()
    t = c["templates"][case["template"]]
    return {**c["defaults"], "single": t["single"], "pair": t["pair"], **case["config"]}


def case_sequences(case):
    """-> (a, b) as pack() takes them; b is None for a batch of singles"""
    return sequence(case["a"]), None if case["b"] is None else sequence(case["b"])


def _planes(ids, digit_rows, token_offsets, csr):
    """rows of ids, {plane: rows of digit strings} and rows of the token slots' flat offsets -> {plane: array}, as pack() returns them"""
    n = len(ids)
    offsets = []
    for r, special, flat in zip(ids, digit_rows["special_tokens_mask"], token_offsets):
        it = iter(flat)
        offsets.append([(0, 0) if c == "1" else (next(it), next(it)) for c in special])
        assert len(special) == len(r) and next(it, None) is None
    rows_ = {"input_ids": ids, **{k: [[int(c) for c in r] for r in v] for k, v in digit_rows.items()}}
    if csr:
        out = {k: np.array([x for r in v for x in r], dtype=np.int64) for k, v in rows_.items()}
        out["offsets"] = np.array([x for r in offsets for x in r], dtype=np.uint64).reshape(-1, 2)
        out["row_offsets"] = np.cumsum([0] + [len(r) for r in ids]).astype(np.uint64)
        return out
    L = len(ids[0]) if n else 0
    out = {k: np.array(v, dtype=np.int64).reshape(n, L) for k, v in rows_.items()}
    out["offsets"] = np.array(offsets, dtype=np.uint64).reshape(n, L, 2)
    return out


def case_planes(case):
    """the recorded planes of a case of the first block -> {plane: array}, as pack() returns them; None for an error case"""
    w = case.get("want")
    if w is None:
        return None
    table = load()["table"]
    digits = {"token_type_ids": [table[i] for i in w["types"]], "special_tokens_mask": [table[i] for i in w["special"]]}
    if "attention" in w:
        digits["attention_mask"] = [table[i] for i in w["attention"]]
    return _planes(w["ids"], digits, w["token_offsets"], "attention" not in w)


def pipeline_planes(block, token_offsets=None):
    """the recorded planes of the second / third block -> {plane: array [n, L]}; `token_offsets`: per row the (start, end) of its
    token slots, for the block that does not record them"""
    import wordpiece_golden as wg
    table, L, pad = block["table"], block["row_length"], block["config"]["pad_id"]
    ids = [r + [pad] * (L - len(r)) for r in block["ids"]]
    digits = {name: [table[i] for i in block[k]] for k, name in (("types", "token_type_ids"), ("attention", "attention_mask"), ("special", "special_tokens_mask"))}
    if token_offsets is None:
        token_offsets = [[tuple(x) for x in p["raw"]] if isinstance(p, dict) else wg.unpack_spans(p) for p in block["token_offsets"]]
    return _planes(ids, digits, [[x for s in r for x in s] for r in token_offsets], False)
