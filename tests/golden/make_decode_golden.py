#!/usr/bin/env python3
"""Writes tests/golden/decode_cases.json (data only): what `tokenizers`' decoders make of id lists, for four tokenizers.

    python tests/golden/make_decode_golden.py            # writes the file
    python tests/golden/make_decode_golden.py --check    # regenerates in memory and compares with the committed bytes

Needs `tokenizers`, no GPU and nothing of the library: from this repository it takes the pure-Python definition tests/decode_golden.py,
the committed vocabularies and the documents and ids of the existing case files.

The tokenizers ("tokenizers": per name its special tokens as [text, id]):
    bpe        tokenizer_bpe_vocab.json with decoders.ByteLevel and the specials of special_tokens_cases.json
    wordpiece  tokenizer_wordpiece_vocab.json with decoders.WordPiece(cleanup=True), BertProcessing and that file's specials
    unigram    tokenizer_unigram_vocab.json with decoders.Metaspace and <s>, </s> behind the vocabulary
    llama      a small hand-written Llama-2-style vocabulary ("pieces") with 256 <0xHH> pieces and the decoder
               Sequence([Replace("▁", " "), ByteFallback(), Fuse(), Strip(" ", 1, 0)])

"cases": {"tok", "ids", "text", "text_all"?, "lossy"?}: text = tok.decode(ids, skip_special_tokens=True), text_all the same with False
(left out where it equals text).  The id lists are the ids `tokenizers` (sentencepiece for unigram) produced on documents of the
existing case files, and hand-made lists: specials at the start, in the middle and at the end, only specials, a ## piece first, the
cleanup triggers as separate tokens, ▁-only pieces, the empty list.  A case whose recorded text is not the UTF-8 reading of the
definition's bytes is "lossy": `tokenizers` has turned ill-formed UTF-8 into U+FFFD where the definition keeps the bytes (a lone
continuation byte, a truncated three-byte sequence; added on purpose).  Asserted here: every other case equals the definition exactly,
for both values of skip_special_tokens; a lossy text holds a U+FFFD and equals the definition's bytes read with replacement characters
once both are stripped of them; there are at least 60 cases, of which at least 2 and at most 10 % are lossy.

"bert_pipeline": BertNormalizer + BertPreTokenizer + WordPiece with [CLS] A [SEP], max_length 16 and padding to the longest row over
the documents of normalize_cases.json: "text"[d] = tok.decode(row d's ids, skip_special_tokens=True), and "specials"."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))   # tests/: decode_golden, normalize_golden, wordpiece_golden

import decode_golden as dg  # noqa: E402
import make_tokenizer_golden as base  # noqa: E402
import normalize_golden as ng  # noqa: E402
import wordpiece_golden as wg  # noqa: E402

MAX_FILE = 64 * 1024
DOCS_PER_FILE = 8      # documents of a case file that become cases: the first non-empty ones of at most MAX_IDS ids
MAX_IDS = 24
LLAMA_WORDS = ["▁", "▁▁", "▁hello", "▁wor", "ld", "▁the", "s", "a", "▁a", "é", "▁€", ".", ",", "▁x▁y", "lo▁"]


def _json(name):
    with open(os.path.join(HERE, name), encoding="utf-8") as f:
        return json.load(f)


def _add_specials(tok, spec):
    from tokenizers import AddedToken
    tok.add_special_tokens([AddedToken(t, special=True) for t, _ in spec])
    assert [tok.token_to_id(t) for t, _ in spec] == [i for _, i in spec], spec


def make_bpe():
    from tokenizers import Tokenizer, decoders, models, pre_tokenizers
    v = _json("tokenizer_bpe_vocab.json")
    mapped = ["".join(base.B2U[b] for b in bytes.fromhex(h)) for h in v["pieces_hex"]]
    tok = Tokenizer(models.BPE(vocab={m: i for i, m in enumerate(mapped)}, merges=[(mapped[a], mapped[b]) for a, b in v["merges"]]))
    tok.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False, use_regex=True)
    tok.decoder = decoders.ByteLevel()
    spec = _json("special_tokens_cases.json")["bpe_specials"]
    _add_specials(tok, spec)
    return tok, spec


def make_wordpiece(spec=None, pipeline=False):
    from tokenizers import Tokenizer, decoders, models, normalizers, pre_tokenizers, processors
    v = wg.load("vocab")
    tok = Tokenizer(models.WordPiece(vocab=v["vocab"], unk_token="[UNK]", max_input_chars_per_word=v["max_input_chars_per_word"], continuing_subword_prefix=v["prefix"]))
    if pipeline:
        tok.normalizer = normalizers.BertNormalizer()
    tok.pre_tokenizer = pre_tokenizers.BertPreTokenizer()
    tok.decoder = decoders.WordPiece(prefix=v["prefix"], cleanup=True)
    spec = spec or _json("special_tokens_cases.json")["wordpiece_specials"]
    _add_specials(tok, spec)
    ids = dict(spec)
    tok.post_processor = processors.BertProcessing(("[SEP]", ids["[SEP]"]), ("[CLS]", ids["[CLS]"]))
    return tok, spec


def make_unigram():
    from tokenizers import Tokenizer, decoders, models
    v = _json("tokenizer_unigram_vocab.json")
    tok = Tokenizer(models.Unigram([(p, float(s)) for p, s in zip(v["pieces"], v["scores"])], unk_id=v["unk_id"], byte_fallback=False))
    tok.decoder = decoders.Metaspace()
    spec = [["<s>", len(v["pieces"])], ["</s>", len(v["pieces"]) + 1]]
    _add_specials(tok, spec)
    return tok, spec


def llama_pieces():
    return ["<unk>", "<s>", "</s>"] + ["<0x%02X>" % b for b in range(256)] + LLAMA_WORDS


def make_llama():
    from tokenizers import Tokenizer, decoders, models
    pieces = llama_pieces()
    tok = Tokenizer(models.BPE(vocab={p: i for i, p in enumerate(pieces)}, merges=[], unk_token="<unk>", byte_fallback=True))
    tok.decoder = decoders.Sequence([decoders.Replace("▁", " "), decoders.ByteFallback(), decoders.Fuse(), decoders.Strip(" ", 1, 0)])
    spec = [["<unk>", 0], ["<s>", 1], ["</s>", 2]]
    _add_specials(tok, spec)
    return tok, spec


def from_files(id_lists):
    out = []
    for ids in id_lists:
        if 0 < len(ids) <= MAX_IDS:
            out.append(list(ids))
        if len(out) == DOCS_PER_FILE:
            break
    assert len(out) == DOCS_PER_FILE
    return out


def around_specials(body, sp):
    """specials at the start, in the middle and at the end, only specials, and the empty list"""
    a, b = sp[0], sp[-1]
    return [[a] + body, body[:2] + [b] + body[2:], body + [b], [a] + body[:1] + [a, b] + body[1:] + [b], [a, b, a], [a], []]


def id_lists():
    """{name: the id lists of its cases}"""
    bpe, wp, uni, st = _json("tokenizer_bpe_cases.json"), _json("tokenizer_wordpiece_cases.json"), _json("tokenizer_unigram_cases.json"), _json("special_tokens_cases.json")
    pieces = dg.bpe_pieces()
    bp = lambda b: pieces.index(b)
    out = {"bpe": from_files(bpe["ids"]) + from_files(st["bpe_ids"][:40]) + around_specials(bpe["ids"][1][:5], [1587, 1591, 1592]) +
                  [[bp(b"\x80")], [bp(b"a"), bp(b"\xe2"), bp(b"\x82")],            # lossy: a lone continuation byte, a truncated sequence
                   [bp(b"\xe2"), bp(b"\x82"), bp(b"\xac")]]}                      # the whole sequence from three tokens
    v = wg.load("vocab")["vocab"]
    w = lambda *ps: [v[p] for p in ps]
    cont = sorted(p for p in v if p.startswith("##") and len(p) > 2)[:3]
    out["wordpiece"] = from_files(wp["ids"]) + from_files(st["wordpiece_ids"][:40]) + around_specials(wp["ids"][0][:5], [1079, 1080, 1084]) + [
        w(cont[0], "a"), w(cont[1], cont[2]), w("a", cont[0], ",", "a", "'", "s"),
        w("a", ".", "a", "?", "a", "!", "a", ",", "a", "'", "a"), w("a", "'", "s", "a", "'", "m"), w(".", "a"), w("'", "a"),
        [v[p] for p in ("do", "not", "'s", "'ve", "'re", "n't", "'m") if p in v] + w("a")]
    pc = _json("tokenizer_unigram_vocab.json")["pieces"]
    u = lambda *ps: [pc.index(p) for p in ps]
    out["unigram"] = from_files(uni["ids"]) + from_files(uni["tie_ids"]) + around_specials(uni["ids"][0][:5], [853, 854]) + [
        u("▁"), u("▁", "▁"), u("▁", "▁the", "▁"), u("▁the"), u("'", "▁the"), [0, 15, 0]]
    lp = llama_pieces()
    q = lambda *ps: [lp.index(p) for p in ps]
    out["llama"] = around_specials(q("▁hello", "▁wor", "ld", "▁", "."), [1, 2]) + [
        q("▁hello", "▁wor", "ld", "▁"), q("▁"), q("▁", "▁"), q("▁▁"), q("▁▁", "a"), q("▁x▁y", "▁x▁y"), q("lo▁", "lo▁"), q("<0x20>", "a"), q("<0x20>", "<0x20>"),
        q("a", "<0xE2>", "<0x82>", "<0xAC>", "s"), q("▁€", "é", "<0xC3>", "<0xA9>"), q("<0x00>", "<0x7F>", "<0x0A>"), q("<unk>", "a"),
        q("<0xE2>", "<0x82>"), q("<0x80>", "a")]   # lossy
    return out


def generate():
    os.environ["TOKENIZERS_PARALLELISM"] = "false"
    import tokenizers

    made = {"bpe": make_bpe(), "wordpiece": make_wordpiece(), "unigram": make_unigram(), "llama": make_llama()}
    fixture = {"tokenizers": {name: {"specials": spec} for name, (_, spec) in made.items()}}
    fixture["tokenizers"]["llama"]["pieces"] = llama_pieces()
    cases, n_lossy = [], 0
    for name, lists in id_lists().items():
        tok = made[name][0]
        table = dg.table(name, fixture)
        for ids in lists:
            text = {b: tok.decode(ids, skip_special_tokens=b) for b in (True, False)}
            mine = {b: dg.decode(table, ids, skip_special=b) for b in (True, False)}
            case = {"tok": name, "ids": ids, "text": text[True]}
            if text[False] != text[True]:
                case["text_all"] = text[False]
            lossy = any(mine[b] != text[b].encode() for b in (True, False))
            if lossy:
                for b in (True, False):
                    assert "�" in text[b] and text[b].replace("�", "") == mine[b].decode("utf-8", "replace").replace("�", ""), (name, ids, text, mine)
                case["lossy"] = True
                n_lossy += 1
            cases.append(case)
    assert len(cases) >= 60 and 2 <= n_lossy <= 0.10 * len(cases), (len(cases), n_lossy)
    # the BERT pipeline over the documents of normalize_cases.json
    spec = [["[CLS]", 1079], ["[SEP]", 1080], ["[PAD]", 1081]]
    tok, _ = make_wordpiece(spec, pipeline=True)
    tok.enable_truncation(16)
    tok.enable_padding(pad_id=1081, pad_token="[PAD]")
    docs = ng.load()["docs"]
    encs = tok.encode_batch(docs)
    texts = [tok.decode(e.ids, skip_special_tokens=True) for e in encs]
    fx = {"tokenizers": {"wordpiece": {"specials": spec}}}
    for e, t in zip(encs, texts):
        assert dg.decode(dg.table("wordpiece", fx), e.ids) == t.encode()
    out = {"about": "tokenizers' decode(ids, skip_special_tokens) for four tokenizers over the committed vocabularies and a hand-written Llama-2-style one; "
                    "make_decode_golden.py's docstring has the layout",
           "versions": {"tokenizers": tokenizers.__version__}, "sensitivity": {"cases": len(cases), "lossy": n_lossy, "with_text_all": sum("text_all" in c for c in cases)},
           **fixture, "cases": cases, "bert_pipeline": {"specials": spec, "max_length": 16, "row_length": len(encs[0].ids), "text": texts}}
    blob = (json.dumps(out, ensure_ascii=False, separators=(",", ":")) + "\n").encode()
    assert len(blob) < MAX_FILE, len(blob)
    return {"decode_cases.json": blob}, {**out["sensitivity"], "file_bytes": len(blob)}


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
