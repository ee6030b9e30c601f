"""tokens_decode (daac_tokens_decode, Decoder): the definition in pure Python, the tables of the three builders restated, and the loaders
of tests/golden/decode_cases.json, which tests/golden/make_decode_golden.py writes from `tokenizers`.  Nothing here imports the library
but library_decoder(), which builds the Decoder under test for a fixture tokenizer.

A table is (rest, first, special): two {id: bytes} mappings over the same ids and a set of ids.  A document's tokens decode to
first[k_0] + rest[k_1] + rest[k_2] + ... over its kept tokens; a token is kept unless it is special and skip_special is set, or its id
has no entry and unknown is "skip" (with "error" such a token raises DecodeError with its index)."""
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CLEANUP = ((b" .", b"."), (b" ?", b"?"), (b" !", b"!"), (b" ,", b","), (b" ' ", b"'"), (b" n't", b"n't"), (b" 'm", b"'m"), (b" do not", b" don't"), (b" 's", b"'s"),
           (b" 've", b"'ve"), (b" 're", b"'re"))
NAMES = ("bpe", "wordpiece", "unigram", "llama")


class DecodeError(Exception):
    def __init__(self, token):
        super().__init__(f"token {token} has no entry")
        self.token = token


def images(table, ids, skip_special=True, unknown="error"):
    """the image of every token of one document, b"" for a token that is not kept"""
    rest, first, special = table
    out, seen_kept = [], False
    for k, i in enumerate(ids):
        if not 0 <= i < 1 << 32 or i not in rest:
            if unknown != "skip":
                raise DecodeError(k)
            out.append(b"")
        elif skip_special and i in special:
            out.append(b"")
        else:
            out.append(rest[i] if seen_kept else first[i])
            seen_kept = True
    return out


def decode(table, ids, skip_special=True, unknown="error"):
    return b"".join(images(table, ids, skip_special, unknown))


def decode_batch(table, docs, skip_special=True, unknown="error"):
    """-> (the documents' texts, the starts of all tokens in the concatenated text with the total as the closing entry); DecodeError names
    the flat index of the lowest token without an entry"""
    texts, starts, at, flat = [], [], 0, 0
    for ids in docs:
        try:
            imgs = images(table, ids, skip_special, unknown)
        except DecodeError as e:
            raise DecodeError(flat + e.token) from None
        for img in imgs:
            starts.append(at)
            at += len(img)
        flat += len(ids)
        texts.append(b"".join(imgs))
    return texts, starts + [at]


# ---- the builders' tables, restated: {id: piece bytes} and the specials' {id: text bytes} -> a table
def _table(by_id, specials, rest_of, first_of):
    by_id = {**by_id, **specials}
    return {i: rest_of(p) for i, p in by_id.items()}, {i: first_of(p) for i, p in by_id.items()}, set(specials)


def byte_level_table(pieces, specials):
    return _table(dict(enumerate(pieces)), specials, lambda p: p, lambda p: p)


def wordpiece_table(vocab, specials, prefix=b"##", cleanup=True):
    def clean(img):
        for old, new in CLEANUP if cleanup else ():
            img = img.replace(old, new)
        return img
    return _table({i: p.encode() for p, i in vocab.items()}, specials, lambda p: clean(p[len(prefix):] if p.startswith(prefix) else b" " + p), clean)


def metaspace_table(pieces, specials, byte_fallback=False, strip_one=None, replacement="▁".encode()):
    """strip_one: the first image loses one leading space (Llama-2's Sequence decoder; the default with byte_fallback); otherwise it loses
    every replacement character (`tokenizers`' decoders.Metaspace)"""
    strip_one = byte_fallback if strip_one is None else strip_one

    def byte_of(p):
        if byte_fallback and len(p) == 6 and p.startswith(b"<0x") and p.endswith(b">"):
            try:
                return bytes([int(p[3:5].decode(), 16)])
            except ValueError:
                return None
        return None

    def rest_of(p):
        b = byte_of(p)
        return b if b is not None else p.replace(replacement, b" ")

    def first_of(p):
        if not strip_one and byte_of(p) is None:
            return p.replace(replacement, b"")
        img = rest_of(p)
        return img[1:] if img.startswith(b" ") else img

    return _table({i: p.encode() for i, p in enumerate(pieces)}, specials, rest_of, first_of)


# ---- the fixture
_cache = {}


def load():
    if "fixture" not in _cache:
        with open(os.path.join(GOLDEN, "decode_cases.json"), encoding="utf-8") as f:
            _cache["fixture"] = json.load(f)
    return _cache["fixture"]


def _vocab(name):
    with open(os.path.join(GOLDEN, f"tokenizer_{name}_vocab.json"), encoding="utf-8") as f:
        return json.load(f)


def bpe_pieces():
    return [bytes.fromhex(h) for h in _vocab("bpe")["pieces_hex"]]


def specials(name, fixture=None):
    """{id: text bytes} of a fixture tokenizer's special tokens"""
    return {i: t.encode() for t, i in (fixture or load())["tokenizers"][name]["specials"]}


def table(name, fixture=None):
    """the definition's table of one of the fixture's tokenizers (NAMES)"""
    key = ("table", name, id(fixture))
    if key not in _cache:
        f = fixture or load()
        sp = specials(name, f)
        if name == "bpe":
            t = byte_level_table(bpe_pieces(), sp)
        elif name == "wordpiece":
            t = wordpiece_table(_vocab("wordpiece")["vocab"], sp)
        elif name == "unigram":
            t = metaspace_table(_vocab("unigram")["pieces"], sp)
        else:
            t = metaspace_table(f["tokenizers"]["llama"]["pieces"], sp, byte_fallback=True)
        _cache[key] = t
    return _cache[key]


def library_decoder(name):
    """the library's Decoder for the same tokenizer, through its builders"""
    import daachorse_amd as da
    sp = da.SpecialTokens({t: i for i, t in specials(name).items()})
    if name == "bpe":
        return da.Decoder.byte_level(bpe_pieces(), special=sp)
    if name == "wordpiece":
        return da.Decoder.wordpiece(_vocab("wordpiece")["vocab"], special=sp)
    if name == "unigram":
        return da.Decoder.metaspace(_vocab("unigram")["pieces"], special=sp)
    return da.Decoder.metaspace(load()["tokenizers"]["llama"]["pieces"], byte_fallback=True, special=sp)


def cases():
    """(tokenizer name, ids, {skip_special: recorded text}, lossy) of every case"""
    return [(c["tok"], c["ids"], {True: c["text"], False: c.get("text_all", c["text"])}, bool(c.get("lossy"))) for c in load()["cases"]]


def pad_id(name):
    """the special id the dense forms of the tests pad with: the last of the tokenizer's specials"""
    return load()["tokenizers"][name]["specials"][-1][1]


def padded(docs, pad, left=False, row_length=None):
    """the documents as rows of one length (the longest + 1 by default, so that every row holds padding)"""
    L = max([len(d) for d in docs] + [0]) + 1 if row_length is None else row_length
    return [[pad] * (L - len(d)) + list(d) if left else list(d) + [pad] * (L - len(d)) for d in docs]
