"""The tokenizer fixtures of tests/golden/ (written by make_tokenizer_golden.py from `tokenizers` and `sentencepiece`) as the host test and
the GPU test read them, and the explicit adapters between the libraries' conventions and this library's definitions.  A plain helper:
no test lives here, and nothing here reads the three libraries."""
import functools
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BATCH_SIZES = (63, 64, 65, 256, 257)   # the wave and workgroup edges of the kernels that give a document to a lane


@functools.lru_cache(maxsize=None)
def load(name):
    with open(os.path.join(GOLDEN, f"tokenizer_{name}.json"), encoding="utf-8") as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def bpe_pieces():
    """the byte-level BPE vocabulary as bytes, in id order: id = rank"""
    return [bytes.fromhex(h) for h in load("bpe_vocab")["pieces_hex"]]


@functools.lru_cache(maxsize=None)
def bpe_words():
    """(distinct words as bytes, their ids as `tokenizers` gives them)"""
    c = load("bpe_cases")
    return [w.encode() for w in c["words"]], c["word_ids"]


@functools.lru_cache(maxsize=None)
def unigram_model():
    """-> (patterns, values, scores float32[n], unk_id, unk_score float32): every piece but the one at unk_id is a pattern whose value is
    its id; an unknown piece scores min - 10, sentencepiece's kUnkPenalty"""
    v = load("unigram_vocab")
    unk_id = v["unk_id"]
    scores = np.array(v["scores"], dtype=np.float32)
    assert scores.astype(np.float64).tolist() == v["scores"]   # the stored doubles are float32 values
    keep = [i for i in range(len(scores)) if i != unk_id]
    unk_score = np.float32(scores[keep].min()) - np.float32(10.0)
    return [v["pieces"][i].encode() for i in keep], np.array(keep, dtype=np.uint32), scores, unk_id, unk_score


def byte_alphabet():
    """byte -> its printable stand-in in GPT-2's byte-level vocabularies (encoder.py's bytes_to_unicode): the printable Latin-1 bytes
    stand for themselves, the other 68 are U+0100 onwards in byte order"""
    keep = list(range(ord("!"), ord("~") + 1)) + list(range(0xA1, 0xAD)) + list(range(0xAE, 0x100))
    rest = [b for b in range(256) if b not in keep]
    return {**{b: chr(b) for b in keep}, **{b: chr(256 + i) for i, b in enumerate(rest)}}


def sp_text(doc):
    """a document as sentencepiece's Viterbi sees it: its normalizer writes U+2581 for every space (the rest is the identity here)"""
    return doc.replace(" ", "▁").encode()


def collapse(ids, unk_id):
    """sentencepiece reports a run of unknown code points as one unk_id; this library reports one token per unknown code point"""
    ids = list(ids)
    return [v for i, v in enumerate(ids) if v != unk_id or i == 0 or ids[i - 1] != unk_id]


def permutation(n, seed=11):
    """a fixed permutation pi of 0 .. n-1 and the rank table with ranks[pi[id]] = id"""
    pi = np.random.default_rng(seed).permutation(n).astype(np.uint32)
    ranks = np.empty(n, dtype=np.uint32)
    ranks[pi] = np.arange(n, dtype=np.uint32)
    return pi, ranks
