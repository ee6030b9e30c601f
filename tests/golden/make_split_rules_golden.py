"""Writes tests/golden/split_rules_cases.json: documents with the word boundaries (byte offsets, [0, .., len]) of the cl100k_base and
Llama-3 pre-tokenizer patterns as the `regex` module matches them, and for Llama-3 also as `tokenizers`' Split(Regex(pattern),
"isolated") cuts them; the two must agree or nothing is written.  (`tokenizers` reads cl100k's `{1,3}+` as a repeated interval, not as a
possessive one, so that pattern is anchored to `regex` alone.)  Run by hand where both libraries are installed, not by a test:

    python tests/golden/make_split_rules_golden.py
"""
import json
import os
import random
import sys

import regex
import tokenizers

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]
from test_split_rules_host import CHARS, CL100K_PATTERN, LLAMA3_PATTERN, byte_bounds, random_text  # noqa: E402

HAND = [
    "", " ", "\n", "a", "1", "'", "it's WE'LL  a\n'D !'s 123abc", "I'M he'S they'Re we'vE x'T", "x'ſ y'K 'ſ", "''s 's's",
    " 's", "\t's", "\n's", "!'s", "1's", "a 'll", "a  'll", "'l", "'r", "'re", "'rex", "'sx", "x'sx", "x'llx", "x'l'l",
    "1", "12", "123", "1234", "12345", "123456", "1234567", "1281", "1٣23٣", "٣٣٣٣", "a1234b12", "12 345 6789", "1.234.56789",
    "a!\n\n b", "a\n\n b", "a \n  b", "a  \n\n  ", "a   ", "   ", " \n", "\n ", "\r\n", "\r\n\r\n", "!\r\n\r\nx", "! \n", "!\n \n",
    "a\n", "a\n\n", "a \n", "a\n ", "a \n ", "\n\na", "  \n  \n  a", "  \n  \n  ", " \n\u0085", "a  b", "a  ",
    "\tab-cd", "\nab", " ab", "!ab", "!!ab", " !ab", "  !ab", "a !", "a  !", "a\t!", "a\n!", "a!\nb", "a!\n1", "a!\n!", "a!\n \n",
    "é中ſ٣K", "中1中", " 中", "\u0085中", "K's", "'K", "ſ's", "'sſ",
    "1" * 1500, ("1" * 7 + "a") * 60, " " * 1200 + "a", " " * 1200, " " * 700 + "\n" + " " * 700, "!" + "\n" * 1100 + " x", "a" + "\n" * 1100,
]


def main():
    pats = {"cl100k": regex.compile(CL100K_PATTERN), "llama3": regex.compile(LLAMA3_PATTERN)}
    pre = tokenizers.pre_tokenizers.Split(tokenizers.Regex(LLAMA3_PATTERN), "isolated")
    rng = random.Random(20261019)
    texts = list(HAND)
    texts += [random_text(rng, 16) for _ in range(250)]
    texts += [random_text(rng, 60) for _ in range(60)]
    texts += [random_text(rng, 10) + rng.choice(" \n\t\r") * rng.randrange(1, 5) for _ in range(40)]
    cases = []
    for s in texts:
        case = {"text": s}
        for name, pat in pats.items():
            pieces = [m.group() for m in pat.finditer(s)]
            assert "".join(pieces) == s, (name, s)
            case[name] = byte_bounds(pieces)
        pieces = [p for p, _ in pre.pre_tokenize_str(s)]
        assert "".join(pieces) == s, s
        case["llama3_tokenizers"] = byte_bounds(pieces)
        assert case["llama3_tokenizers"] == case["llama3"], s
        cases.append(case)
    doc = {"regex": regex.__version__, "tokenizers": tokenizers.__version__, "alphabet": "".join(sorted(set(CHARS))), "cases": cases}
    path = os.path.join(HERE, "split_rules_cases.json")
    with open(path, "w", encoding="utf-8") as fh:
        json.dump(doc, fh, ensure_ascii=True, separators=(",", ":"))
        fh.write("\n")
    print(path, len(cases), "cases", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
