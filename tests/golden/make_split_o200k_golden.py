"""Writes tests/golden/split_o200k_cases.json: documents with the word boundaries (byte offsets, [0, .., len]) of tiktoken's o200k_base
pre-tokenizer pattern as the `regex` module matches them and as `tokenizers`' Split(Regex(pattern), "isolated") cuts them; the two must
agree or nothing is written.  Every code point used has had its general category since Unicode 13 (the standard library's tables may be
older than `regex`'s).  Run by hand where both libraries are installed, not by a test:

    python tests/golden/make_split_o200k_golden.py
"""
import json
import os
import random
import sys

import regex
import tokenizers

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]
from test_split_o200k_host import O200K_PATTERN, SMALL, WIDE, byte_bounds, random_text  # noqa: E402

M = "\u0301"
CONTRACTIONS = ("'s", "'t", "'re", "'ve", "'m", "'ll", "'d")
HAND = [
    # the examples of the rule's definition
    "HTMLParser", "XMLHttpRequest", "helloWorld", "a中B", "A中Bc", "AB中CD", "AB中CDe", "AB中CD中EF x",
    f"!{M}abc", f"!!{M}abc", f" !{M}abc", f"!{M * 5}abc", f"!!{M * 5}abc", f" !{M * 5}abc", f"{M}A", f"a{M}B", f"A{M}B c",
    "don't", " DON'T", " don'T", " he'll", " x'ſ", "a's't", "A'sB", "ab'sCd", "abC's", "1's", "x''s", " 's's",
    "!\n/!", "!/!", "a/\n/b",
    # camel case, acronyms, caseless scripts next to cased ones
    "", "a", "A", "aB", "Ab", "AB", "ABc", "ABcD", "aBC", "aBCd", "getHTTPResponseCode", "iPhone", "McDonald", "NASA's", "NASAs", "eBay IDs",
    "中", "中a", "中A", "a中", "A中", "中中A", "中Aa", "a中a", "A中A", "a中A中a", "A中a中A", "ab中中CD中e", "AB中中 cd", "東京Tokyo", "Tokyo東京", "TOKYO東京都",
    "ʰa", "aʰB", "AʰB", "AʰB ", "ʰ", "日本語のテキスト", "Привет Мир", "ПРИВЕТмир", "éÉ", "Éé", "ÉÉé", "éÉÉ", "straßeSTRASSE",
    # titlecase letters
    "ǅ", "ǅa", "aǅ", "ǅǅ", "ǅaǅ", "Aǅa", "aǅA", " ǅungla",
    # marks after letters, after one punctuation character, after two, after a space plus punctuation
    f"a{M}", f"A{M}", f"a{M}b", f"A{M}b", f"A{M}B", f"a{M}{M}B", f"A{M}{M}Bc", f"e{M}te{M}", f"{M}", f"{M}{M}", f"{M}a", f"{M}{M}a", f"{M}!", f"{M}1",
    f"!{M}", f"!{M}!", f"!{M}A", f"!{M}A ", f"!{M}Ab", f"!!{M}", f"!!{M}A", f"!!{M}'s", f" {M}", f" {M}a", f" {M}A", f" !{M}", f" !{M}A", f"  !{M}a",
    f"\t{M}a", f"\n{M}a", f"1{M}a", f"a!{M}b", f"a!!{M}b", f"/{M}a", f"'{M}s", f"a'{M}s", f"a{M}'s", f"!!{M}\n/a", f"!{M}\n/a", f"a{M}\n/",
    # contractions: all seven, both cases, U+017F, what may stand in front of them
    *[f"we{c}" for c in CONTRACTIONS], *[f" WE{c.upper()}" for c in CONTRACTIONS], *[f"x{c}y" for c in CONTRACTIONS], *[f"X{c.upper()}Y z" for c in CONTRACTIONS],
    "it's WE'LL  a\n'D !'s 123abc", "I'M he'S they'Re we'vE x'T", "x'ſ y'K 'ſ", "ſ's", "'sſ", "a'ſb", "''s 's's", " 's", "\t's", "\n's", "!'s", "a 'll", "a  'll",
    "'l", "'r", "'re", "'rex", "'sx", "x'sx", "x'llx", "x'l'l", "a'", "a''", "a'1", "a' s", "a'S's", "中's", "中'S中", f"a{M}'ll", "a'll'll", "a'r", "a'rE", "a'l", "a'v'e",
    # / and newlines behind punctuation
    "!/", "!\n", "!\n/", "!/\n", "!/\n/", "!\n\n//\n!", "!\n/a", "!\n/ a", "!\n/\t", "!\n /", "a/b", "a//b", "a/\nb", "/\n/", "/", "//", "\n/", " /", " /\n/", " //a",
    "http://a.b/c", "a.\n/b", "a!\r\n/\r\n/x", "1/2", "1/\n/2", "a \n/",
    # digit runs, whitespace runs with and without newlines
    "1", "12", "123", "1234", "12345", "1234567", "1٣23٣", "a1234b12", "12 345 6789", "1.234.56789", "A1b2C3",
    "a!\n\n b", "a\n\n b", "a \n  b", "a  \n\n  ", "a   ", "   ", " \n", "\n ", "\r\n", "\r\n\r\n", "!\r\n\r\nx", "! \n", "!\n \n",
    "a\n", "a \n", "a\n ", "\n\na", "  \n  \n  a", "  \n  \n  ", " \n\u0085", "a  b", "a  B", "a  ", "\tab-cd", "\nab", " ab", "!ab", "!!ab", " !ab", "  !ab", "a !", "a  !",
    "a\t!", "a\n!", "a!\nb", "a B", "a  b", " !a",
    # runs over more than a tile
    "a" + "中" * 1100 + "B", "A" + "中" * 1100 + "Bc", "A" + "中" * 1100 + "B ", "中" + "A" * 1100 + " ", "中" + "A" * 1100 + "b", "!" + M * 700 + "a", "!!" + M * 700 + "a",
    "!" + "\n" * 1100 + "/!", "1" * 1500, " " * 700 + "\n" + " " * 700 + "a",
]


def main():
    pat = regex.compile(O200K_PATTERN)
    pre = tokenizers.pre_tokenizers.Split(tokenizers.Regex(O200K_PATTERN), "isolated")
    rng = random.Random(20261019)
    texts = list(dict.fromkeys(HAND))
    texts += [random_text(rng, 16, SMALL) for _ in range(120)]
    texts += [random_text(rng, 16) for _ in range(150)]
    texts += [random_text(rng, 60) for _ in range(60)]
    texts += [random_text(rng, 10) + rng.choice(" \n\t\r/") * rng.randrange(1, 5) for _ in range(40)]
    cases = []
    for s in texts:
        pieces = [m.group() for m in pat.finditer(s)]
        assert "".join(pieces) == s, s
        case = {"text": s, "o200k": byte_bounds(pieces)}
        pieces = [p for p, _ in pre.pre_tokenize_str(s)]
        assert "".join(pieces) == s, s
        case["o200k_tokenizers"] = byte_bounds(pieces)
        assert case["o200k_tokenizers"] == case["o200k"], s
        cases.append(case)
    doc = {"regex": regex.__version__, "tokenizers": tokenizers.__version__, "alphabet": "".join(sorted(set(WIDE))), "cases": cases}
    path = os.path.join(HERE, "split_o200k_cases.json")
    with open(path, "w", encoding="utf-8") as fh:
        json.dump(doc, fh, ensure_ascii=True, separators=(",", ":"))
        fh.write("\n")
    print(path, len(cases), "cases", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
