"""The upload's layout layer on the CPU (no GPU): daachorse_amd/csrc/upload_layout.hpp turns the builders' tables into what the kernels read
— LDS offsets, padded sizes, rank blobs, hash tables, packed records, the gates behind every *_ok flag — and hands each array to a sink.
tests/native/upload_layout_check.cpp runs it with a sink that records (element size, count, FNV-1a 64 of the bytes) of every put, in order,
and prints every field of every kernel-argument struct.  Here that program is built with the address and undefined-behaviour sanitizers
and run over the dictionaries below; its output must be tests/golden/upload_layout.txt byte for byte (recorded from the upload function
before it was split into per-engine steps), and the dictionaries together must reach every branch of the layout.

Dictionaries come from daachorse_amd/synth.py (its own counter-based generator), tests/tier_layouts.py, tests/gram_u32dir.py and the
written-out LCG below.  To record the golden anew after a deliberate change of a layout: python tests/test_upload_layout_host.py"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from daachorse_amd import synth   # noqa: E402
import gram_u32dir as gu          # noqa: E402
import tier_layouts as tl         # noqa: E402

CSRC = os.path.join(ROOT, "daachorse_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "upload_layout.txt")
UNITS = ["pma.cpp", "repack.cpp", "gram.cpp", "gram2.cpp", "gram4.cpp", "gram2w.cpp", "pfx.cpp", "builder.cpp", "charwise.cpp", "charwise_builder.cpp"]
STANDARD, LEFTMOST_LONGEST, LEFTMOST_FIRST = 0, 1, 2


class Lcg:
    """x <- x * 6364136223846793005 + 1442695040888963407 mod 2^64 (Knuth's MMIX constants); a draw is the state's upper 32 bits"""
    def __init__(self, seed):
        self.x = seed & 0xFFFFFFFFFFFFFFFF

    def below(self, n):
        self.x = (self.x * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        return ((self.x >> 32) * n) >> 32


def words(seed, n, alphabet, lo, hi):
    """n distinct words of lo .. hi letters of `alphabet`, in generation order"""
    rng, seen = Lcg(seed), {}
    while len(seen) < n:
        seen.setdefault(bytes(alphabet[rng.below(len(alphabet))] for _ in range(lo + rng.below(hi - lo + 1))))
    return list(seen)


def chars(code_points):
    return ["".join(map(chr, cp)).encode("utf-8") for cp in code_points]


LOWER = b"abcdefghijklmnopqrstuvwxyz"
SCATTERED = gu.SCATTERED[:20]
CJK = 0x4E00


def _dictionaries():
    """name -> (b | c, match kind, patterns, options of the upload other than the defaults)"""
    w200 = words(1, 200, LOWER, 4, 12)
    d = {}
    # ---- bytewise, Standard
    d["words"] = ("b", STANDARD, synth.patterns_cfg3(2000), {})                          # K = 3, short patterns, find3, filter + perfect hash
    d["len1"] = ("b", STANDARD, w200 + [b"bcd", b"ab", b"a"], {})                        # a one-byte pattern
    d["no_short"] = ("b", STANDARD, w200, {})                                            # nothing of K bytes or fewer
    d["scattered"] = ("b", STANDARD, words(2, 300, SCATTERED, 2, 9), {})                 # byte classes by table, not by arithmetic
    d["long20"] = ("b", STANDARD, w200 + [b"abcdefghijklmnopqrst"], {})                  # a pattern beyond find3's 19 bytes
    d["copies17"] = ("b", STANDARD, w200[:100] + [w200[7]] * 16 + w200[100:], {})        # 16 further copies: more than EXPAND's extras hold
    d["dup4"] = ("b", STANDARD, w200 + [b"wxyz", b"wxyz"], {})                           # a depth-4 state with two patterns: K = 2
    d["alpha29"] = ("b", STANDARD, words(3, 3000, LOWER + b"012", 1, 7), {})             # 30 classes: no room for rfull, CID / H or the filter
    d["alpha29_rank"] = ("b", STANDARD, words(3, 3000, LOWER + b"012", 1, 7), {"gram4_mph": 0})   # ... records by rank: the directory leaves the filter no room
    d["short_only"] = ("b", STANDARD, words(6, 150, LOWER, 1, 3), {})                    # no depth-4 state: nothing to hash or to filter
    d["u32dir"] = ("b", STANDARD, gu.dictionary("big20").words, {})                      # 70 000 depth-4 states: 32-bit directory
    d["edge_lo"] = ("b", STANDARD, gu.dictionary("edge_lo").words, {})                   # 65 535: the largest 16-bit directory, too small for the hash
    d["wide"] = ("b", STANDARD, synth.patterns_cfg3_wide(2000), {})                      # 60 pattern bytes: wide GRAM, no TIERED
    d["binary"] = ("b", STANDARD, synth.patterns_binary256(3000), {})                    # all 256 byte values: PFX and its emitter
    d["binary_dup"] = ("b", STANDARD, synth.patterns_binary256(3000) + synth.patterns_binary256(1), {})   # ... a pattern twice: PFX without
    d["tier_w"] = ("b", STANDARD, tl.w_patterns("W"), {})                                # 32 classes: TIERED (16-bit rows) and nothing of GRAM
    d["tier_rows32"] = ("b", STANDARD, tl.w_patterns("W"), {"lds_budget": tl.BIG_BUDGET, "dense_depth": 3})
    d["rank_hbm"] = ("b", STANDARD, w200, {"gram_rank_in_lds": 0})
    d["rank_lds"] = ("b", STANDARD, w200, {"gram_rank_in_lds": 1})
    # ---- bytewise, leftmost
    d["left_shadow"] = ("b", LEFTMOST_LONGEST, w200 + [b"ab", b"a"], {})
    d["left_first"] = ("b", LEFTMOST_FIRST, w200 + [b"ab", b"a"], {})
    d["left_long"] = ("b", LEFTMOST_LONGEST, w200 + [b"abcdefghijklmnopqrst"], {})       # 20 bytes: no shadow
    d["left_alpha30"] = ("b", LEFTMOST_LONGEST, words(4, 400, LOWER + b"0123", 2, 8), {})  # 30 distinct bytes: no shadow
    d["left_empty"] = ("b", LEFTMOST_LONGEST, w200 + [b""], {})                          # "" in the set
    # ---- charwise
    d["char_ascii"] = ("c", STANDARD, w200, {})                                          # mapper and ROOT's row in LDS
    d["char_left"] = ("c", LEFTMOST_LONGEST, synth.patterns_cfg5(2000), {})
    rng = Lcg(5)
    d["char_spread"] = ("c", STANDARD, chars([0x3041 + rng.below(80) if rng.below(2) else 0x9000 + rng.below(200) for _ in range(3)] for _ in range(300)), {})
    d["char_9000"] = ("c", STANDARD, chars([CJK + i] for i in range(9000)), {})          # the mapper fits, ROOT's row beside it does not
    d["char_65536"] = ("c", STANDARD, chars([CJK + i // 256, CJK + i % 256] for i in range(65536)), {})   # 8 filter bits beside 24 of output_pos
    return d


def write_patterns(path, pats):
    """u32 n | u64 offsets[n + 1] | u32 values[n] | bytes.  Values: the index times a large odd number, so that they use all 32 bits"""
    n = len(pats)
    offs = np.zeros(n + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(p) for p in pats], dtype=np.uint64)
    vals = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    with open(path, "wb") as f:
        f.write(np.uint32(n).tobytes() + offs.tobytes() + vals.tobytes() + b"".join(pats))


def build_check(outdir, flags):
    from concurrent.futures import ThreadPoolExecutor
    from daachorse_amd import _build
    hip_include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(_build._hipcc()))), "include")   # (headers only: types such as uint4)
    units = [os.path.join(CSRC, u) for u in UNITS] + [os.path.join(ROOT, "tests", "native", "upload_layout_check.cpp")]

    def compile_one(src):
        obj = os.path.join(outdir, os.path.basename(src) + ".o")
        subprocess.check_call(["g++", "-std=c++17", *flags, "-D__HIP_PLATFORM_AMD__", "-I", hip_include, "-c", src, "-o", obj])
        return obj
    with ThreadPoolExecutor(max_workers=8) as pool:
        objs = list(pool.map(compile_one, units))
    exe = os.path.join(outdir, "upload_layout_check")
    subprocess.check_call(["g++", *flags, "-o", exe] + objs)
    return exe


def run_check(exe, workdir):
    args = []
    for name, (kind, match_kind, pats, opts) in _dictionaries().items():
        path = os.path.join(workdir, name + ".pat")
        write_patterns(path, pats)
        args += [name, kind, str(match_kind), path, ",".join(f"{k}={v}" for k, v in opts.items()) or "-"]
    r = subprocess.run([exe] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and b"runtime error" not in r.stderr and b"AddressSanitizer" not in r.stderr, r.stderr.decode()[-3000:]
    return r.stdout.decode()


SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


@pytest.fixture(scope="module")
def record(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("upload_layout"))
    return run_check(build_check(d, SANITIZE), d)


def _parse(record):
    """-> {dictionary: {struct: {field: text}}}; put lines under "put" as a list"""
    out, cur = {}, None
    for line in record.splitlines():
        head, *rest = line.split(" ")
        if head == "==":
            cur = out.setdefault(rest[0], {"put": []})
        elif head == "put":
            cur["put"].append(rest)
        else:
            cur[head] = dict(kv.split("=") for kv in rest)
    return out


def test_layout_is_the_recorded_one(record):
    with open(GOLDEN) as f:
        want = f.read()
    if record != want:
        got, exp = record.splitlines(), want.splitlines()
        first = next((i for i, (a, b) in enumerate(zip(got, exp)) if a != b), min(len(got), len(exp)))
        pytest.fail(f"line {first + 1}:\n  got  {got[first] if first < len(got) else '<end>'}\n  want {exp[first] if first < len(exp) else '<end>'}")


def test_dictionaries_reach_every_branch(record):
    r = _parse(record)
    assert list(r) == list(_dictionaries())

    def seen(struct, field, when=lambda rec: True):
        return {rec[struct][field] for rec in r.values() if when(rec)}

    def flag(rec, name):
        return rec["flags"][name] == "1"
    bytewise = lambda rec: rec["da"]["hot"] != "@-"
    charwise = lambda rec: rec["chr"]["states"] != "@-"
    # charwise
    assert seen("chr", "map_in_lds", charwise) == {"0", "1"} and seen("chr", "row_in_lds", charwise) == {"0", "1"}
    assert any(rec["chr"]["map_in_lds"] == "1" and rec["chr"]["row_in_lds"] == "0" for rec in r.values())
    assert seen("chr", "fbits", charwise) == {"16", "8"} and seen("chr", "leftmost", charwise) == {"0", "1"}
    assert int(r["char_65536"]["put"][1][2]) >= 65536 and r["char_65536"]["chr"]["obits"] == "24"
    # TIERED
    tier = lambda rec: flag(rec, "tier_ok")
    assert seen("tier", "row32", tier) == {"0", "1"}
    assert any(bytewise(rec) and not tier(rec) for rec in r.values())
    # GRAM v1
    gram = lambda rec: flag(rec, "gram_ok")
    assert {flag(rec, "gram_ok") for rec in r.values() if bytewise(rec)} == {False, True}
    assert seen("gram", "has_short", gram) == {"0", "1"} and seen("gram", "rank_in_lds", gram) == {"0", "1"}
    # GRAM v2 and gram4
    g2 = lambda rec: flag(rec, "gram2_ok")
    assert {g2(rec) for rec in r.values() if bytewise(rec)} == {False, True}
    assert {flag(rec, "gram4_ok") for rec in r.values() if bytewise(rec)} == {False, True}
    for field in ("s16", "exact_ok", "rfull_ok"):
        assert seen("gram2", field, g2) == {"0", "1"}, field
    assert r["u32dir"]["gram2"]["s16"] == "0" and r["u32dir"]["gram2"]["rfull"] == "@-"
    assert seen("gram4", "arith", g2) == {"0", "1"}
    assert "0" in seen("gram4", "mph_bytes", g2) and len(seen("gram4", "mph_bytes", g2)) > 1
    assert "0" in seen("gram4", "bloom_words", g2) and len(seen("gram4", "bloom_words", g2)) > 1
    # the emitter, find3, left3
    emit = lambda rec: rec["emit"]["me"] != "@-"
    assert "3" in seen("emit", "K", emit) and seen("emit", "K", emit) - {"3"}
    assert {flag(rec, "emit3_has_len1") for rec in r.values() if emit(rec)} == {False, True}
    assert emit(r["copies17"]) and not flag(r["copies17"], "emit3_ok") and flag(r["words"], "emit3_ok")
    assert r["copies17"]["emit3_lds"] == r["no_short"]["emit3_lds"]          # (the copies alone decline it: the same tables fit without them)
    assert flag(r["words"], "find3_ok") and r["words"]["find3"]["h1"] != "@-"
    assert emit(r["long20"]) and flag(r["long20"], "emit3_ok") and not flag(r["long20"], "find3_ok") and r["long20"]["find3"]["h1"] == "@-"
    # leftmost handles
    for name in ("left_shadow", "left_first"):
        assert flag(r[name], "left3_ok") and not flag(r[name], "find3_ok") and r[name]["da"]["leftmost"] == "1"
    for name in ("left_long", "left_alpha30", "left_empty"):
        assert not flag(r[name], "left3_ok") and not flag(r[name], "gram2_ok") and r[name]["da"]["leftmost"] == "1"
    assert r["left_empty"]["da"]["root_flag"] == "1"
    # wide GRAM, PFX
    assert flag(r["wide"], "gramw_ok")
    assert flag(r["binary"], "pfx_ok") and flag(r["binary"], "pfx_emit_ok")
    assert flag(r["binary_dup"], "pfx_ok") and not flag(r["binary_dup"], "pfx_emit_ok")
    assert r["words"]["pfx"]["bloom"] == "@-" and r["words"]["flags"]["n_distinct_bytes"] == "0"   # PFX not built


if __name__ == "__main__":
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        text = run_check(build_check(tmp, ["-O2"]), tmp)
    with open(GOLDEN, "w") as f:
        f.write(text)
    print(f"{GOLDEN}: {len(text)} bytes, {len(_dictionaries())} dictionaries")
