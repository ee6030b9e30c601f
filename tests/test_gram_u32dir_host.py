"""The GRAM table sets on either side of 65 536 depth-(K+1) states, walked on the CPU (no GPU): the four check programs of tests/native —
second table set (count + checksum), `.count()` tables with filter, the perfect hash, tuple emission — over the dictionaries and texts of
tests/gram_u32dir.py.  From 65 536 states on the rank directory has 32-bit entries and no per-word companion (gram2.cpp: `s16 = n_deep <
65536`); every other dictionary of the suite stays below that.  The programs print the width they found, and it is asserted here together
with the state count the sorted prefix list gives.  The same programs, built with the address and undefined-behaviour sanitizers, run once
on the first dictionary with 32-bit entries and once on the one with the largest tables."""
import os
import subprocess

import pytest

from conftest import ROOT
import gram_u32dir as gu

CSRC = os.path.join(ROOT, "daachorse_amd", "csrc")
PROGRAMS = {"gram2_check": ["gram2.cpp"], "gram4_check": ["gram2.cpp", "gram4.cpp"], "gram4_mph_check": ["gram2.cpp", "gram4.cpp"], "emit_check": ["gram2.cpp"]}
DICTS = ["big20", "big18", "big26", "edge_lo", "edge_hi"]
# what the upload hands build_gram2_tables: gram_lds_budget (158 KiB) less the hit rings of a 1024-thread workgroup
BUDGET = 158 * 1024 - 16 * 128 * 8
HOLES_HOST = 400_000


def _build_all(outdir, flags):
    """the four programs, every translation unit compiled once and side by side"""
    from concurrent.futures import ThreadPoolExecutor
    units = {s: os.path.join(CSRC, s) for s in ("pma.cpp", "repack.cpp", "gram2.cpp", "gram4.cpp")}
    units.update({name + ".cpp": os.path.join(ROOT, "tests", "native", name + ".cpp") for name in PROGRAMS})

    def compile_one(item):
        subprocess.check_call(["g++", "-std=c++17", *flags, "-c", item[1], "-o", os.path.join(outdir, item[0] + ".o")])
    with ThreadPoolExecutor(max_workers=8) as pool:
        list(pool.map(compile_one, units.items()))
    exes = {}
    for name, needs in PROGRAMS.items():
        exes[name] = os.path.join(outdir, name)
        subprocess.check_call(["g++", *flags, "-o", exes[name]] + [os.path.join(outdir, u + ".o") for u in [name + ".cpp", "pma.cpp", "repack.cpp"] + needs])
    return exes


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    return _build_all(str(tmp_path_factory.mktemp("native")), ["-O2"])


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """name -> (blob file, {text: file}), written when first asked for"""
    d = tmp_path_factory.mktemp("u32dir")
    made = {}

    def get(name):
        if name not in made:
            dic = gu.dictionary(name)
            blob = d / (name + ".blob")
            blob.write_bytes(dic.blob())
            texts = {}
            for kind, n in (("soup", None), ("high", None), ("holes", HOLES_HOST)):
                texts[kind] = d / f"{name}.{kind}.bin"
                dic.text(kind, n).tofile(texts[kind])
            made[name] = (str(blob), {k: str(v) for k, v in texts.items()})
        return made[name]
    return get


def _fields(out):
    return dict(kv.split("=") for kv in out.split() if "=" in kv)


@pytest.mark.parametrize("name", list(gu.SPECS))
def test_dictionaries_lie_where_they_should(name):
    """the conditions on the inputs, from the sorted prefix list alone: the state count, the edge pair one word apart, enough hits of `soup` and
    `high` on prefixes of rank >= 65 536, the scattered dictionary in the order of the plain one"""
    d = gu.dictionary(name)
    assert d.n_deep == {"edge_lo": 65535, "edge_hi": 65536}.get(name, 70000)
    assert all(1 <= len(w) <= 8 for w in d.words) and sum(len(w) < 4 for w in d.words) == 38
    assert len({b for w in d.words for b in w}) == d.letters   # C = letters + 1 classes
    for kind in ("soup", "high"):
        text = d.text(kind)
        assert len(text) == gu.SOUP_BYTES
        hits, above = d.deep_hits(text)
        print(name, kind, "hits", hits, "on rank >= 65536:", above)
        assert hits > 30000
        if name.startswith("big"):
            assert above >= 1000, (name, kind, above)
        else:
            assert above == 0
    if name.startswith("big"):
        assert d.deep_hits(d.text("high"))[1] > 30000 and len(d.high_words) == 70000 - 65536
    else:   # the last 1 000 prefixes: ranks a u16 entry holds, but only just
        assert len(d.high_words) == 1000
    assert len(d.text("holes")) == gu.HOLES_BYTES and d.deep_hits(d.text("holes"))[0] > 1000
    if name == "edge_lo":
        hi = gu.dictionary("edge_hi")
        gone = set(hi.words) - set(d.words)
        assert len(gone) == 1 and set(d.words) < set(hi.words) and next(iter(gone))[:4] == max(w[:4] for w in hi.words if len(w) >= 4)
    if name == "big20s":
        plain = gu.dictionary("big20")
        table = bytes.maketrans(gu.LETTERS[:20], gu.SCATTERED[:20])
        assert [w.translate(table) for w in plain.words] == d.words and sorted(d.words) == [w.translate(table) for w in sorted(plain.words)]
        assert max(d.alphabet) - min(d.alphabet) > 29   # no arithmetic class map


@pytest.mark.parametrize("name", DICTS)
@pytest.mark.parametrize("program", list(PROGRAMS))
def test_tables_reproduce_the_automaton(programs, files, program, name):
    """the table walk of every consumer == the literal automaton walk, on soup, high and holes; the directory width is the one the state count calls for"""
    blob, texts = files(name)
    d = gu.dictionary(name)
    want = f"s16=1 n_deep=65535" if name == "edge_lo" else f"s16=0 n_deep={d.n_deep}"
    for kind, path in texts.items():
        out = subprocess.check_output([programs[program], blob, str(BUDGET), path]).decode()
        print(name, kind, out.strip())
        # (the perfect hash may be declined — big18's is: the handle then fetches by rank; everything else must be served in full)
        ok = ("OK ", "DECLINED ") if program == "gram4_mph_check" else ("OK ",)
        assert out.startswith(ok), (name, kind, out)
        assert want in out and " K=3 " in out and f" C={d.letters + 1} " in out, (name, kind, out)
        if program == "gram4_check":
            assert "arith=1 lo=97" in out and int(_fields(out)["hits"]) == d.deep_hits(d.text(kind, HOLES_HOST if kind == "holes" else None))[0], out


def test_which_dictionary_gets_which_front_table(programs, files):
    """what the GPU tests rely on: big20, big26 and edge_hi get the perfect hash; big18 does not (FILT + rank without an option), nor does edge_lo,
    whose displacement table would have to fit the 4 640 bytes of a u16 directory; every one of them gets the filter in the room the upload
    leaves it (gram4_filter_room beside the front table, less its margin of 512 bytes)"""
    for name, hashed in (("big20", True), ("big18", False), ("big26", True), ("edge_lo", False), ("edge_hi", True)):
        blob, texts = files(name)
        d = gu.dictionary(name)
        out = subprocess.check_output([programs["gram4_mph_check"], blob, str(BUDGET), texts["high"]]).decode()
        assert out.startswith("OK " if hashed else "DECLINED "), (name, out)
        f = _fields(out)
        m_bytes = ((d.letters + 1) ** 3 + 3) // 4 * 16
        front = int(f["buckets"]) if hashed else int(f["s_bytes"])
        assert int(f["s_bytes"]) == (m_bytes // 16 * (2 if name == "edge_lo" else 4) + 15) // 16 * 16
        # 16 waves at 32 positions per lane: hit lists + text slots, then [front table | Bloom array] and M
        room = (160 * 1024 - (16 * 256 * 2 + 16 * (64 * 32 + 32) + front + m_bytes)) // 16 * 16
        out = subprocess.check_output([programs["gram4_check"], blob, str(BUDGET), texts["high"], str(room - 512)]).decode()
        print(name, "front", front, "room", room, out.strip())
        assert out.startswith("OK ") and "filter=1" in out, (name, out)


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    return _build_all(str(tmp_path_factory.mktemp("native_san")), ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])


@pytest.mark.parametrize("name", ["edge_hi", "big26"])
@pytest.mark.parametrize("program", list(PROGRAMS))
def test_table_builders_under_the_sanitizers(sanitized, files, program, name):
    """the stand-alone check programs with -fsanitize=address,undefined: building and walking tables with a 32-bit directory touches nothing
    out of bounds"""
    blob, texts = files(name)
    r = subprocess.run([sanitized[program], blob, str(BUDGET), texts["high"]], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and r.stdout.decode().startswith("OK ") and "s16=0" in r.stdout.decode(), (r.stdout.decode(), r.stderr.decode()[-2000:])
    assert b"runtime error" not in r.stderr and b"AddressSanitizer" not in r.stderr, r.stderr.decode()[-2000:]
