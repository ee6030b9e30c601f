"""The waiting set of gram4's filter body (gram4_kernels.hip, FILT process_batch / survivors_ask) at the fill levels where its fill, wrap and flush can
go wrong: what passes the probe of a batch of 64 hits joins the lanes [sb_n, sb_n + s), the set is asked for when 64 are together, what went beyond
lane 63 wraps to lanes 0 .. and waits on, and the end of a scan flushes what is left.

A small dictionary with few depth-4 states makes texts of known hits: tests/native/gram4_survivors_check.cpp builds the Bloom array as the upload does
and says for every hit of a text whether g4f_probe lets it pass, so every constructed text is first checked on the CPU to have the pass counts it was
made for.  With one region (gram_region >= the text) one wave scans the text and its batches are the text's hits in order, 64 at a time.  Every text is
counted by the FILT body with records by hash and by rank, at 32 and 16 positions per lane, and compared with the oracle's count."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

import daachorse_amd as da
from daachorse_amd import Engine, ScanMode, synth

LETTERS = b"abcdefghijklmnopqrstuvwxyz"
ONE_REGION = 1 << 20


def _small_words():
    """about 200 words of 4 to 8 letters on 28 stems of four letters: 10 stems are words themselves (their hits END a pattern and always pass), the
    other 18 are not and have five or six of the 26 letters as children (most other next bytes fail the probe)"""
    rng = np.random.default_rng(12)
    al = np.frombuffer(LETTERS, dtype=np.uint8)
    stems = []
    while len(stems) < 28:
        s = bytes(al[rng.permutation(26)[:4]])   # four different letters: a stem does not overlap itself
        if s not in stems:
            stems.append(s)
    words = set(stems[:10])
    for s in stems:
        for c in rng.permutation(26)[:int(rng.integers(5, 7))]:
            w = s + LETTERS[c:c + 1]
            words.add(w)
            if rng.random() < 0.3:
                words.add(w + bytes(al[rng.integers(0, 26, size=int(rng.integers(1, 4)))]))
    return sorted(words), stems[:10], stems[10:]


class _Dict:
    def __init__(self, pats, exe, tmp):
        self.pats, self.exe, self.tmp = pats, exe, tmp
        self.oracle = orc.OraclePma.build(pats)
        self.blob = os.path.join(tmp, "d%d.blob" % len(pats))
        with open(self.blob, "wb") as f:
            f.write(self.oracle.serialize())
        self.handles = {}
        for how, mph in (("hash", 8), ("rank", 0)):
            p, _ = da.DoubleArrayAhoCorasick.deserialize(self.oracle.serialize())
            p.set_option("gram4_mph", mph)   # (read when the tables are laid out)
            info = p.upload().info()
            assert info.gram2_available and info.gram2_k == 3, info.gram2_k
            self.handles[how] = p
        self._n = 0

    def hits(self, text, how):
        """(positions, passed) of the text's hits in order, by the CPU walk with g4f_probe against the Bloom array of the `how` handle"""
        self._n += 1
        h, o = os.path.join(self.tmp, "h%d.bin" % self._n), os.path.join(self.tmp, "o%d.bin" % self._n)
        np.asarray(text, dtype=np.uint8).tofile(h)
        out = subprocess.check_output([self.exe, self.blob, h, "1" if how == "hash" else "0", o]).decode()
        assert out.startswith("OK K=3 "), out
        v = np.fromfile(o, dtype=np.uint32)
        os.remove(h)
        os.remove(o)
        return (v & 0x7fffffff).astype(np.int64), (v >> 31).astype(bool)

    def check(self, text, what, region=ONE_REGION, ppls=(32, 16), hows=("hash", "rank")):
        """the FILT body's count of `text` with records by hash and by rank, at 32 and 16 positions per lane, against the oracle's"""
        import torch
        text = np.ascontiguousarray(text, dtype=np.uint8)
        want = self.oracle.overlapping_count(text, threads=4)[0]
        dev = torch.from_numpy(text).cuda()
        for how in hows:
            p = self.handles[how]
            for ppl in ppls:
                for k, v in {"gram_version": 4, "gram_ppl": ppl, "gram3_tail": 0, "gram2_rfull": 1, "threads": 1024, "gram4_arith": 1, "gram4_filter": 1,
                             "gram_region": region, "gram_slab": 4096}.items():
                    p.set_option(k, v)
                got = p.count(ScanMode.FindOverlapping, dev, engine=Engine.Gram)
                lk = da.last_kernel()
                assert da.last_engine() == int(Engine.Gram) and lk.startswith("gram4 "), lk
                f = dict(kv.split("=") for kv in lk.split()[1:])
                assert (f["ppl"], f["filter"], f["mph"], f["tail"]) == (str(ppl), "1", "1" if how == "hash" else "0", "0"), (what, how, ppl, lk)
                assert got == want, (what, how, ppl, region, lk, got, want)


@pytest.fixture(scope="module")
def probe_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("native") / "gram4_survivors_check")
    csrc = os.path.join(ROOT, "daachorse_amd", "csrc")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "native", "gram4_survivors_check.cpp"),
                           os.path.join(csrc, "pma.cpp"), os.path.join(csrc, "repack.cpp"), os.path.join(csrc, "gram2.cpp"), os.path.join(csrc, "gram4.cpp")])
    return exe


class _Small(_Dict):
    """the small dictionary and its units — a stem, one more byte and a space: six bytes with exactly one hit whatever stands around them (a 4-gram
    with a space in it is no hit), which passes the probe (`yes`) or does not (`no`) with both Bloom arrays"""

    def __init__(self, exe, tmp):
        pats, ending, open_stems = _small_words()
        super().__init__(pats, exe, tmp)
        assert 150 <= len(pats) <= 260, len(pats)
        cands = [s + bytes([y]) + b" " for s in ending + open_stems for y in LETTERS + b" "]
        text = np.frombuffer(b"".join(cands), dtype=np.uint8)
        ok = np.ones(len(cands), dtype=bool)   # the unit's only hit is its stem's
        passes = []
        for how in ("hash", "rank"):
            pos, passed = self.hits(text, how)
            per = np.bincount(pos // 6, minlength=len(cands))
            flag = np.zeros(len(cands), dtype=bool)
            flag[pos // 6] = passed
            ok &= (per == 1) & np.isin(np.arange(len(cands)) * 6 + 3, pos)
            passes.append(flag)
        same = ok & (passes[0] == passes[1])
        self.yes = [c for c, s, f in zip(cands, same, passes[0]) if s and f]
        self.no = [c for c, s, f in zip(cands, same, passes[0]) if s and not f]
        assert len(self.yes) >= 50 and len(self.no) >= 50, (len(self.yes), len(self.no))

    def text_of(self, batches, rng, pad_to=None):
        """64 units per entry of `batches`, of which that many pass, at random places of the batch; space up to `pad_to` bytes"""
        units = []
        for s in batches:
            flags = np.zeros(64, dtype=bool)
            flags[rng.permutation(64)[:s]] = True
            units += [(self.yes if f else self.no)[int(rng.integers(0, len(self.yes if f else self.no)))] for f in flags]
        t = b"".join(units)
        if pad_to is not None:
            assert len(t) <= pad_to
            t += b" " * (pad_to - len(t))
        return np.frombuffer(t, dtype=np.uint8)

    def pass_counts(self, text, group=64, by_region=None):
        """per batch of 64 hits in text order (or per region of `by_region` bytes): how many pass — the same with both Bloom arrays, or it fails"""
        res = []
        for how in ("hash", "rank"):
            pos, passed = self.hits(text, how)
            if by_region:
                res.append((np.bincount(pos // by_region, minlength=len(text) // by_region).tolist(),
                            np.bincount(pos // by_region, weights=passed, minlength=len(text) // by_region).astype(int).tolist()))
            else:
                pad = (-len(passed)) % group
                res.append(([group] * (len(passed) // group) + ([len(passed) % group] if pad else []),
                            np.concatenate([passed, np.zeros(pad, dtype=bool)]).reshape(-1, group).sum(axis=1).tolist()))
        assert res[0] == res[1]
        return res[0]


_small = {}


@pytest.fixture
def small(probe_exe, tmp_path_factory):
    if "d" not in _small:
        _small["d"] = _Small(probe_exe, str(tmp_path_factory.mktemp("small")))
    return _small["d"]


def test_a_every_hit_passes(small):
    """(a) a 5-byte dictionary prefix over and over: every batch has s = 64, the one case where the failing lanes' target lies inside the arrivals —
    and more hits in a step than a wave's hit list holds"""
    for prefix in sorted(set(w[:5] for w in small.pats if len(w) >= 6)):   # (one whose other four 4-grams are no hits)
        text = np.frombuffer(prefix * ((64 << 10) // 5), dtype=np.uint8)
        hits, passes = small.pass_counts(text)
        if sum(hits) == len(text) // 5:
            break
    assert sum(hits) == len(text) // 5 and hits[:-1] == passes[:-1] == [64] * (len(hits) - 1) and hits[-1] == passes[-1], (hits[:4], passes[:4])
    small.check(text, "a")
    small.check(text, "a, 2 KiB regions", region=2048)


def test_b_no_hit_passes(small):
    """(b) depth-4 states followed by a byte that is no child and that the Bloom word rejects: the waiting set stays empty to the end"""
    rng = np.random.default_rng(3)
    text = small.text_of([0] * 171, rng)
    assert len(text) >= 64 << 10
    hits, passes = small.pass_counts(text)
    assert hits == [64] * 171 and passes == [0] * 171, passes
    small.check(text, "b")


def test_c_fill_to_exactly_64_and_to_65(small):
    """(c) the first batches carry 1, 31, 32 and 63 survivors: 1 + 31 + 32 brings the set to exactly 64 (nothing wraps), 63 + 2 to 65 (one lane wraps),
    then a full batch onto a waiting one, empty batches in between, 63 + 64 and 63 + 1, and random fills"""
    rng = np.random.default_rng(4)
    batches = [1, 31, 32, 63, 2, 64, 0, 62, 64, 1, 63, 0, 1, 0, 63, 1, 64, 64, 0, 33, 31, 32, 32, 1] + rng.integers(0, 65, size=150).tolist()
    text = small.text_of(batches, rng)
    assert len(text) >= 64 << 10
    hits, passes = small.pass_counts(text)
    assert hits == [64] * len(batches) and passes == batches, passes[:24]
    small.check(text, "c")


@pytest.mark.parametrize("left", [1, 63])
def test_d_last_flush(small, left):
    """(d) survivors_ask(sb_n) at the end of a scan with 1 and with 63 waiting: regions of 2 KiB, one per wave, each with 64 k + 1 (64 k + 63) survivors,
    so that every wave ends on such a flush; and the same text as one region, where the one wave's last flush has as many"""
    rng = np.random.default_rng(5 + left)
    regions, per_region = [], []
    for r in range(64):
        # 5 batches of 64 units of 6 bytes in 2 048; the last region brings the text's total to 64 k + left as well
        b = [int(rng.integers(0, 65)) for _ in range(4)]
        want_mod = left if r < 63 else (left - sum(per_region)) % 64
        b.append((want_mod - sum(b)) % 64)
        per_region.append(sum(b))
        regions.append(small.text_of(b, rng, pad_to=2048))
    text = np.concatenate(regions)
    assert len(text) == 128 << 10 and sum(per_region) % 64 == left
    hits, passes = small.pass_counts(text, by_region=2048)
    assert hits == [320] * 64 and passes == per_region and all(p % 64 == left for p in passes[:-1]), passes
    small.check(text, "d, 2 KiB regions", region=2048)
    small.check(text, "d, one region")


_cfg3 = {}


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_e_uniform_text(small, probe_exe, tmp_path_factory, seed):
    """(e) 1 MiB of uniform text over a-z and space, cfg3's dictionary and the small one, with the library's own region size and with 2 KiB regions"""
    if "d" not in _cfg3:
        _cfg3["d"] = _Dict(synth.patterns_cfg3(), probe_exe, str(tmp_path_factory.mktemp("cfg3")))
    text = synth.uniform_haystack(1 << 20, synth.SEEDS["cfg3_hay"] + seed, synth.ALPHA_LOWER_SPACE)
    _cfg3["d"].check(text, "e cfg3", region=0)
    _cfg3["d"].check(text, "e cfg3, 2 KiB regions", region=2048, ppls=(32,))
    small.check(text, "e small", region=0, ppls=(32,))
