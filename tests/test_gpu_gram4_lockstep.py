"""The lock-step pass of gram4's filter body (gram4_kernels.hip, process_pass): the full batches of 64 hits a step has queued go through list read, text
read, Bloom probe and permute together, up to two at a time at 32 positions per lane, and join the waiting set in batch order.  What a pass can get
wrong and a single batch could not: which list entries each of its batches takes (the first also the entries the step before left behind), the fill
of the waiting set each batch meets (worked out for all of them before the first has joined), two sets of 64 coming together in one pass, a pass cut
short by the end of the list, and the passes of a step with more hits than the list holds.

Built on tests/test_gpu_gram4_survivors.py: its small dictionary and six-byte units with exactly one hit that passes the probe or does not, and
tests/native/gram4_survivors_check.cpp, which says for every hit of a text whether it passes — every text here is first checked on the CPU to carry,
step by step, the hits and passes it was made for.  A text is a sequence of steps of 2 048 bytes (a wave's step at 32 positions per lane), each with
its units packed at the front and spaces behind, scanned as one region, so that one wave sees the hits in order; the FILT body counts it with records
by hash and by rank, at 32 and at 16 positions per lane (where the same bytes are twice as many steps), and the oracle's count is the expected one."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

import test_gpu_gram4_survivors as sv

STEP = 2048          # bytes of a wave's step at 32 positions per lane
LIST = 256           # entries of a wave's hit list
# hits of one step: around every multiple of the batch, up to the list's size, and beyond it (the scan of the step runs again on the rest):
# 257 leaves one entry for the second scan, 320 a full batch, 341 is what fits into a step
COUNTS = [0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 320, 341]
# the same split over consecutive steps: what the first leaves behind (fewer than 64) opens the next step's first pass
SEQUENCES = [(n,) for n in COUNTS] + [(63, 65), (1, 127), (127, 1), (63, 129, 64)]


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    """the small dictionary of test_gpu_gram4_survivors.py (shared with that module when both run)"""
    if "d" not in sv._small:
        exe = str(tmp_path_factory.mktemp("native") / "gram4_survivors_check")
        csrc = os.path.join(ROOT, "daachorse_amd", "csrc")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "native", "gram4_survivors_check.cpp"),
                               os.path.join(csrc, "pma.cpp"), os.path.join(csrc, "repack.cpp"), os.path.join(csrc, "gram2.cpp"), os.path.join(csrc, "gram4.cpp")])
        sv._small["d"] = sv._Small(exe, str(tmp_path_factory.mktemp("small")))
    return sv._small["d"]


def _flags(pattern, n, at):
    """pass / no pass of the n hits of a step whose first hit is the text's hit number `at`"""
    if pattern == "all":
        return [True] * n
    if pattern == "none":
        return [False] * n
    assert pattern == "alternating"
    return [(at + i) % 2 == 0 for i in range(n)]


def _text(small, steps, rng):
    """one step of STEP bytes per entry of `steps` (a list of pass flags, one per hit): the units at its front, spaces behind"""
    out = []
    for flags in steps:
        assert len(flags) * 6 <= STEP
        units = [(small.yes if f else small.no)[int(rng.integers(0, len(small.yes if f else small.no)))] for f in flags]
        t = b"".join(units)
        out.append(t + b" " * (STEP - len(t)))
    return np.frombuffer(b"".join(out), dtype=np.uint8)


def _checked(small, steps, rng, what):
    """the text of `steps`, after the CPU walk has found in every step exactly the hits and passes it was made for, with both Bloom arrays"""
    text = _text(small, steps, rng)
    want_hits = [len(f) for f in steps]
    want_pass = [bool(x) for f in steps for x in f]
    for how in ("hash", "rank"):
        pos, passed = small.hits(text, how)
        assert np.bincount(pos // STEP, minlength=len(steps)).tolist() == want_hits, (what, how, "hits per step")
        assert passed.tolist() == want_pass, (what, how, "passes")
    return text


def _steps(pattern, seq, waiting=None):
    """the steps of a case: `seq` hits per step with `pattern`; `waiting`: a step of 64 hits in front of which that many pass, so that the passes
    of `seq` meet a waiting set of that size"""
    steps, at = [], 0
    if waiting is not None:
        steps.append([i < waiting for i in range(64)])
    for n in seq:
        steps.append(_flags(pattern, n, at))
        at += n
    return steps


@pytest.mark.parametrize("pattern", ["all", "none", "alternating"])
def test_hits_per_step(small, pattern):
    """every count and every split over steps, with every hit passing, none, and every other one"""
    rng = np.random.default_rng(131 + len(pattern))
    for seq in SEQUENCES:
        what = "%s %s" % (pattern, seq)
        small.check(_checked(small, _steps(pattern, seq), rng, what), what)


@pytest.mark.parametrize("waiting", [1, 63])
def test_waiting_set_in_front_of_full_passes(small, waiting):
    """1 and 63 survivors wait when passes come whose batches pass entirely: every batch brings 64 together and wraps — two sets of 64 in one
    pass, the second consuming the first's records before it asks —, with 63 waiting all but one lane wrap"""
    rng = np.random.default_rng(137 + waiting)
    for seq in SEQUENCES:
        what = "%d waiting, all pass %s" % (waiting, seq)
        small.check(_checked(small, _steps("all", seq, waiting=waiting), rng, what), what)


@pytest.mark.parametrize("pattern", ["all", "alternating"])
def test_scan_ends_and_regions(small, pattern):
    """a scan that ends with an odd number of full batches and a partial one (the last pass is cut to one batch, the rest and the waiting survivors
    go out by the flush at the end of the scan), alone and behind a step that leaves entries; then all of this file's sequences in one text, as one
    region and with regions of one and of two steps, whose ends fall inside it (a wave's state goes on from one of its regions to the next)"""
    rng = np.random.default_rng(139 + len(pattern))
    for seq in [(3 * 64 + 17,), (64 + 5,), (40, 3 * 64 - 40 + 17), (5 * 64 + 1,)]:
        what = "scan end %s %s" % (pattern, seq)
        small.check(_checked(small, _steps(pattern, seq), rng, what), what)
    steps = []
    for seq in SEQUENCES:
        steps += _steps(pattern, seq)
    what = "all sequences, %s" % pattern
    text = _checked(small, steps, rng, what)
    assert len(text) <= 1 << 20
    small.check(text, what)
    small.check(text, what + ", 2 KiB regions", region=STEP)
    small.check(text, what + ", 4 KiB regions", region=2 * STEP)
