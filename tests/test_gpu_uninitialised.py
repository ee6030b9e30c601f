"""What a call may assume of the memory it is given: nothing.  Scratch and result buffers come from the device's
stream-ordered pool, which returns a freed block as the last call left it, from a handle's kept workspace, which lives from call to
call, and from plain hipMalloc, whose memory is zero only by habit.  Option debug_fill sets every byte those sources hand out to a chosen
byte first; every case of tests/uninit_cases.py — every device entry point of the header, on the routes the header and DESIGN.md name —
must return exactly the CPU reference's result with the fill off, 0x00, 0xFF and 0xA5, with the kept workspace and without it
(workspace_keep = 0: the pool serves the emitter and find3 too), and name the same route (daac_last_kernel) under every fill.

Three more tests: caller-owned result buffers prefilled with 0xA5; twelve different calls on one set of handles in two seeded orders
with the fill off, which leaves the structured leftovers of real calls in the pool and the workspace; and, in
tests/test_uninit_ledger_host.py (no GPU), the ledger: every entry point of the header is host-only or driven by a case.

The module runs on the null stream except for the result_dev case, and sorts behind test_gpu_streams.py on purpose."""
import numpy as np
import pytest
import torch

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

import daachorse_amd as da
from daachorse_amd import Engine, ScanMode

import uninit_cases as uc

FILLS = (-1, 0x00, 0xFF, 0xA5)
KEEP_DEFAULT = 8 << 30
OV = ScanMode.FindOverlapping


@pytest.fixture(scope="module")
def world():
    try:
        yield uc.World()
    finally:   # whatever happened
        da.set_option("debug_fill", -1)
        da.set_option("workspace_keep", KEEP_DEFAULT)


@pytest.fixture(autouse=True)
def _restore():
    yield
    da.set_option("debug_fill", -1)
    da.set_option("workspace_keep", KEEP_DEFAULT)


_wants = {}


def _want(world, name):
    if name not in _wants:
        _wants[name] = uc.CASES[name].want(world)
    return _wants[name]


def _run(c, world):
    """the case's call; a device error ends the session: after a fault nothing more is started on the device"""
    try:
        return c.run(world)
    except da.DaachorseError as e:
        if e.code == 7:   # DAAC_ERR_DEVICE: a HIP error
            pytest.exit(f"{c.name}: the device reported an error ({e}); nothing more is run on it", returncode=3)
        raise


def _differs(got, want):
    """where two plain results part, for the assertion's message"""
    if type(got) is not type(want):
        return f"{type(got).__name__} / {type(want).__name__}"
    if isinstance(got, dict):
        return {k: _differs(got.get(k), want.get(k)) for k in sorted(set(got) | set(want)) if got.get(k) != want.get(k)}
    if isinstance(got, (list, tuple)):
        if len(got) != len(want):
            return f"{len(got)} / {len(want)} entries"
        for i, (g, x) in enumerate(zip(got, want)):
            if g != x:
                return {i: _differs(g, x)}
    return f"{str(got)[:120]} / {str(want)[:120]}"


@pytest.mark.parametrize("name", sorted(uc.CASES))
def test_every_call_under_every_fill(world, name):
    c = uc.CASES[name]
    want = _want(world, name)
    for keep in (KEEP_DEFAULT, 0):
        da.set_option("workspace_keep", keep)
        labels = {}
        for fill in FILLS:
            da.set_option("debug_fill", fill)
            got = _run(c, world)
            labels[fill] = got.pop() if name.startswith("gram-") else da.last_kernel()   # (those cases make two calls and return the first's label)
            assert got == want, (name, f"debug_fill={fill} workspace_keep={keep}", labels[fill], _differs(got, want))
        assert len(set(labels.values())) == 1, (name, keep, labels)


# --------------------------------------------------------------------------------------------------------- caller-owned outputs
def _a5(n):
    t = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda").repeat_interleave(8).view(torch.int64)
    assert t.numel() == n and int(t[0].item()) & 0xFF == 0xA5
    return t


def _u64(t):
    return t.cpu().numpy().view(np.uint64).tolist()


@pytest.mark.parametrize("fill", FILLS)
def test_caller_owned_outputs_prefilled_with_a5(world, fill):
    """result_dev of the count calls ({count, S1, S2}; daac_scan_count_only_range: word 0 alone has a meaning), out= of histogram and
    out=(counts, checksums) of scan_count_batch: every word the header calls meaningful is exact whatever the buffer held"""
    da.set_option("debug_fill", fill)
    o, p = world.gram()
    uc._set(p, {})
    m = world.tuples("soup", uc.SMALL)
    cs = orc.matches_checksum(m)
    stream = torch.cuda.Stream()
    for engine in (Engine.Auto, Engine.DArray):   # gram4 / the v1 kernels; the segment scanners
        for hay in (world.dev("soup", uc.SMALL), world.dev("soup", uc.SMALL)[:0]):
            n, want_cs = (len(m), cs) if hay.numel() else (0, 0)
            res = _a5(3)
            torch.cuda.synchronize()
            assert p.count(OV, hay, engine=engine, result_dev=res.data_ptr(), stream=stream.cuda_stream) is None
            stream.synchronize()
            assert _u64(res)[0] == n, (engine, hay.numel(), _u64(res))
            res = _a5(3)
            torch.cuda.synchronize()
            assert p.scan_count(OV, hay, engine=engine, result_dev=res.data_ptr(), stream=stream.cuda_stream) is None
            stream.synchronize()
            r = _u64(res)
            assert r[0] == n and (((r[1] & 0xffffffff) << 32) | (r[2] & 0xffffffff)) == want_cs, (engine, hay.numel(), r)
    # a find_iter count through find3 and through the chain walkers
    fm = world.tuples("uniform", uc.SMALL, "find_iter")
    for find3 in (2, 0):
        p.set_option("find3", find3)
        res = _a5(3)
        torch.cuda.synchronize()
        assert p.scan_count(ScanMode.Find, world.dev("uniform", uc.SMALL), result_dev=res.data_ptr()) is None
        torch.cuda.synchronize()
        r = _u64(res)
        assert r[0] == len(fm) and (((r[1] & 0xffffffff) << 32) | (r[2] & 0xffffffff)) == orc.matches_checksum(fm), (find3, r)
    p.set_option("find3", None)
    # histogram: every slot, the patterns that never match included
    so, sp, text, dev = uc._rich_handle(world, True)
    for bins in (0, None):
        sp.set_option("hist_lds_bins", bins)
        out = _a5(world.s.slots.n)
        assert sp.histogram(OV, dev, out=out) is None
        torch.cuda.synchronize()
        assert _u64(out) == uc.ts._hist_dense(world.s, so.find_overlapping_iter(text)), bins
    # scan_count_batch: every document's two words, the empty documents' included
    host, devb = uc._batch_input(world, "scan_count_batch-standard-Find", 64), uc._batch_dev(world, "scan_count_batch-standard-Find", 64)
    docs = uc.ts._split(*host)
    for mode, api, pma, orac in ((OV, "find_overlapping_iter", world.s.p, world.s.o), (ScanMode.Find, "find_iter", world.s.p, world.s.o),
                                 (ScanMode.LeftmostFind, "leftmost_find_iter", world.s.pl, world.s.ol)):
        cnt, sums = _a5(len(docs)), _a5(len(docs))
        assert pma.scan_count_batch(mode, tuple(devb), out=(cnt, sums)) is None
        torch.cuda.synchronize()
        ms = [getattr(orac, api)(d) for d in docs]
        assert _u64(cnt) == [len(x) for x in ms] and _u64(sums) == [orc.matches_checksum(x) for x in ms], mode


# ------------------------------------------------------------------------------------------------------------------ the sequence
# twelve different calls, all on the cfg3 Standard handle: the count kernels, the emitter, find3 with and without its own tuple list, the
# chain walkers, the lazy iterator and a shard worker share one kept workspace and one pool
SEQUENCE = ["emit-gram", "gram4-unclaimed-soup", "gram4-unclaimed-uniform", "gram4-shard-begin5", "scan_count-plain", "select-standard-windows-select_emit1",
            "select-standard-windows-select_emit0", "chain-standard-restart_chain1", "chain-standard-restart_chain0", "iter-next_batch", "iter-next_batch8",
            "scan_count_multi-two-shards"]


@pytest.mark.parametrize("seed", [1, 2])
def test_twelve_calls_in_two_orders(world, seed):
    """with the fill off: every call runs over what the calls in front of it left in the pool and in the handle's workspace, in two orders"""
    assert len(set(SEQUENCE)) == 12
    order = np.random.default_rng(seed).permutation(12).tolist()
    for rep in range(2):
        for i in order:
            name = SEQUENCE[i]
            got = uc.CASES[name].run(world)
            assert got == _want(world, name), (name, seed, rep, [SEQUENCE[j] for j in order], _differs(got, _want(world, name)))
