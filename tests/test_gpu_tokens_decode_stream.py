"""daac_tokens_decode on a caller's stream that still has work queued in front (the pattern of tests/test_gpu_streams.py, as
tests/test_gpu_tokens_pack_stream.py follows it); the other GPU tests of the call are tests/test_gpu_decode.py.  A module of its own,
named so that it is collected behind test_gpu_streams.py: that module's control test wants to be the first in the process to open
streams beside the null stream, and fails when this module's two have been opened before it."""
import numpy as np
import pytest
import torch

import decode_golden as dg
from test_gpu_decode import SKIP, _seeded_table
from test_gpu_streams import _Delay, _h, _no_collection

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def delay():
    return _Delay()


@pytest.mark.parametrize("form", ["csr", "dense"])
def test_decode_on_a_busy_callers_stream(delay, form):
    """the inputs are decoys until the copies queued behind a delay on the caller's stream have run: the call has to be ordered
    behind them with every one of its steps (the pattern of tests/test_gpu_streams.py, as tests/test_gpu_special.py follows it)"""
    dec, table = _seeded_table()
    lens = [3, 9, 0, 14, 6] * 40

    def docs(seed, lengths):
        rng = np.random.default_rng(seed)
        return [rng.integers(0, SKIP + 1, size=n).tolist() for n in lengths]

    real_docs, decoy_docs = docs(21, lens), docs(22, lens[::-1])
    if form == "dense":
        real_docs, decoy_docs = dg.padded(real_docs, SKIP, row_length=15), dg.padded(decoy_docs, SKIP, left=True, row_length=15)
    want, want_decoy = dg.decode_batch(table, real_docs), dg.decode_batch(table, decoy_docs)
    assert want[0] != want_decoy[0]

    def arrays(d):
        if form == "dense":
            return [np.array(d, dtype=np.int64)]
        return [np.array([i for x in d for i in x], dtype=np.int32), np.cumsum([0] + [len(x) for x in d]).astype(np.int64)]

    def call(tensors, **kw):
        got, starts = dec.decode_batch(tensors[0] if form == "dense" else tuple(tensors), token_starts=True, **kw)
        return got, starts.tolist()

    real, decoy = arrays(real_docs), arrays(decoy_docs)
    assert all(r.shape == d.shape and r.dtype == d.dtype for r, d in zip(real, decoy))
    warm = [torch.from_numpy(a.copy()).cuda() for a in decoy]
    assert call(warm) == want_decoy, "the decoy on the null stream"   # (and the decoder's table is on the device from here on)
    s = torch.cuda.Stream()
    dev = [torch.from_numpy(a.copy()).cuda() for a in decoy]
    src = [torch.from_numpy(a.copy()).pin_memory() for a in real]
    torch.cuda.synchronize()
    with _no_collection():
        with torch.cuda.stream(s):
            delay.queue()
            for d, r in zip(dev, src):
                d.copy_(r, non_blocking=True)
        busy = not s.query()
        got = call(dev, stream=_h(s))
    assert busy, "the delay had drained before the call was made: the run proved nothing"
    assert got == want, "the call on a stream with the caller's copies pending in front of it"
    for t, a in zip(dev, real):   # the inputs are the caller's: the real ones, unchanged
        assert np.array_equal(t.cpu().numpy(), a)
