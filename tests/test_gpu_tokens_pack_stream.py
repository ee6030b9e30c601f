"""daac_tokens_pack on a caller's stream that still has work queued in front (the pattern of tests/test_gpu_streams.py, as
tests/test_gpu_special.py follows it); the other GPU tests of the call are tests/test_gpu_pack.py.  A module of its own, collected
behind test_gpu_streams.py: that module's control test wants to be the first in the process to open streams beside the null stream."""
import numpy as np
import pytest
import torch

import pack_golden as pg
from test_gpu_pack import BERT_PAIR, BERT_SINGLE, _packer, _same, _seeded
from test_gpu_streams import _Delay, _h, _no_collection

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def delay():
    return _Delay()


@pytest.mark.parametrize("padding", ["longest", None], ids=["dense", "csr"])
def test_pack_on_a_busy_callers_stream(delay, padding):
    """the inputs are decoys until the copies queued behind a delay on the caller's stream have run: the call has to be ordered
    behind them with every one of its steps (the pattern of tests/test_gpu_streams.py, as tests/test_gpu_special.py follows it)"""
    cfg = pg.config(single=BERT_SINGLE, pair=BERT_PAIR, max_length=12, padding=padding)
    p = _packer(cfg)
    la, lb = [3, 9, 0, 14, 6] * 40, [8, 2, 5, 14, 0] * 40
    real_seq, decoy_seq = (_seeded(11, la), _seeded(12, lb)), (_seeded(13, la[::-1]), _seeded(14, lb[::-1]))
    want, want_decoy = pg.pack(*real_seq, cfg), pg.pack(*decoy_seq, cfg)
    assert not np.array_equal(want["input_ids"], want_decoy["input_ids"])

    def arrays(seqs):
        return [x.view(np.int32 if x.dtype.itemsize == 4 else np.int64) for s in seqs for x in pg.flatten(s)]

    real, decoy = arrays(real_seq), arrays(decoy_seq)
    assert all(r.shape == d.shape and r.dtype == d.dtype for r, d in zip(real, decoy))
    warm = [torch.from_numpy(a.copy()).cuda() for a in decoy]
    _same(p.pack(tuple(warm[:3]), tuple(warm[3:])), want_decoy, np.int64, "the decoy on the null stream")
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
        got = p.pack(tuple(dev[:3]), tuple(dev[3:]), stream=_h(s))
    assert busy, "the delay had drained before the call was made: the run proved nothing"
    _same(got, want, np.int64, "the call on a stream with the caller's copies pending in front of it")
    for t, a in zip(dev, real):   # the inputs are the caller's: the real ones, unchanged
        assert np.array_equal(t.cpu().numpy(), a)
