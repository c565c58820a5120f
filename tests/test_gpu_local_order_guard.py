"""The local-order state (m3g_lo_state_bytes) and every device input of m3g_lo_sample on buffers of exactly their size between guard
bands (tests/guarded.py), once with 0x00 and once with 0xFF inside, over the batch of tests/local_order_cases.py: the bands intact
after the init and after the five samples, and every output the same bits under both fills -- nothing is read that nobody wrote."""
import ctypes as C

import numpy as np
import pytest
import torch

import local_order_cases as lc
from guarded import Arena

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILLS = (0x00, 0xFF)


def _run(monkeypatch, fill):
    import test_gpu_local_order as t
    from torch_m3gnet import _lib, local_order

    arena = Arena(DEV)
    taken = []

    def state_tensor(state_bytes, *sizes, device):
        nbytes = C.c_size_t()
        _lib.check(state_bytes(*sizes, C.byref(nbytes)))   # as _driver.state_tensor asks
        taken.append(nbytes.value)
        return arena.take(nbytes.value, fill, "local-order state")

    real_init = local_order.LoState.__init__

    def checked_init(self, *args, **kwargs):
        real_init(self, *args, **kwargs)
        torch.cuda.synchronize()
        arena.check()   # after the init: tables uploaded, accumulators cleared

    with monkeypatch.context() as mp:
        mp.setattr(local_order, "state_tensor", state_tensor)
        mp.setattr(local_order.LoState, "__init__", checked_init)
        out = t._accumulate(lc.N_FRAMES, take=lambda x: arena.take_copy(x, "input"))
    torch.cuda.synchronize()
    arena.check()
    assert len(taken) == 1 and taken[0] > 0 and out["state_bytes"] == taken[0]
    return out, taken[0]


def test_local_order_state_and_inputs_on_exact_size_buffers(monkeypatch):
    import test_gpu_local_order as t

    (zeros, size), (ones, _) = (_run(monkeypatch, fill) for fill in FILLS)
    print(f"local-order state of the batch: {size} B, bands intact after init and five samples under both fills")
    for s in range(len(lc.SIZES)):
        t._same(zeros[s], ones[s])   # (depends on what the state held before init, if it fails)
        assert np.isfinite(zeros[s]["moments"]).all() and zeros[s]["n_samples"] + zeros[s]["n_skipped"] == lc.N_FRAMES
        assert all(np.isfinite(fr["qlm"]).all() and np.isfinite(fr["qbar"]).all() for fr in zeros[s]["frames"])
