"""The thermo state (m3g_thermo_state_bytes) and every device input of m3g_thermo_sample on buffers of exactly their size between guard
bands (tests/guarded.py), once with 0x00 and once with 0xFF inside, over the batch of tests/thermo_cases.py in both modes: the bands
intact after the init and after the eleven samples, and every output the same bits under both fills -- nothing is read that nobody
wrote."""
import ctypes as C

import numpy as np
import pytest
import torch

import thermo_cases as tc
from guarded import Arena

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILLS = (0x00, 0xFF)


def _run(monkeypatch, fill, **kw):
    import test_gpu_thermo as t
    from torch_m3gnet import _lib, thermo

    arena = Arena(DEV)
    taken = []

    def state_tensor(state_bytes, *sizes, device):
        nbytes = C.c_size_t()
        _lib.check(state_bytes(*sizes, C.byref(nbytes)))   # as _driver.state_tensor asks
        taken.append(nbytes.value)
        return arena.take(nbytes.value, fill, "thermo state")

    real_init = thermo.ThermoState.__init__

    def checked_init(self, *args, **kwargs):
        real_init(self, *args, **kwargs)
        torch.cuda.synchronize()
        arena.check()   # after the init: tables uploaded, accumulators cleared

    with monkeypatch.context() as mp:
        mp.setattr(thermo, "state_tensor", state_tensor)
        mp.setattr(thermo.ThermoState, "__init__", checked_init)
        out = t._accumulate(take=lambda x: arena.take_copy(x, "input"), **kw)
    torch.cuda.synchronize()
    arena.check()
    assert len(taken) == 1 and taken[0] > 0 and out["state_bytes"] == taken[0]
    return out, taken[0]


@pytest.mark.parametrize("mode", ["a", "b"])
def test_thermo_state_and_inputs_on_exact_size_buffers(monkeypatch, mode):
    import test_gpu_thermo as t

    kw = dict(mode=mode, remove_com=mode == "a")
    (zeros, size), (ones, _) = (_run(monkeypatch, fill, **kw) for fill in FILLS)
    print(f"thermo state of the batch, mode ({mode}): {size} B, bands intact after init and eleven samples under both fills")
    for s in range(len(tc.SIZES)):
        t._same(zeros[s], ones[s])   # (depends on what the state held before init, if it fails)
        assert np.isfinite(zeros[s]["mean"]).all() and np.isfinite(zeros[s]["comoments"]).all() and np.isfinite(zeros[s]["lag_uu"]).all()
        assert zeros[s]["n_samples"] + zeros[s]["n_skipped"] == tc.N_FRAMES
