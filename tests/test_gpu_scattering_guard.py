"""The scattering state (m3g_sq_state_bytes) and every device input of m3g_sq_sample on buffers of exactly their size between guard
bands (tests/guarded.py), once with 0x00 and once with 0xFF inside, over the batch of tests/scattering_cases.py: the bands intact
after the init and after five samples, and every output the same bits under both fills -- nothing is read that nobody wrote."""
import ctypes as C

import numpy as np
import pytest
import torch

import scattering_cases as sc
from guarded import Arena

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILLS = (0x00, 0xFF)


def _run(monkeypatch, fill):
    import test_gpu_scattering as t
    from torch_m3gnet import _lib, scattering

    arena = Arena(DEV)
    taken = []

    def state_tensor(state_bytes, *sizes, device):
        nbytes = C.c_size_t()
        _lib.check(state_bytes(*sizes, C.byref(nbytes)))   # as _driver.state_tensor asks
        taken.append(nbytes.value)
        return arena.take(nbytes.value, fill, "scattering state")

    real_init = scattering.SqState.__init__

    def checked_init(self, *args, **kwargs):
        real_init(self, *args, **kwargs)
        torch.cuda.synchronize()
        arena.check()   # after the init: tables uploaded, accumulators cleared

    with monkeypatch.context() as mp:
        mp.setattr(scattering, "state_tensor", state_tensor)
        mp.setattr(scattering.SqState, "__init__", checked_init)
        out = t._accumulate(5, frames=(0, 3), take=lambda x: arena.take_copy(x, "input"))
    torch.cuda.synchronize()
    arena.check()
    assert len(taken) == 1 and taken[0] > 0
    return out, taken[0]


def test_scattering_state_and_inputs_on_exact_size_buffers(monkeypatch):
    (zeros, size), (ones, _) = (_run(monkeypatch, fill) for fill in FILLS)
    print(f"scattering state of the batch: {size} B, bands intact after init and five samples under both fills")
    for s in range(len(sc.SIZES)):
        assert sorted(zeros[s]) == sorted(ones[s])
        for key, want in zeros[s].items():
            pairs = zip(want, ones[s][key]) if isinstance(want, tuple) else [(want, ones[s][key])]
            for a, b in pairs:
                a, b = np.asarray(a), np.asarray(b)
                assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (s, key, fill_note())
        assert np.isfinite(zeros[s]["f"]).all() and list(zeros[s]["lag_count"]) == [5, 4, 3, 2]


def fill_note():
    return "depends on what the state held before init"
