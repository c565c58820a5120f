"""The collective-variable bias state on a buffer of exactly the size the library asks for, between guard bands, over memory that
held 0x00 and 0xFF before the init call (the seam and the arena of tests/test_gpu_guard_bands.py).  Two COORDINATION CVs with a hill
list small enough to fill is the largest per-atom footprint the family has (both gradient regions written, every hill slot written,
the FULL flag set); one DISTANCE CV with one hill the smallest.  The batch of 2, 7, 257, 600 and 600 atoms holds a part-filled
chunk and a one-row one."""
import pytest

import test_gpu_meta as t
from test_gpu_guard_bands import _driver_on_guarded_states

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kinds,max_hills,calls", [(("coordination", "coordination"), 4, 6), (("distance",), 2, 2)], ids=["two-coordination-fills", "distance-one-hill"])
def test_meta_state_on_exact_size_buffer(kinds, max_hills, calls, monkeypatch):
    from torch_m3gnet import metadynamics

    def run():
        batch = t.Batch(kinds, max_hills=max_hills, inv_kdt=8.0)
        for c in range(calls):
            batch.device(deposit=(c > 0))
        out = batch.result()
        if max_hills == 4:
            assert out["flags"].tolist() == [2] * 5 and out["n_hills"].tolist() == [4, 4, 4, 4]
        else:
            assert out["flags"].tolist() == [0] * 5 and out["n_hills"].tolist() == [1, 1, 1, 2]
        rows = batch.membership != 0     # (the gradient rows of atoms in no group are never written, nor read)
        return dict(out, gradients=batch.state.gradients.cpu().numpy()[rows] if "coordination" in kinds else out["obs"])

    _driver_on_guarded_states(monkeypatch, f"meta {'-'.join(kinds)} max_hills {max_hills}", {"metadynamics": metadynamics}, run)
