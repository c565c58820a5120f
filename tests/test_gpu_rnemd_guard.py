"""The reverse non-equilibrium MD state on a buffer of exactly the size the library asks for, between guard bands, over memory that held
0x00 and 0xFF before the init call (the seam and the arena of tests/test_gpu_guard_bands.py).  64 slabs with 8 swaps is the largest
per-chunk and per-structure footprint the family has; the batch of 7, 257 and 64 atoms holds a part-filled chunk and a one-row one."""
import pytest

import test_gpu_rnemd as t
from test_gpu_guard_bands import _driver_on_guarded_states

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", [("heat", 64, 8, False, True), ("momentum", 6, 3, True, False)], ids=lambda c: "-".join(map(str, c)))
def test_rnemd_state_on_exact_size_buffer(case, monkeypatch):
    from torch_m3gnet import dynamics, transport

    def run():
        batch = t.Batch(case).settle()
        batch.exchange(check=False)
        batch.exchange(swap=False, check=False)
        batch.exchange(sample=False, check=False)
        return dict(batch.result(), pos=batch.dyn.pos, flags=batch.dyn.read()["flags"])

    _driver_on_guarded_states(monkeypatch, f"rnemd {case[0]} {case[1]} slabs {case[2]} swaps", {"transport": transport, "dynamics": dynamics}, run)
