"""The path-integral MD state on a buffer of exactly the size the library asks for, between guard bands, over memory that held 0x00
and 0xFF before the init call (the seam and the arena of tests/test_gpu_guard_bands.py)."""
import pytest

import test_gpu_pimd as t
from test_gpu_guard_bands import _driver_on_guarded_states

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("thermostat", ["none", "pile_l"])
def test_pimd_state_on_exact_size_buffer(thermostat, monkeypatch):
    from torch_m3gnet import path_integral

    sizes, P = [1, 40, 257], 3

    def run():
        st = t._state(thermostat, sizes, P)
        obs, _ = t._run(st, sizes, P, 10)
        return dict(st.read(), obs=obs, pos=st.pos)

    _driver_on_guarded_states(monkeypatch, f"pimd {thermostat}", {"path_integral": path_integral}, run)
