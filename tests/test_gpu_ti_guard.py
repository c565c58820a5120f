"""The thermodynamic-integration state on a buffer of exactly the size the library asks for, between guard bands, over memory that held
0x00 and 0xFF before the init call (the seam and the arena of tests/test_gpu_guard_bands.py)."""
import pytest

import test_gpu_ti as t
from test_gpu_guard_bands import _driver_on_guarded_states

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("friction", [0.0, 0.02])
def test_ti_state_on_exact_size_buffer(friction, monkeypatch):
    from torch_m3gnet import free_energy

    sizes = [2, 40, 257]

    def run():
        st = t._state("smooth", friction, sizes)
        obs, _ = t._run(st, sizes, 20)   # (across the change of path at call 15)
        return dict(st.read(), obs=obs, pos=st.pos)

    _driver_on_guarded_states(monkeypatch, f"ti friction {friction}", {"free_energy": free_energy}, run)
