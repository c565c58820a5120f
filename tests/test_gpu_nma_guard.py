"""The normal-mode state on a buffer of exactly the size the library asks for, between guard bands, over memory that held 0x00 and
0xFF before the init call (the seam and the arena of tests/test_gpu_guard_bands.py).  Case (c) of tests/test_gpu_nma.py has the largest
eigenvector matrices (63 x 63) and mode count per q, case (d) the most q-points, a phase table of 150 x 300 and a part-filled second
chunk; five samples over four lags wrap the ring."""
import pytest

import test_gpu_nma as t
from test_gpu_guard_bands import _driver_on_guarded_states

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("names", ["c", "d", "cd"])
def test_nma_state_on_exact_size_buffer(names, monkeypatch):
    from torch_m3gnet import normal_modes

    def run():
        batch = t.Batch(names).run(5)
        return {f"{name}.{key}": val for name in names for key, val in batch.result(name).items()}

    _driver_on_guarded_states(monkeypatch, f"nma {names}", {"normal_modes": normal_modes}, run)
