"""What the batched drivers (relax, dynamics, neb, phonons, elasticity) share on the host: argument checks, the model every driver
evaluates, state allocation and the split of one structure's copies into engine sub-batches.  The FIRE loop they share is
`relax.fire_loop`, beside `fire_step`; the status read after the last evaluation is `VerletGraph.raise_on_step_errors`."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .data.atomic_masses import masses_of
from .nn.modules import Gradient

EV_A3_TO_GPA = 160.21766208


def positive(name: str, x) -> float:
    x = float(x)
    if not (math.isfinite(x) and x > 0.0):
        raise ValueError(f"{name} must be a finite number > 0; got {x}")
    return x


def integer(name: str, x, least: int) -> int:
    if isinstance(x, bool) or int(x) != x or x < least:
        raise ValueError(f"{name} must be an integer >= {least}; got {x}")
    return int(x)


def boolean(name: str, x) -> bool:
    if not isinstance(x, (bool, np.bool_)):
        raise ValueError(f"{name} must be True or False; got {x!r}")
    return bool(x)


def structure_arrays(lattices, positions, atomic_numbers):
    """The structure lists every driver takes, checked: ([3,3] fp64 lattices, [n_s,3] fp64 positions, [n_s] atomic numbers)."""
    if not (len(lattices) == len(positions) == len(atomic_numbers)) or len(lattices) == 0:
        raise ValueError("lattices, positions and atomic_numbers must hold one entry per structure (at least one)")
    lat = [np.asarray(L, dtype=np.float64) for L in lattices]
    pos = [np.asarray(p, dtype=np.float64) for p in positions]
    z = [np.asarray(a).reshape(-1) for a in atomic_numbers]
    for s, (L, p, a) in enumerate(zip(lat, pos, z)):
        if L.shape != (3, 3):
            raise ValueError(f"structure {s}: lattice must be [3, 3]; got {L.shape}")
        if p.ndim != 2 or p.shape[1] != 3 or p.shape[0] != len(a) or len(a) == 0:
            raise ValueError(f"structure {s}: positions must be [n, 3] with n = len(atomic_numbers) >= 1; got {p.shape} for {len(a)} atoms")
        if not (np.isfinite(L).all() and np.isfinite(p).all()):
            raise ValueError(f"structure {s}: non-finite lattice or positions")
        if abs(np.linalg.det(L)) < 1e-12:
            raise ValueError(f"structure {s}: singular lattice")
    return lat, pos, z


def structure_masses(masses, z) -> list:
    """[n_s] fp64 masses (amu) per structure: the caller's, checked, or the standard atomic weights of `z`."""
    if masses is None:
        return [masses_of(a) for a in z]
    if len(masses) != len(z):
        raise ValueError("masses: expected one array per structure")
    m = [np.asarray(x, dtype=np.float64).reshape(-1) for x in masses]
    for s, (ms, a) in enumerate(zip(m, z)):
        if len(ms) != len(a) or not (np.isfinite(ms).all() and (ms > 0).all()):
            raise ValueError(f"structure {s}: masses must be {len(a)} finite values > 0")
    return m


def check_tensor(name: str, x: torch.Tensor, shape: tuple, dtype: torch.dtype, device=None) -> None:
    """`x` is a contiguous `dtype` tensor of `shape` (a string entry stands for any size), on `device` when one is given."""
    fits = x.dim() == len(shape) and all(isinstance(n, str) or d == n for d, n in zip(x.shape, shape))
    if x.dtype != dtype or not fits or not x.is_contiguous() or (device is not None and x.device != device):
        where = "" if device is None else f" on {device}"
        raise ValueError(f"{name} must be a contiguous [{', '.join(map(str, shape))}] {str(dtype).split('.')[-1]} tensor{where}")


def batch_layout(pos: torch.Tensor, lattice: torch.Tensor | None, offsets):
    """(offsets int64, N, S) of a state over the caller's `pos` [N,3] / `lattice` [S,3,3] (fp64, moved in place), checked."""
    check_tensor("pos", pos, ("N", 3), torch.float64)
    offsets = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64))
    n_structs = int(len(offsets) - 1)
    if n_structs < 1:
        raise ValueError("offsets must hold S + 1 >= 2 entries")
    if lattice is not None:
        check_tensor("lattice", lattice, (n_structs, 3, 3), torch.float64)
    return offsets, int(pos.size(0)), n_structs


def gpu_device(device, what: str) -> torch.device:
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError(f"{what} runs on a GPU device; got {device}")
    return torch.device("cuda", torch.cuda.current_device()) if device.index is None else device


def state_tensor(state_bytes, *sizes, device) -> torch.Tensor:
    """The uint8 tensor of a device state, of the size `state_bytes` (an m3g_*_state_bytes) gives for `sizes`."""
    nbytes = C.c_size_t()
    _lib.check(state_bytes(*sizes, C.byref(nbytes)))
    return torch.empty(nbytes.value, dtype=torch.uint8, device=device)


def sub_batches(n_copies: int, n: int, max_atoms: int):
    """(first_copy, count) of the engine sub-batches of `n_copies` copies of one structure of `n` atoms: in order, at most `max_atoms`
    atoms each (at least one copy).  The engine's rounding depends on the composition of its batch, so a structure's sub-batches hold
    its own copies only -- and its results are the same alone or in any batch."""
    per = max(1, max_atoms // n)
    for first in range(0, n_copies, per):
        yield first, min(per, n_copies - first)


class Driver:
    """The model handling of every driver.  `model`: the `Gradient` returned by `build_model`; the driver evaluates a
    `pair_virial=True` engine of its own made from its `Sequential`, at the precision of the caller's engine."""

    def __init__(self, model: Gradient, skin: float = 0.5, device="cuda"):
        if not isinstance(model, Gradient):
            raise TypeError(f"{type(self).__name__} needs the Gradient model returned by build_model")
        self.skin = positive("skin", skin)
        self.model = Gradient(model.model, pair_virial=True, legendre_backward=model.legendre_backward)
        if model._engine is not None:
            self.model.engine.set_precision(model._engine.precision)
        self.device = torch.device(device)
