"""Batched structure relaxation on the device: FIRE or L-BFGS with an optional unit-cell filter (C ABI: m3g_fire_*,
csrc/m3g_relax.hip; m3g_lbfgs_*, csrc/m3g_lbfgs.hip).

The reference relaxes through m3gnet's `Relaxer` (scripts/relax_org.py): ASE's FIRE over a UnitCellFilter, `fmax=0.1`, `steps=500`,
one optimiser per structure on the host.  `Relaxer.relax` takes a whole batch: every structure is relaxed on its own, with the
semantics of ASE's FIRE applied to that structure alone (unit masses, ASE's default parameters), and a structure that has converged
is frozen -- its positions, cell and FIRE state stay bitwise unchanged while the others go on.  Per iteration the energies, forces
and (pair-virial) stresses come from `VerletGraph.step` and the FIRE step of the whole batch is three kernel launches; with the cell
fixed the loop waits for nothing but the skin test's verdict `m3g_md_step` waits for anyway, behind which the number of structures
still relaxing (written by the previous FIRE launch) is already in host memory.  With the cell relaxed every step moves the cell,
so the candidates are searched again at every step (`VerletGraph.set_lattice`).

`Relaxer(optimizer="lbfgs")` runs ASE's LBFGS (no line search) per structure instead, with the same cell filter, verdicts, freezing
and loop: a quasi-Newton step from the newest `memory` pairs (s, y) of that structure, five launches per iteration whatever the
memory and the batch; near a minimum it needs several times fewer force evaluations than FIRE.
"""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np
import torch

from . import _cuda, _lib
from ._driver import (Driver, atom_offsets, batch_layout, check_tensor, integer, positive, read_state, state_tensor,
                      structure_arrays)
from .data import MaterialGraphKey as K
from .data.graph_gpu import _ptr, _stream
from .data.md import VerletGraph
from .nn.modules import Gradient

# ASE's FIRE defaults (ase/optimize/fire.py), as m3gnet's Relaxer uses them
FIRE_DEFAULTS = dict(dt=0.1, maxstep=0.2, dtmax=1.0, nmin=5, finc=1.1, fdec=0.5, astart=0.1, fa=0.99)
# ASE's LBFGS defaults (ase/optimize/lbfgs.py); H0 = 1 / alpha
LBFGS_DEFAULTS = dict(maxstep=0.2, memory=100, damping=1.0, alpha=70.0)


class OptimizerState:
    """What `FireState` and `LbfgsState` share: an optimiser's state of a batch on the device over the caller's tensors.  `pos`
    ([N,3] fp64) and, when `relax_cell`, `lattice` ([S,3,3] fp64) are moved IN PLACE by `step` (and `lattice32`, their fp32 copy);
    `offsets`: S + 1 atom offsets, strictly increasing.  A subclass names its parameters (`NAME`, `DEFAULTS`), its m3g_<PREFIX>_state_bytes
    / _init / _step / _read, builds its parameter struct (`_params`) and lists what `read()` returns (`_sizes`, `_fields`)."""

    def __init__(self, pos: torch.Tensor, lattice: torch.Tensor | None, offsets: Sequence[int], relax_cell: bool = True, fmax: float = 0.1,
                 **params):
        unknown = set(params) - set(self.DEFAULTS)
        if unknown:
            raise TypeError(f"unknown {self.NAME} parameters {sorted(unknown)}")
        self.params = self._params(dict(self.DEFAULTS, **params), fmax, 1 if relax_cell else 0)
        self.offsets, self.N, self.S = batch_layout(pos, lattice, offsets)
        if relax_cell and lattice is None:
            raise ValueError("a cell relaxation needs the lattice")
        self.relax_cell = bool(relax_cell)
        self.pos, self.lattice = pos, lattice
        self.lattice32 = lattice.to(torch.float32) if lattice is not None else None
        self.device = pos.device
        self.lib = _lib.load_library()
        state_bytes, init, self._step, self._read = (getattr(self.lib, f"m3g_{self.PREFIX}_{fn}") for fn in ("state_bytes", "init", "step", "read"))
        self.state = state_tensor(state_bytes, *self._sizes(), device=self.device)
        self.unconverged = torch.full((1,), self.S, dtype=torch.int32).pin_memory()   # written by every step's launch
        self._unconverged = self.unconverged.numpy()
        with _cuda.on_device(self.device):
            _lib.check(init(C.byref(self.params), self.N, self.S, self.offsets.ctypes.data, _ptr(pos), _ptr(lattice), _ptr(self.state),
                            self.state.numel(), _stream()))

    def _sizes(self) -> tuple:
        return self.N, self.S

    @property
    def n_unconverged(self) -> int:
        """Structures neither converged nor failed after the last `step` whose launch the host has waited for."""
        return int(self._unconverged[0])

    def read(self) -> dict:
        return read_state(self._read, self._sizes(), self.state, self._fields())

    def step(self, forces: torch.Tensor, stresses: torch.Tensor | None = None, check_only: bool = False) -> None:
        """One iteration of the batch at `forces` [N,3] and `stresses` [S,6] (float32, pair-virial convention: the virial is
        W = V * stresses) evaluated at `pos`: converged / failed structures are flagged and frozen, every other one takes a step.
        Queued on the current stream; no wait."""
        check_tensor("forces", forces, (self.N, 3), torch.float32)
        if stresses is not None:
            check_tensor("stresses", stresses, (self.S, 6), torch.float32)
        with _cuda.on_device(self.device):
            _lib.check(self._step(C.byref(self.params), self.N, self.S, _ptr(self.state), self.state.numel(), _ptr(forces),
                                  _ptr(stresses), _ptr(self.pos), _ptr(self.lattice) if self.relax_cell else None,
                                  _ptr(self.lattice32) if self.relax_cell else None, 1 if check_only else 0,
                                  C.c_void_p(self.unconverged.data_ptr()), _stream()))


class FireState(OptimizerState):
    """FIRE state of a batch on the device (m3g_fire_init): the generalized coordinates and velocities in fp64, the per-structure
    dt, a, n, flags and step counts.  `read()`: flags / n_steps / dt / a / n [S] and the generalized coordinates X / velocities v
    [N + 3S, 3] (atom rows, then three cell rows per structure), copied to the host (waits for the stream)."""
    NAME, PREFIX, DEFAULTS = "FIRE", "fire", FIRE_DEFAULTS

    def _params(self, p: dict, fmax, relax_cell: int):
        return _lib.M3GFireParams(dt=p["dt"], maxstep=p["maxstep"], dtmax=p["dtmax"], finc=p["finc"], fdec=p["fdec"], astart=p["astart"],
                                  fa=p["fa"], fmax=positive("fmax", fmax), nmin=int(p["nmin"]), relax_cell=relax_cell)

    def _fields(self):
        S, R = self.S, self.N + 3 * self.S
        return (("flags", np.int32, S), ("n_steps", np.int32, S), ("dt", np.float64, S), ("a", np.float64, S), ("n", np.int32, S),
                ("x", np.float64, (R, 3)), ("v", np.float64, (R, 3)))


def fire_step(state: FireState, forces: torch.Tensor, stresses: torch.Tensor | None = None, check_only: bool = False) -> None:
    """One FIRE iteration of the batch (m3g_fire_step): `OptimizerState.step`."""
    state.step(forces, stresses, check_only)


class LbfgsState(OptimizerState):
    """L-BFGS state of a batch on the device (m3g_lbfgs_init): the generalized coordinates, the previous point and gradient, the ring
    of the newest `memory` pairs (s, y) and the per-structure Gram matrices in fp64, flags, step counts and history depths.
    `read()`: flags / n_steps / n_pairs (the history depth) [S] and the generalized coordinates X [N + 3S, 3]."""
    NAME, PREFIX, DEFAULTS = "L-BFGS", "lbfgs", LBFGS_DEFAULTS

    def _params(self, p: dict, fmax, relax_cell: int):
        self.memory = integer("memory", p["memory"], 1)
        if self.memory > _lib.LBFGS_MAX_MEMORY:
            raise ValueError(f"memory must be <= {_lib.LBFGS_MAX_MEMORY}; got {self.memory}")
        return _lib.M3GLbfgsParams(maxstep=positive("maxstep", p["maxstep"]), damping=positive("damping", p["damping"]),
                                   alpha=positive("alpha", p["alpha"]), fmax=positive("fmax", fmax), memory=self.memory,
                                   relax_cell=relax_cell)

    def _sizes(self) -> tuple:
        return self.N, self.S, self.memory

    def _fields(self):
        S = self.S
        return (("flags", np.int32, S), ("n_steps", np.int32, S), ("n_pairs", np.int32, S), ("x", np.float64, (self.N + 3 * S, 3)))


def lbfgs_step(state: LbfgsState, forces: torch.Tensor, stresses: torch.Tensor | None = None, check_only: bool = False) -> None:
    """One L-BFGS iteration of the batch (m3g_lbfgs_step): `OptimizerState.step`."""
    state.step(forces, stresses, check_only)


OPTIMIZERS = {"fire": (FireState, FIRE_DEFAULTS), "lbfgs": (LbfgsState, LBFGS_DEFAULTS)}   # name -> (state class, its parameters)


def fire_loop(vg: VerletGraph, model: Gradient, fire: FireState | LbfgsState, steps: int, project=None) -> dict:
    """Up to `steps` iterations of the optimiser state `fire` (a `FireState` or an `LbfgsState`: the loop calls its `step`) over
    `vg.step(model, fire.pos)`; returns the evaluation at the final positions.
    `project(out)`: the forces the optimiser takes instead of `out`'s own (NEB).  With a relaxed cell every iteration copies the cells
    to the host and searches the candidates again (`vg.set_lattice`).  `fire.n_unconverged` is pinned memory written by the step's
    launch: it is read only behind a wait that follows that launch (the next `vg.step`'s skin test, or the lattice copy)."""
    out = None
    for k in range(steps + 1):
        out = vg.step(model, fire.pos)   # waits for the skin test, hence for the previous FIRE launch and its count
        if k > 0 and not fire.relax_cell and fire.n_unconverged == 0:
            break                        # (nothing moved at that launch: `out` holds the final positions' results)
        forces, stresses = (out[K.FORCES], out[K.STRESSES]) if project is None else (project(out), None)
        fire.step(forces, stresses, check_only=(k == steps))
        if fire.relax_cell:
            host_lat = fire.lattice.cpu().numpy()   # (waits: the candidate search in the new cells needs them on the host)
            if fire.n_unconverged == 0 or k == steps:
                break
            vg.set_lattice(list(host_lat))
    return out


def _relax(model: Gradient, lat: list, pos: list, z: list, *, relax_cell: bool, fmax: float, steps: int, skin: float, device,
           optimizer: str = "fire", optimizer_params: dict | None = None) -> list:
    """`Relaxer.relax` on checked arguments, with the pair-virial `model` of the driver that calls it."""
    cfg = model.engine.cfg
    vg = VerletGraph(lat, z, cfg.cutoff, cfg.threebody_cutoff, skin=skin, device=device)
    pos_t = torch.tensor(np.concatenate(pos), dtype=torch.float64, device=vg.device)
    offsets = atom_offsets(z)
    lat64 = vg.lattice.clone()   # the optimiser's launch writes the relaxed cells here
    fire = OPTIMIZERS[optimizer][0](pos_t, lat64, offsets, relax_cell=relax_cell, fmax=fmax, **(optimizer_params or {}))
    out = fire_loop(vg, model, fire, steps)
    vg.raise_on_step_errors("relaxation")
    st = fire.read()
    e, f, sv = (out[key].double().cpu().numpy() for key in (K.TOTAL_ENERGY, K.FORCES, K.STRESSES))
    p_host, l_host = pos_t.cpu().numpy(), lat64.cpu().numpy()
    res = []
    for s in range(len(z)):
        a, b = int(offsets[s]), int(offsets[s + 1])
        res.append({"positions": p_host[a:b].copy(), "lattice": l_host[s].copy(), "total_energy": float(e[s]), "forces": f[a:b].copy(),
                    "stresses": sv[s].copy(), "n_steps": int(st["n_steps"][s]),
                    "converged": bool(st["flags"][s] & _lib.FIRE_CONVERGED), "error": bool(st["flags"][s] & _lib.FIRE_ERROR)})
    return res


class Relaxer(Driver):
    """Batched counterpart of m3g's `Relaxer` (scripts/relax_org.py): FIRE (the default) or, with `optimizer="lbfgs"`, L-BFGS, the
    cell relaxed by default (ASE's UnitCellFilter).  `optimizer_params`: ASE's parameters of that optimiser (`FIRE_DEFAULTS`,
    `LBFGS_DEFAULTS`); an unknown optimiser is a ValueError, an unknown parameter a TypeError.

    `model`: the `Gradient` returned by `build_model`; the relaxation evaluates a `pair_virial=True` engine made from its
    `Sequential` (the cell forces need the strain derivative, which the reference's stress formula is not)."""

    def __init__(self, model: Gradient, relax_cell: bool = True, skin: float = 0.5, device="cuda", optimizer: str = "fire",
                 **optimizer_params):
        if optimizer not in OPTIMIZERS:
            raise ValueError(f"optimizer must be one of {sorted(OPTIMIZERS)}; got {optimizer!r}")
        unknown = set(optimizer_params) - set(OPTIMIZERS[optimizer][1])
        if unknown:
            raise TypeError(f"unknown {optimizer} parameters {sorted(unknown)}")
        super().__init__(model, skin, device)
        self.relax_cell = bool(relax_cell)
        self.optimizer, self.optimizer_params = optimizer, dict(optimizer_params)

    def relax(self, lattices: Sequence, positions: Sequence, atomic_numbers: Sequence, fmax: float = 0.1, steps: int = 500) -> list:
        """Relax every structure (lattices: [3,3] rows = lattice vectors, positions: [n_s,3] Cartesian, atomic_numbers: [n_s]) until
        max_i |g_i| < fmax (cell rows included when the cell is relaxed) or `steps` optimiser steps.  Returns one dict per structure:
        positions [n_s,3], lattice [3,3], total_energy, forces [n_s,3], stresses [6] (pair virial) at the final positions, n_steps,
        converged, error (its forces became non-finite: it was stopped where it stood)."""
        fmax, steps = positive("fmax", fmax), integer("steps", steps, 0)
        lat, pos, z = structure_arrays(lattices, positions, atomic_numbers)
        return _relax(self.model, lat, pos, z, relax_cell=self.relax_cell, fmax=fmax, steps=steps, skin=self.skin, device=self.device,
                      optimizer=self.optimizer, optimizer_params=self.optimizer_params)
