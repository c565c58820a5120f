"""numpy fp64 restatement of batched FIRE relaxation (ASE's FIRE, optionally over ASE's UnitCellFilter), one structure at a time:
the yardstick of torch_m3gnet.relax / m3g_fire_* (tests/test_relax_cpu.py, tests/test_gpu_relax.py).

Per structure, ASE's Optimizer.run loop: evaluate -> converged? -> step, with

    first step:  v = 0
    otherwise:   P = g.v
                 P > 0:  v = (1 - a) v + a |v| g / |g|;  if n > Nmin: dt = min(dt finc, dtmax), a *= fa;  n += 1
                 else:   v = 0;  a = astart;  dt *= fdec;  n = 0
    v += dt g;  dr = dt v;  |dr| > maxstep: dr *= maxstep / |dr|   (norm over all rows of the structure);  X += dr

Cell filter (UnitCellFilter, linear deformation gradient): F = solve(L0, L)^T, cell_factor = number of atoms,
X = [solve(F, pos^T)^T ; cell_factor F], g = [f F ; solve(F, W^T)^T / cell_factor] with the virial W = V * stresses (Voigt
xx yy zz yz zx xy; pair-virial convention, W = -dE/d eps); after the step F' = X_cell / cell_factor, L = L0 F'^T, pos = X_atoms F'^T.
Converged: max_i |g_i| < fmax over every row; a converged structure is frozen.  Non-finite g: flagged, frozen, never moved."""
from __future__ import annotations

import numpy as np

DEFAULTS = dict(dt=0.1, maxstep=0.2, dtmax=1.0, nmin=5, finc=1.1, fdec=0.5, astart=0.1, fa=0.99)
STARTED, CONVERGED, ERROR = 1, 2, 4


def voigt_to_full(s6) -> np.ndarray:
    xx, yy, zz, yz, zx, xy = (float(x) for x in s6)
    return np.array([[xx, xy, zx], [xy, yy, yz], [zx, yz, zz]])


class FireReference:
    """One structure.  `pos` [n,3], `lattice` [3,3] (rows = lattice vectors); `step(forces, stresses)` with the forces / stresses
    evaluated at `self.pos` / `self.lattice` does what one m3g_fire_step call does to this structure."""

    def __init__(self, pos, lattice, relax_cell: bool, fmax: float, **params):
        self.p = dict(DEFAULTS, **params)
        self.fmax, self.relax_cell = float(fmax), bool(relax_cell)
        self.pos = np.array(pos, dtype=np.float64).reshape(-1, 3)
        self.lattice = np.array(lattice, dtype=np.float64).reshape(3, 3)
        self.L0 = self.lattice.copy()
        self.n_atoms = len(self.pos)
        self.cell_factor = float(self.n_atoms)
        self.F = np.eye(3)
        self.X = np.concatenate([self.pos, self.cell_factor * self.F]) if self.relax_cell else self.pos.copy()
        self.v = np.zeros_like(self.X)
        self.dt, self.a, self.n = self.p["dt"], self.p["astart"], 0
        self.flags, self.n_steps = 0, 0

    def generalized_forces(self, forces, stresses) -> np.ndarray:
        f = np.asarray(forces, dtype=np.float64).reshape(-1, 3)
        if not self.relax_cell:
            return f
        vol = abs(np.linalg.det(self.lattice))
        W = vol * voigt_to_full(stresses)
        g_cell = np.linalg.solve(self.F, W.T).T / self.cell_factor
        return np.concatenate([f @ self.F, g_cell])

    def step(self, forces, stresses=None, check_only: bool = False) -> None:
        if self.flags & (CONVERGED | ERROR):
            return
        g = self.generalized_forces(forces, stresses)
        if not np.isfinite(g).all():
            self.flags |= ERROR
            return
        if (g ** 2).sum(axis=1).max() < self.fmax ** 2:
            self.flags |= CONVERGED
            return
        if check_only:
            return
        p = self.p
        if not self.flags & STARTED:
            self.v = np.zeros_like(self.X)
        else:
            P = float(np.vdot(g, self.v))
            if P > 0.0:
                self.v = (1.0 - self.a) * self.v + self.a * g / np.sqrt(np.vdot(g, g)) * np.sqrt(np.vdot(self.v, self.v))
                if self.n > p["nmin"]:
                    self.dt = min(self.dt * p["finc"], p["dtmax"])
                    self.a *= p["fa"]
                self.n += 1
            else:
                self.v = np.zeros_like(self.X)
                self.a = p["astart"]
                self.dt *= p["fdec"]
                self.n = 0
        self.v = self.v + self.dt * g
        dr = self.dt * self.v
        norm = np.sqrt(np.vdot(dr, dr))
        if norm > p["maxstep"]:
            dr = p["maxstep"] * dr / norm
        self.X = self.X + dr
        self.flags |= STARTED
        self.n_steps += 1
        if self.relax_cell:
            Fn = self.X[self.n_atoms:] / self.cell_factor
            self.F = Fn
            self.lattice = self.L0 @ Fn.T
            self.pos = self.X[: self.n_atoms] @ Fn.T
        else:
            self.pos = self.X.copy()

    @property
    def converged(self) -> bool:
        return bool(self.flags & CONVERGED)


def relax(pos, lattice, energy_forces_virial, relax_cell=True, fmax=0.1, steps=500, **params):
    """The Optimizer.run loop over one structure: `energy_forces_virial(pos, lattice) -> (E, forces [n,3], W [3,3])`.  Returns the
    FireReference after the loop (converged or `steps` steps) and the last evaluation."""
    fr = FireReference(pos, lattice, relax_cell, fmax, **params)
    for k in range(steps + 1):
        ev = energy_forces_virial(fr.pos, fr.lattice)
        W = ev[2]
        s6 = np.array([W[0, 0], W[1, 1], W[2, 2], W[1, 2], W[2, 0], W[0, 1]]) / abs(np.linalg.det(fr.lattice))
        fr.step(ev[1], s6, check_only=(k == steps))
        if fr.flags & (CONVERGED | ERROR) or k == steps:
            return fr, ev
    return fr, ev
