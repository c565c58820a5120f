"""numpy fp64 restatement of batched L-BFGS relaxation (ASE's LBFGS without line search, optionally over ASE's UnitCellFilter), one
structure at a time: the yardstick of torch_m3gnet.relax.LbfgsState / m3g_lbfgs_* (tests/test_lbfgs_cpu.py, tests/test_gpu_lbfgs.py).

Per structure, ASE's Optimizer.run loop: evaluate -> converged? -> step, with grad = -g and

    stepped before:  s = X - X_prev, y = grad - grad_prev; the pair joins the history with rho = 1 / y.s unless y.s is zero or not
                     finite (ASE would divide by zero); only the newest `memory` pairs are kept
    q = grad;  newest to oldest: a_i = rho_i s_i.q, q -= a_i y_i;  z = H0 q (H0 = 1 / alpha);
    oldest to newest: b = rho_i y_i.z, z += s_i (a_i - b);  p = -z
    longest = max_row |p_row| (cell rows included);  longest >= maxstep: p *= maxstep / longest;  dr = damping p
    dr not finite: flagged, not moved;  else X_prev = X, grad_prev = grad, X += dr

The cell filter, the verdicts and the freezing are those of fire_reference.py."""
from __future__ import annotations

import numpy as np

from fire_reference import voigt_to_full

DEFAULTS = dict(maxstep=0.2, memory=100, damping=1.0, alpha=70.0)
STARTED, CONVERGED, ERROR = 1, 2, 4


def two_loop(grad, s, y, rho, h0):
    """p = -H grad by the two-loop recursion over the pairs (oldest first)."""
    q = grad.copy()
    a = np.empty(len(s))
    for i in range(len(s) - 1, -1, -1):
        a[i] = rho[i] * np.vdot(s[i], q)
        q -= a[i] * y[i]
    z = h0 * q
    for i in range(len(s)):
        b = rho[i] * np.vdot(y[i], z)
        z += s[i] * (a[i] - b)
    return -z


class LbfgsReference:
    """One structure.  `pos` [n,3], `lattice` [3,3] (rows = lattice vectors); `step(forces, stresses)` with the forces / stresses
    evaluated at `self.pos` / `self.lattice` does what one m3g_lbfgs_step call does to this structure."""

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
        self.X_prev = self.grad_prev = None
        self.s, self.y, self.rho = [], [], []
        self.flags, self.n_steps = 0, 0
        self.clipped = self.wrapped = self.rejected = 0   # what the tests ask of a run

    @property
    def n_pairs(self) -> int:
        return len(self.s)

    def generalized_forces(self, forces, stresses) -> np.ndarray:
        f = np.asarray(forces, dtype=np.float64).reshape(-1, 3)
        if not self.relax_cell:
            return f
        vol = abs(np.linalg.det(self.lattice))
        W = vol * voigt_to_full(stresses)
        g_cell = np.linalg.solve(self.F, W.T).T / self.cell_factor
        return np.concatenate([f @ self.F, g_cell])

    def direction(self, grad) -> np.ndarray:
        return two_loop(grad, self.s, self.y, self.rho, 1.0 / self.p["alpha"])

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
        grad = -g
        if self.flags & STARTED:
            s, y = self.X - self.X_prev, grad - self.grad_prev
            ys = float(np.vdot(y, s))
            if ys != 0.0 and np.isfinite(ys):
                self.s.append(s), self.y.append(y), self.rho.append(1.0 / ys)
                if len(self.s) > p["memory"]:
                    self.s.pop(0), self.y.pop(0), self.rho.pop(0)
                    self.wrapped += 1
            else:
                self.rejected += 1
        d = self.direction(grad)
        longest = np.sqrt((d ** 2).sum(axis=1).max())
        if longest >= p["maxstep"]:
            d = d * (p["maxstep"] / longest)
            self.clipped += 1
        dr = p["damping"] * d
        if not np.isfinite(dr).all():
            self.flags |= ERROR
            return
        self.X_prev, self.grad_prev = self.X.copy(), grad
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
    LbfgsReference after the loop (converged or `steps` steps) and the last evaluation."""
    lb = LbfgsReference(pos, lattice, relax_cell, fmax, **params)
    for k in range(steps + 1):
        ev = energy_forces_virial(lb.pos, lb.lattice)
        W = ev[2]
        s6 = np.array([W[0, 0], W[1, 1], W[2, 2], W[1, 2], W[2, 0], W[0, 1]]) / abs(np.linalg.det(lb.lattice))
        lb.step(ev[1], s6, check_only=(k == steps))
        if lb.flags & (CONVERGED | ERROR) or k == steps:
            return lb, ev
    return lb, ev
