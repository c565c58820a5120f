"""numpy fp64 restatement of the batched climbing-image NEB (ASE's NEB(method="improvedtangent", climb=...).get_forces driven by
ASE's FIRE): the yardstick of torch_m3gnet.neb / m3g_neb_* (tests/test_neb_cpu.py, tests/test_gpu_neb.py).

For interior image i of a band with energies V and positions R (3n vectors, never wrapped):

    tau+ = R_i+1 - R_i,  tau- = R_i - R_i-1
    tau  = tau+                                   if V_i+1 > V_i > V_i-1
           tau-                                   if V_i+1 < V_i < V_i-1
           dVmax tau+ + dVmin tau-                 otherwise, if V_i+1 > V_i-1
           dVmin tau+ + dVmax tau-                 otherwise
           (dVmax / dVmin: max / min of |V_i+1 - V_i| and |V_i-1 - V_i|);   tau_hat = tau / |tau|
    ordinary image:  F_neb = F - (F.tau_hat) tau_hat + k (|tau+| - |tau-|) tau_hat
    climbing image:  F_neb = F - 2 (F.tau_hat) tau_hat       (the interior image of highest energy, lowest index on ties)

An image with a non-finite input or |tau| = 0 gets NaN rows.  The optimiser is tests/fire_reference.FireReference with the cell fixed
over all interior rows of the band as ONE structure (ASE's FIRE over the NEB optimizable)."""
from __future__ import annotations

import numpy as np

import fire_reference as fr


def tangent(v_prev, v, v_next, tau_plus, tau_minus) -> np.ndarray:
    """ASE's ImprovedTangentMethod.get_tangent before normalisation."""
    if v_next > v > v_prev:
        return tau_plus.copy()
    if v_next < v < v_prev:
        return tau_minus.copy()
    dmax = max(abs(v_next - v), abs(v_prev - v))
    dmin = min(abs(v_next - v), abs(v_prev - v))
    if v_next > v_prev:
        return tau_plus * dmax + tau_minus * dmin
    return tau_plus * dmin + tau_minus * dmax


def climbing_index(interior_energies) -> int:
    """Index (among the interior images) of the highest energy, the lowest one on ties; -1 if every energy is NaN."""
    e = np.asarray(interior_energies, dtype=np.float64)
    best = -1
    for i, v in enumerate(e):
        if v == v and (best < 0 or v > e[best]):
            best = i
    return best


def neb_forces(images, energies, forces, k: float, climb: bool):
    """images: M arrays [n,3] (endpoints included); energies [M]; forces: M-2 arrays [n,3] of the interior images.  Returns the NEB
    forces [M-2, n, 3] (fp64) and the observables rows [M-2, 5]: |tau+|, |tau-|, F.tau_hat, spring term (0 at the climbing image),
    climbing flag."""
    R = [np.asarray(p, dtype=np.float64) for p in images]
    V = [float(x) for x in energies]
    m = len(R)
    imax = 1 + climbing_index(V[1:-1]) if climb else -1
    out = np.empty((m - 2,) + R[0].shape)
    rows = np.empty((m - 2, 5))
    for i in range(1, m - 1):
        f = np.asarray(forces[i - 1], dtype=np.float64)
        tp, tm = R[i + 1] - R[i], R[i] - R[i - 1]
        t = tangent(V[i - 1], V[i], V[i + 1], tp, tm)
        with np.errstate(invalid="ignore", divide="ignore"):
            t = t / np.linalg.norm(t)
            ft = float(np.vdot(f, t))
            if i == imax:
                fn = f - 2.0 * ft * t
                spring = 0.0
            else:
                spring = k * (np.linalg.norm(tp) - np.linalg.norm(tm))
                fn = f - ft * t + spring * t
        finite = all(np.isfinite(x).all() for x in (R[i - 1], R[i], R[i + 1], f)) and np.isfinite([V[i - 1], V[i], V[i + 1]]).all()
        out[i - 1] = fn if finite and np.isfinite(fn).all() else np.nan
        rows[i - 1] = [np.linalg.norm(tp), np.linalg.norm(tm), ft, spring, 1.0 if i == imax else 0.0]
    return out, rows


class BandReference:
    """One band under FIRE: `step(energies, forces)` with the interior images' energies [M-2] and forces [M-2, n, 3] evaluated at
    `self.images[1:-1]` does what one neb_forces + fire_step pair does to this band.  `f32`: the NEB forces are rounded to float32
    before FIRE reads them, as the device stores them."""

    def __init__(self, images, endpoint_energies, k=0.1, climb=True, fmax=0.05, f32=True, **fire_params):
        self.images = [np.array(p, dtype=np.float64).reshape(-1, 3) for p in images]
        self.n = len(self.images[0])
        self.e0, self.e1 = (float(x) for x in endpoint_energies)
        self.k, self.climb, self.f32 = float(k), bool(climb), bool(f32)
        inner = np.concatenate(self.images[1:-1])
        self.fire = fr.FireReference(inner, np.eye(3), False, fmax, **fire_params)
        self.neb_forces = self.rows = self.energies = None

    def step(self, energies, forces, check_only: bool = False) -> None:
        self.energies = np.concatenate([[self.e0], np.asarray(energies, dtype=np.float64), [self.e1]])
        nf, self.rows = neb_forces(self.images, self.energies, forces, self.k, self.climb)
        self.neb_forces = nf.astype(np.float32).astype(np.float64) if self.f32 else nf
        self.fire.step(self.neb_forces.reshape(-1, 3), check_only=check_only)
        inner = self.fire.pos.reshape(-1, self.n, 3)
        self.images = [self.images[0]] + [p.copy() for p in inner] + [self.images[-1]]

    @property
    def climbing_image(self) -> int:
        hit = np.flatnonzero(self.rows[:, 4] == 1.0)
        return int(hit[0]) + 1 if len(hit) else -1


def run_band(images, energy_forces, k=0.1, climb=True, fmax=0.05, steps=500, f32=True, **fire_params) -> BandReference:
    """The Optimizer.run loop over one band: `energy_forces(pos [n,3]) -> (E, forces [n,3])` evaluates one image (the endpoints once).
    With `f32` the energies and forces are rounded to float32, as the engine returns them.  Returns the BandReference after the loop
    (converged, failed or `steps` steps); its `energies` / `neb_forces` belong to the final images."""
    cast = (lambda x: np.asarray(x, dtype=np.float32).astype(np.float64)) if f32 else (lambda x: np.asarray(x, dtype=np.float64))
    e0, e1 = (float(cast(energy_forces(p)[0])) for p in (images[0], images[-1]))
    band = BandReference(images, (e0, e1), k=k, climb=climb, fmax=fmax, f32=f32, **fire_params)
    for it in range(steps + 1):
        ev = [energy_forces(p) for p in band.images[1:-1]]
        band.step(cast([e for e, _ in ev]), np.stack([cast(f) for _, f in ev]), check_only=(it == steps))
        if band.fire.flags & (fr.CONVERGED | fr.ERROR) or it == steps:
            return band
    return band
