"""numpy fp64 restatement of batched molecular dynamics (torch_m3gnet.dynamics / m3g_dyn_*), one structure at a time: the yardstick
of tests/test_dynamics_cpu.py and tests/test_gpu_dynamics.py.

Units: A, fs, amu, eV; a_i = KAPPA F_i / m_i; KE = sum m |v|^2 / (2 KAPPA); T = 2 KE / (3 n KB).  One `step(forces, stresses)` with the
forces at `self.pos` does what one m3g_dyn_step call does to this structure:

    finish (started):   v += dt/2 a
    observables:        KE, T, P = (tr W + 2 KE) / (3 V) with W = V * stresses, V
    start (not finish_only; finish_only clears `started` instead):
      nve:              v += dt/2 a;  fix_com: v_i -= mean_j(m_j v_j) / m_i;  x += dt v
      nvt_berendsen:    lambda = clamp(sqrt(max(1 + dt/taut (T0/T - 1), 0)), 0.9, 1.1)  (1.1 at T = 0);  v = lambda v;  then nve
      npt_berendsen:    lambda as nvt;  v = lambda v;  P = (tr W + lambda^2 2 KE) / (3 V);  mu = 1 - dt beta / (3 taup) (P0 - P);
                        L = mu L;  x = mu x;  then nve (forces of the unscaled positions)
      nvt_langevin:     BAOAB: v += dt/2 a;  x += dt/2 v;  v = c1 v + sqrt((1 - c1^2) KB T0 KAPPA / m) xi;  x += dt/2 v
                        (c1 = exp(-friction dt); xi from Philox4x64-10, key (seed, 0), counter (k, local atom index, 0, 0))
Non-finite forces (NPT: or stresses): flagged ERROR, frozen from then on."""
from __future__ import annotations

import numpy as np

KAPPA = 9.648533215665e-3   # A/fs^2 per eV/(A amu)
KB = 8.617333262e-5         # eV/K
STARTED, ERROR = 1, 2
ENSEMBLES = {"nve": 0, "nvt_berendsen": 1, "nvt_langevin": 2, "npt_berendsen": 3}

_M32 = np.uint64(0xFFFFFFFF)
_PHILOX_M = (np.uint64(0xD2E7470EE14C6C93), np.uint64(0xCA5A826395121157))
_PHILOX_W = (np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBB67AE8584CAA73B))


def _mulhilo(a, b):
    a = np.asarray(a, dtype=np.uint64)
    b = np.asarray(b, dtype=np.uint64)
    s32 = np.uint64(32)
    al, ah, bl, bh = a & _M32, a >> s32, b & _M32, b >> s32
    p0, p1, p2, p3 = al * bl, al * bh, ah * bl, ah * bh
    mid = (p0 >> s32) + (p1 & _M32) + (p2 & _M32)
    return p3 + (p1 >> s32) + (p2 >> s32) + (mid >> s32), a * b


def philox4x64_10(ctr, key):
    """Philox4x64-10 blocks: ctr [..., 4], key [..., 2] (uint64, broadcast) -> [..., 4] uint64."""
    with np.errstate(over="ignore"):
        ctr = np.asarray(ctr, dtype=np.uint64)
        key = np.asarray(key, dtype=np.uint64)
        c0, c1, c2, c3 = (ctr[..., j] for j in range(4))
        k0, k1 = key[..., 0], key[..., 1]
        for r in range(10):
            if r:
                k0, k1 = k0 + _PHILOX_W[0], k1 + _PHILOX_W[1]
            hi0, lo0 = _mulhilo(_PHILOX_M[0], c0)
            hi1, lo1 = _mulhilo(_PHILOX_M[1], c2)
            c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1)


def gaussians(seed: int, k: int, n: int) -> np.ndarray:
    """[n, 3] standard normals of the n atoms of a structure seeded `seed` at its start number k."""
    ctr = np.zeros((n, 4), dtype=np.uint64)
    ctr[:, 0] = np.uint64(k)
    ctr[:, 1] = np.arange(n, dtype=np.uint64)
    w = philox4x64_10(ctr, np.array([seed, 0], dtype=np.uint64))
    u = ((w >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53
    r0, r1 = np.sqrt(-2.0 * np.log(u[:, 0])), np.sqrt(-2.0 * np.log(u[:, 2]))
    two_pi = 6.283185307179586
    return np.stack([r0 * np.cos(two_pi * u[:, 1]), r0 * np.sin(two_pi * u[:, 1]), r1 * np.cos(two_pi * u[:, 3])], axis=1)


class DynReference:
    """One structure: `pos` [n,3] (unwrapped), `lattice` [3,3] (rows = lattice vectors), `masses` [n] amu, `vel` [n,3] A/fs."""

    def __init__(self, pos, lattice, masses, vel, ensemble="nve", temperature=0.0, seed=0, dt=1.0, taut=100.0, friction=0.01,
                 pressure=0.0, taup=1000.0, compressibility=1.0, fix_com=False):
        self.ensemble = ensemble
        self.pos = np.array(pos, dtype=np.float64).reshape(-1, 3)
        self.lattice = np.array(lattice, dtype=np.float64).reshape(3, 3)
        self.m = np.array(masses, dtype=np.float64).reshape(-1)
        self.v = np.array(vel, dtype=np.float64).reshape(-1, 3)
        self.t0, self.seed = float(temperature), int(seed)
        self.dt, self.taut, self.friction, self.p0, self.taup, self.beta = dt, taut, friction, pressure, taup, compressibility
        self.fix_com = bool(fix_com)
        self.flags, self.n_steps = 0, 0
        self.lam = self.mu = 1.0
        self.obs = np.full(4, np.nan)

    def step(self, forces, stresses=None, finish_only: bool = False) -> None:
        if self.flags & ERROR:
            return
        f = np.asarray(forces, dtype=np.float64).reshape(-1, 3)
        s6 = None if stresses is None else np.asarray(stresses, dtype=np.float64).reshape(6)
        npt = self.ensemble == "npt_berendsen"
        if not np.isfinite(f).all() or (npt and not np.isfinite(s6).all()):
            self.flags |= ERROR
            return
        n, h, m = len(self.m), 0.5 * self.dt, self.m[:, None]
        a = KAPPA * f / m
        v = self.v + h * a if self.flags & STARTED else self.v.copy()
        ke = (m[:, 0] * (v * v).sum(1)).sum() / (2.0 * KAPPA)
        two_ke = 2.0 * ke
        temp = two_ke / (3.0 * n * KB)
        L = self.lattice
        vol = abs(L[0, 0] * (L[1, 1] * L[2, 2] - L[1, 2] * L[2, 1]) - L[0, 1] * (L[1, 0] * L[2, 2] - L[1, 2] * L[2, 0])
                  + L[0, 2] * (L[1, 0] * L[2, 1] - L[1, 1] * L[2, 0]))
        trw = vol * ((s6[0] + s6[1]) + s6[2]) if s6 is not None else np.nan
        self.obs = np.array([ke, temp, (trw + two_ke) / (3.0 * vol), vol])
        if finish_only:
            self.v = v
            self.flags &= ~STARTED
            return
        x = self.pos.copy()
        lam = mu = 1.0
        if self.ensemble in ("nvt_berendsen", "npt_berendsen"):
            if temp == 0.0:
                lam = 1.1
            else:
                lam = min(max(np.sqrt(max(1.0 + (self.dt / self.taut) * (self.t0 / temp - 1.0), 0.0)), 0.9), 1.1)
        if npt:
            pressure = (trw + lam * lam * two_ke) / (3.0 * vol)
            mu = 1.0 - (self.dt * self.beta / (3.0 * self.taup)) * (self.p0 - pressure)
            self.lattice = mu * self.lattice
        if self.ensemble == "nvt_langevin":
            c1 = np.exp(-self.friction * self.dt)
            xi = gaussians(self.seed, self.n_steps, n)
            sigma = np.sqrt((1.0 - c1 * c1) * KB * self.t0 * KAPPA / m)
            v = v + h * a
            x = x + h * v
            v = c1 * v + sigma * xi
            x = x + h * v
        else:
            v = lam * v
            v = v + h * a
            if self.fix_com:
                v = v - (m * v).sum(0) / n / m
            x = mu * x
            x = x + self.dt * v
        self.v, self.pos, self.lam, self.mu = v, x, lam, mu
        self.flags |= STARTED
        self.n_steps += 1

    @property
    def kinetic_energy(self) -> float:
        return float((self.m * (self.v * self.v).sum(1)).sum() / (2.0 * KAPPA))
