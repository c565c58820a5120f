"""numpy fp64 restatement of the Nose-Hoover chain NVT and isotropic MTK NPT ensembles of batched molecular dynamics
(torch_m3gnet.dynamics / m3g_nhc_*), one structure at a time: the yardstick of tests/test_nhc_cpu.py and tests/test_gpu_nhc.py, with
the interface of md_reference.DynReference.

Units as md_reference: A, fs, amu, eV; a_i = KAPPA F_i / m_i; 2 KE = sum m |v|^2 / KAPPA; thermostat and barostat velocities vxi, veps
in 1/fs; their masses Q, W in eV fs^2.  Per structure: g = 3 n - 3 (fix_com) or 3 n, kT = KB T0, Q_1 = g kT taut^2, Q_k>1 = kT taut^2,
barostat chain masses kT taup^2, W = (g + 3) kT taup^2, alpha = 1 + 3 / g.

One step is T(h) B(h) A(dt) [forces] B(h) T(h), h = dt / 2 (Martyna, Tuckerman, Tobias, Klein 1996), and one `step(forces, stresses)`
with the forces at `self.pos` does what one m3g_nhc_step call does: finish the step under way, write the observables, start the next:

    finish (started):   B(h): v = v kA + a kB, the coefficients of the start's kick (veps has not changed since)
                        NPT: veps += h G_eps;  barostat chain half-step (scales veps);  particle chain half-step (v = s1 v)
    observables:        KE, T = 2 KE / (3 n KB), P = (tr W + 2 KE) / (3 V), V, extended, 0
    start (not finish_only; finish_only clears `started` instead):
                        particle chain half-step (v = s2 v);  NPT: barostat chain half-step;  veps += h G_eps
                        B(h): NVT kA = 1, kB = h;  NPT y = alpha veps h / 2, kA = exp(-2 y), kB = h exp(-y) sinhc(y)
                        fix_com: v_i -= mean_j(m_j v_j) / m_i
                        A(dt): NVT x += dt v;  NPT y = veps h, x = x exp(2 y) + v dt exp(y) sinhc(y), lattice = exp(2 y) lattice
    G_eps = (alpha 2 KE + tr W - 3 V P_ext) / W_baro, with tr W = V (s0 + s1 + s2) of the pair-virial stresses.
The kinetic energy after a uniform scale is known in closed form (s^2 times the sum over the atoms), as in the kernel.
extended = g kT xi_0 + kT sum_{k>0} xi_k + 1/2 sum Q vxi^2 (+ P_ext V + 1/2 W veps^2 + kT sum xib + 1/2 sum Qb vxib^2 in NPT):
e_pot + KE + extended is conserved.  Non-finite forces (NPT: or stresses): flagged ERROR, frozen from then on."""
from __future__ import annotations

import numpy as np

KAPPA = 9.648533215665e-3   # A/fs^2 per eV/(A amu)
KB = 8.617333262e-5         # eV/K
STARTED, ERROR = 1, 2
ENSEMBLES = {"nvt_nose_hoover": 0, "npt_mtk": 1}


def sinhc(y):
    """sinh(y) / y as its series to y^6: the next term is y^8 / 362880, below 2^-53 for |y| < 0.05."""
    y2 = y * y
    return 1.0 + y2 / 6.0 * (1.0 + y2 / 20.0 * (1.0 + y2 / 42.0))


def chain_half_step(q, xi, vxi, k2, gkt, kt, h, n_c):
    """The chain half-step of length h in n_c equal parts, in place on xi, vxi: returns (scale, scale^2 k2)."""
    m = len(q)
    d = h / n_c
    scale = 1.0

    def force(k, k2):
        return (k2 - gkt) / q[0] if k == 0 else (q[k - 1] * vxi[k - 1] * vxi[k - 1] - kt) / q[k]

    for _ in range(n_c):
        vxi[m - 1] += 0.5 * d * force(m - 1, k2)
        for k in range(m - 2, -1, -1):
            e = np.exp(-0.25 * d * vxi[k + 1])
            vxi[k] = (vxi[k] * e + 0.5 * d * force(k, k2)) * e
        s = np.exp(-d * vxi[0])
        scale *= s
        k2 = s * s * k2
        for k in range(m):
            xi[k] += d * vxi[k]
        for k in range(m - 1):
            e = np.exp(-0.25 * d * vxi[k + 1])
            vxi[k] = (vxi[k] * e + 0.5 * d * force(k, k2)) * e
        vxi[m - 1] += 0.5 * d * force(m - 1, k2)
    return scale, k2


class NhcReference:
    """One structure: `pos` [n,3] (unwrapped), `lattice` [3,3] (rows = lattice vectors), `masses` [n] amu, `vel` [n,3] A/fs."""

    def __init__(self, pos, lattice, masses, vel, ensemble="nvt_nose_hoover", temperature=300.0, dt=1.0, taut=100.0, pressure=0.0,
                 taup=1000.0, chain_length=3, chain_substeps=1, fix_com=True):
        if ensemble not in ENSEMBLES:
            raise ValueError(f"unknown ensemble {ensemble!r}")
        self.ensemble = ensemble
        self.npt = ensemble == "npt_mtk"
        self.pos = np.array(pos, dtype=np.float64).reshape(-1, 3)
        self.lattice = np.array(lattice, dtype=np.float64).reshape(3, 3)
        self.m = np.array(masses, dtype=np.float64).reshape(-1)
        self.v = np.array(vel, dtype=np.float64).reshape(-1, 3)
        self.t0, self.dt, self.taut, self.p0, self.taup = float(temperature), dt, taut, pressure, taup
        self.M, self.n_c, self.fix_com = int(chain_length), int(chain_substeps), bool(fix_com)
        n = len(self.m)
        if not (1 <= self.M <= 8 and 1 <= self.n_c <= 8) or not self.t0 > 0.0 or (self.fix_com and n == 1):
            raise ValueError("chain_length and chain_substeps in 1..8, temperature > 0, more than one atom with fix_com")
        self.g = 3.0 * n - 3.0 if self.fix_com else 3.0 * n
        self.kt = KB * self.t0
        self.q = np.full(self.M, self.kt * taut * taut)
        self.q[0] = self.g * self.kt * taut * taut
        self.qb = np.full(self.M, self.kt * taup * taup)
        self.w = (self.g + 3.0) * self.kt * taup * taup
        self.alpha = 1.0 + 3.0 / self.g
        self.xi, self.vxi, self.xib, self.vxib = (np.zeros(self.M) for _ in range(4))
        self.veps = 0.0
        self.kick = (1.0, 0.0)
        self.flags, self.n_steps = 0, 0
        self.lam = 1.0
        self.obs = np.full(6, np.nan)

    def _volume(self):
        L = self.lattice
        return abs(L[0, 0] * (L[1, 1] * L[2, 2] - L[1, 2] * L[2, 1]) - L[0, 1] * (L[1, 0] * L[2, 2] - L[1, 2] * L[2, 0])
                   + L[0, 2] * (L[1, 0] * L[2, 1] - L[1, 1] * L[2, 0]))

    def _g_eps(self, k2, vol, trw):
        return (self.alpha * k2 + trw - 3.0 * vol * self.p0) / self.w

    def _baro_chain(self, h):
        s, _ = chain_half_step(self.qb, self.xib, self.vxib, self.w * self.veps * self.veps, self.kt, self.kt, h, self.n_c)
        self.veps = self.veps * s

    def extended(self, vol):
        e = self.g * self.kt * self.xi[0] + self.kt * self.xi[1:].sum() + 0.5 * (self.q * self.vxi * self.vxi).sum()
        if self.npt:
            e += self.p0 * vol + 0.5 * self.w * self.veps * self.veps + self.kt * self.xib.sum() + 0.5 * (self.qb * self.vxib * self.vxib).sum()
        return e

    def step(self, forces, stresses=None, finish_only: bool = False) -> None:
        if self.flags & ERROR:
            return
        f = np.asarray(forces, dtype=np.float64).reshape(-1, 3)
        s6 = None if stresses is None else np.asarray(stresses, dtype=np.float64).reshape(6)
        if not np.isfinite(f).all() or (self.npt and not np.isfinite(s6).all()):
            self.flags |= ERROR
            return
        n, h, m = len(self.m), 0.5 * self.dt, self.m[:, None]
        a = KAPPA * f / m
        started = bool(self.flags & STARTED)
        v = self.v * self.kick[0] + a * self.kick[1] if started else self.v.copy()
        k2 = (m[:, 0] * (v * v).sum(1)).sum() / KAPPA
        mv, fsum = (m * v).sum(0), f.sum(0)
        vol = self._volume()
        trw = vol * ((s6[0] + s6[1]) + s6[2]) if s6 is not None else np.nan
        gkt = self.g * self.kt
        s1 = 1.0
        if started:
            if self.npt:
                self.veps += h * self._g_eps(k2, vol, trw)
                self._baro_chain(h)
            s1, k2 = chain_half_step(self.q, self.xi, self.vxi, k2, gkt, self.kt, h, self.n_c)
        self.obs = np.array([0.5 * k2, k2 / (3.0 * n * KB), (trw + k2) / (3.0 * vol), vol, self.extended(vol), 0.0])
        if finish_only:
            self.v = s1 * v
            self.flags &= ~STARTED
            return
        s2, k2 = chain_half_step(self.q, self.xi, self.vxi, k2, gkt, self.kt, h, self.n_c)
        lam = s1 * s2
        ka, kb, da, db = 1.0, h, 1.0, self.dt
        if self.npt:
            self._baro_chain(h)
            self.veps += h * self._g_eps(k2, vol, trw)
            y = 0.5 * self.alpha * self.veps * h
            ka, kb = np.exp(-2.0 * y), h * np.exp(-y) * sinhc(y)
            y = self.veps * h
            da, db = np.exp(2.0 * y), self.dt * np.exp(y) * sinhc(y)
            self.lattice = da * self.lattice
        v = lam * v
        v = v * ka + a * kb
        if self.fix_com:
            v = v - (ka * lam * mv + kb * KAPPA * fsum) / n / m
        self.pos = self.pos * da + v * db
        self.v, self.kick, self.lam = v, (ka, kb), lam
        self.flags |= STARTED
        self.n_steps += 1

    def reverse(self) -> None:
        """Negate every velocity (after a finish_only step): the next steps retrace the trajectory."""
        self.v, self.vxi, self.vxib, self.veps = -self.v, -self.vxi, -self.vxib, -self.veps
