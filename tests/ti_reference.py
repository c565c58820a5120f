"""numpy fp64 restatement of batched thermodynamic integration to an Einstein crystal (torch_m3gnet.free_energy / m3g_ti_*), one
structure at a time: the yardstick of tests/test_ti_cpu.py and tests/test_gpu_ti.py.

Units: A, fs, amu, eV, K.  H(lambda) = KE + lambda E_model(x) + (1 - lambda) U_s(x), U_s = 1/2 sum_i k_i |x_i - r0_i|^2.  With u_i = x_i -
r0_i and G_i = lambda F_i - (1 - lambda) k_i u_i the force on atom i is G_i - (m_i / M) sum_j G_j: the centre of mass is held.  One
`step(forces, energy, finish_only)` with the model's forces and energy at `self.pos` does what one m3g_ti_step call does to this
structure (BAOAB, h = dt / 2):

    lambda = lambda_b + (lambda_e - lambda_b) g(min(c, n_switch) / n_switch)   (lambda_b when n_switch = 0)
    finish (started):   v += h a,  a_i = KAPPA (G_i - m_i sum_j G_j / M) / m_i
    D = E - U_s;  W += (lambda - lambda_prev) (D + D_prev) / 2 (not on the first call of a path);  when c >= n_discard: D into Welford's
    count / mean / M2 and |u_i|^2 into the per-atom sums
    observables:        KE, T = 2 KE / ((3 n - 3) KB), U_s, D, lambda, W, 0, 0
    start (not finish_only; finish_only clears `started` instead):
      B(h)   v += h a
      A(h)   x += h v
      O(dt)  v_i = c1 v_i + sigma_i xi_i - pbar / M, c1 = exp(-friction dt), sigma_i = sqrt((1 - c1^2) KB T KAPPA / m_i), pbar = sum_j m_j
             sigma_j xi_j; xi from Philox4x64-10, key (seed, 4), counter (n_steps, atom, 0, 0), the Box-Muller of md_reference.gaussians
      A(h)   x += h v;  c += 1
A non-finite force or energy: flagged ERROR, frozen from then on (`path` leaves such a structure alone too)."""
from __future__ import annotations

import numpy as np

from md_reference import ERROR, KAPPA, KB, STARTED, philox4x64_10

SCHEDULES = {"linear": 0, "smooth": 1}
NOISE_BLOCKS = 1 << 16   # Philox blocks drawn at a time: the starts ahead that fit (numpy's overhead per call, not the numbers)


def schedule_value(schedule: str, t: float) -> float:
    """g(t) on [0, 1]: t, or the polynomial of Freitas, Asta, de Koning (2016) whose first four derivatives vanish at both ends."""
    if schedule == "linear":
        return t
    t2 = t * t
    return t2 * t2 * t * (70.0 * t2 * t2 - 315.0 * t2 * t + 540.0 * t2 - 420.0 * t + 126.0)


def ti_gaussians(seed: int, steps, n: int) -> np.ndarray:
    """[len(steps), n, 3] standard normals of the n atoms of a structure seeded `seed` at its starts number `steps`."""
    steps = np.asarray(steps, dtype=np.uint64).reshape(-1)
    ctr = np.zeros((len(steps), n, 4), dtype=np.uint64)
    ctr[..., 0] = steps[:, None]
    ctr[..., 1] = np.arange(n, dtype=np.uint64)[None, :]
    w = philox4x64_10(ctr, np.array([seed, 4], dtype=np.uint64))
    u = ((w >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53
    r0, r1 = np.sqrt(-2.0 * np.log(u[..., 0])), np.sqrt(-2.0 * np.log(u[..., 2]))
    two_pi = 6.283185307179586
    return np.stack([r0 * np.cos(two_pi * u[..., 1]), r0 * np.sin(two_pi * u[..., 1]), r1 * np.cos(two_pi * u[..., 3])], axis=-1)


class TiReference:
    """One structure: `pos` [n,3] (unwrapped), `masses` [n] amu, `springs` [n] eV/A^2, `vel` [n,3] A/fs, `reference` [n,3] sites."""

    def __init__(self, pos, masses, springs, vel, reference, temperature, seed=0, schedule="smooth", dt=1.0, friction=0.01):
        self.pos = np.array(pos, dtype=np.float64).reshape(-1, 3)
        self.v = np.array(vel, dtype=np.float64).reshape(-1, 3)
        self.r0 = np.array(reference, dtype=np.float64).reshape(-1, 3)
        self.m = np.array(masses, dtype=np.float64).reshape(-1)
        self.k = np.array(springs, dtype=np.float64).reshape(-1)
        self.n = len(self.m)
        assert self.pos.shape == self.v.shape == self.r0.shape == (self.n, 3) and self.k.shape == (self.n,) and self.n >= 2
        assert schedule in SCHEDULES
        self.schedule, self.t0, self.seed, self.dt, self.friction = schedule, float(temperature), int(seed), float(dt), float(friction)
        self.mtot = 0.0
        for x in self.m:   # (the order of the init call's host loop)
            self.mtot += x
        self.c1 = np.exp(-self.friction * self.dt)
        self.flags, self.n_steps = 0, 0
        self.obs = np.full(8, np.nan)
        self._noise, self._noise_from = None, 0
        self.path(1.0, 1.0, 0, 0)

    def path(self, lambda_begin: float, lambda_end: float, n_switch: int, n_discard: int = 0) -> None:
        if self.flags & ERROR:
            return
        self.lam_b, self.lam_e, self.n_switch, self.n_discard, self.c = float(lambda_begin), float(lambda_end), int(n_switch), int(n_discard), 0
        self.work, self.lam_prev, self.d_prev, self.has_prev = 0.0, 0.0, 0.0, False
        self.count, self.mean, self.m2 = 0, 0.0, 0.0
        self.msd_sum = np.zeros(self.n)

    @property
    def lam(self) -> float:
        if self.n_switch == 0:
            return self.lam_b
        if self.c >= self.n_switch:
            return self.lam_e   # (the end of the path to the bit)
        return self.lam_b + (self.lam_e - self.lam_b) * schedule_value(self.schedule, min(self.c, self.n_switch) / self.n_switch)

    def _gaussians(self):
        k = self.n_steps - self._noise_from
        if self._noise is None or not 0 <= k < len(self._noise):
            self._noise_from, k = self.n_steps, 0
            self._noise = ti_gaussians(self.seed, self.n_steps + np.arange(max(1, NOISE_BLOCKS // self.n)), self.n)
        return self._noise[k]

    def step(self, forces, energy, finish_only: bool = False) -> None:
        if self.flags & ERROR:
            return
        f = np.asarray(forces, dtype=np.float64).reshape(-1, 3)
        e = float(energy)
        if not (np.isfinite(f).all() and np.isfinite(e)):
            self.flags |= ERROR
            return
        n, h, m, k, lam = self.n, 0.5 * self.dt, self.m[:, None], self.k[:, None], self.lam
        u = self.pos - self.r0
        g = lam * f - (1.0 - lam) * (k * u)
        a = KAPPA * (g - m * (g.sum(0) / self.mtot)) / m
        v = self.v + h * a if self.flags & STARTED else self.v.copy()
        u2 = (u * u).sum(1)
        us = 0.5 * (self.k * u2).sum()
        d = e - us
        if self.has_prev:
            self.work += (lam - self.lam_prev) * (0.5 * (d + self.d_prev))
        self.lam_prev, self.d_prev, self.has_prev = lam, d, True
        if self.c >= self.n_discard:
            self.count += 1
            delta = d - self.mean
            self.mean += delta / self.count
            self.m2 += delta * (d - self.mean)
            self.msd_sum = self.msd_sum + u2
        ke = (m[:, 0] * (v * v).sum(1)).sum() / (2.0 * KAPPA)
        self.obs = np.array([ke, 2.0 * ke / ((3.0 * n - 3.0) * KB), us, d, lam, self.work, 0.0, 0.0])
        if finish_only:
            self.v = v
            self.flags &= ~STARTED
            return
        v = v + h * a
        x = self.pos + h * v
        if self.c1 < 1.0:
            sigma = np.sqrt((1.0 - self.c1 * self.c1) * KB * self.t0 * KAPPA / m)
            noise = sigma * self._gaussians()
            v = self.c1 * v + noise - (m * noise).sum(0) / self.mtot
        x = x + h * v
        self.pos, self.v = x, v
        self.flags |= STARTED
        self.n_steps += 1
        self.c += 1

    def reverse(self) -> None:
        """Turn every velocity round (at a synchronous point: after a finish_only call)."""
        assert not self.flags & STARTED
        self.v = -self.v

    @property
    def variance(self) -> float:
        return self.m2 / (self.count - 1) if self.count > 1 else float("nan")
