"""numpy fp64 restatement of batched path-integral molecular dynamics (torch_m3gnet.path_integral / m3g_pimd_*), one ring polymer at a
time: the yardstick of tests/test_pimd_cpu.py and tests/test_gpu_pimd.py.

Units: A, fs, amu, eV; a = KAPPA F / m; HBAR in eV fs.  A ring of P beads of n atoms at target temperature T samples

    H_P = sum_j [KE_j + 1/2 sum_i m_i w_P^2 |q_i,j - q_i,j+1|^2 + V(q_j)],   w_P = P KB T / HBAR,   at temperature P T,

so every bead feels the full force.  Normal modes by the real orthogonal C[j][k] of Ceriotti, Parrinello, Markland, Manolopoulos,
J. Chem. Phys. 133, 124104 (2010) (`mode_matrix`), frequencies w_k = 2 w_P sin(k pi / P).  One `step(forces [P,n,3], finish_only)`
with the forces at `self.pos` does what one m3g_pimd_step call does to this ring (BAOAB, h = dt / 2):

    heat += what the previous call's O step added to the ring kinetic energy
    finish (started):   v += h a
    observables:        KE of all beads, T = 2 KE / (3 n P^2 KB), E_spring, K_prim = 3 n P kT / 2 - E_spring / P,
                        K_cv = 3 n kT / 2 - 1 / (2 P) sum_j sum_i (q_ij - qbar_i) . F_ij, heat, 0, 0
    start (not finish_only; finish_only clears `started` instead):
      B(h)   v += h a
      A(h)   in normal modes: mode 0 x += h v; mode k >= 1 x' = cos(w_k h) x + sin(w_k h) / w_k v, v' = cos(w_k h) v - w_k sin(w_k h) x
      O(dt)  "pile_l" only, in normal modes: v' = c1_k v + c2_k sqrt(P KB T KAPPA / m_i) xi, c1_k = exp(-gamma_k dt), c2_k = sqrt(1 -
             c1_k^2), gamma_0 = centroid_friction, gamma_k = 2 pile_lambda w_k; xi from Philox4x64-10, key (seed, 3), counter
             (n_steps, atom, k, 0), the Box-Muller of md_reference.gaussians
      A(h)   and back to beads
A non-finite force on any bead: flagged ERROR, the whole ring frozen from then on."""
from __future__ import annotations

import numpy as np

from md_reference import ERROR, KAPPA, KB, STARTED, philox4x64_10

HBAR = 0.6582119569   # eV fs
THERMOSTATS = {"none": 0, "pile_l": 1}
NOISE_BLOCKS = 1 << 16   # Philox blocks drawn at a time: the starts ahead that fit (numpy's overhead per call, not the numbers)


def mode_matrix(P: int) -> np.ndarray:
    """C [P, P]: x_mode[k] = sum_j C[j, k] x_bead[j]."""
    j, k = np.meshgrid(np.arange(P), np.arange(P), indexing="ij")
    arg = 2.0 * np.pi * ((j * k) % P).astype(np.float64) / P
    c = np.where(2 * k < P, np.sqrt(2.0 / P) * np.cos(arg), np.sqrt(2.0 / P) * np.sin(arg))
    c = np.where(2 * k == P, np.sqrt(1.0 / P) * np.where(j % 2 == 1, -1.0, 1.0), c)
    return np.where(k == 0, np.sqrt(1.0 / P), c)


def mode_frequencies(P: int, temperature: float) -> np.ndarray:
    """w_k [P] (1/fs) of a ring of P beads at `temperature` (K)."""
    return 2.0 * (P * KB * temperature / HBAR) * np.sin(np.arange(P) * np.pi / P)


def mode_gaussians(seed: int, steps, n: int, P: int) -> np.ndarray:
    """[len(steps), P, n, 3] standard normals of the P modes of the n atoms of a ring seeded `seed` at its starts number `steps`."""
    steps = np.asarray(steps, dtype=np.uint64).reshape(-1)
    ctr = np.zeros((len(steps), P, n, 4), dtype=np.uint64)
    ctr[..., 0] = steps[:, None, None]
    ctr[..., 1] = np.arange(n, dtype=np.uint64)[None, None, :]
    ctr[..., 2] = np.arange(P, dtype=np.uint64)[None, :, None]
    w = philox4x64_10(ctr, np.array([seed, 3], dtype=np.uint64))
    u = ((w >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53
    r0, r1 = np.sqrt(-2.0 * np.log(u[..., 0])), np.sqrt(-2.0 * np.log(u[..., 2]))
    two_pi = 6.283185307179586
    return np.stack([r0 * np.cos(two_pi * u[..., 1]), r0 * np.sin(two_pi * u[..., 1]), r1 * np.cos(two_pi * u[..., 3])], axis=-1)


class PimdReference:
    """One ring: `pos` [P,n,3] (unwrapped), `masses` [n] amu, `vel` [P,n,3] A/fs."""

    def __init__(self, pos, masses, vel, temperature, seed=0, thermostat="pile_l", dt=0.5, centroid_friction=0.01, pile_lambda=0.5):
        self.pos = np.array(pos, dtype=np.float64)
        self.v = np.array(vel, dtype=np.float64)
        self.m = np.array(masses, dtype=np.float64).reshape(-1)
        self.P, self.n = self.pos.shape[0], len(self.m)
        assert self.pos.shape == self.v.shape == (self.P, self.n, 3) and thermostat in THERMOSTATS
        self.thermostat, self.t0, self.seed, self.dt = thermostat, float(temperature), int(seed), float(dt)
        P, h = self.P, 0.5 * self.dt
        self.C = mode_matrix(P)
        self.w = mode_frequencies(P, self.t0)
        w = self.w
        gamma = np.concatenate([[centroid_friction], 2.0 * pile_lambda * w[1:]])
        self.cs, self.ws = np.cos(w * h), w * np.sin(w * h)
        self.sw = np.concatenate([[h], np.sin(w[1:] * h) / w[1:]])
        self.c1 = np.exp(-gamma * self.dt)
        self.c2 = np.sqrt(1.0 - self.c1 * self.c1)
        self.flags, self.n_steps = 0, 0
        self.heat, self.pending = 0.0, 0.0
        self.obs = np.full(8, np.nan)
        self._noise, self._noise_from = None, 0

    def _gaussians(self):
        k = self.n_steps - self._noise_from
        if self._noise is None or not 0 <= k < len(self._noise):
            self._noise_from, k = self.n_steps, 0
            ahead = max(1, NOISE_BLOCKS // (self.P * self.n))
            self._noise = mode_gaussians(self.seed, self.n_steps + np.arange(ahead), self.n, self.P)
        return self._noise[k]

    def _modes(self, C, a):
        """sum_j C[j, k] a[j] for a [P,n,3]."""
        return (C.T @ a.reshape(self.P, -1)).reshape(a.shape)

    def _free_ring(self, x, v):
        """A(h) on normal-mode coordinates [P,n,3]."""
        cs, sw, ws = (a[:, None, None] for a in (self.cs, self.sw, self.ws))
        x1, v1 = cs * x + sw * v, cs * v - ws * x
        x1[0], v1[0] = x[0] + 0.5 * self.dt * v[0], v[0]
        return x1, v1

    def step(self, forces, finish_only: bool = False) -> None:
        if self.flags & ERROR:
            return
        f = np.asarray(forces, dtype=np.float64).reshape(self.P, self.n, 3)
        if not np.isfinite(f).all():
            self.flags |= ERROR
            return
        P, n, h, m = self.P, self.n, 0.5 * self.dt, self.m[None, :, None]
        self.heat += self.pending
        self.pending = 0.0
        a = KAPPA * f / m
        v = self.v + h * a if self.flags & STARTED else self.v.copy()
        kt = KB * self.t0
        wp = P * kt / HBAR
        ke = (m * v * v).sum() / (2.0 * KAPPA)
        bonds = self.pos - np.roll(self.pos, -1, axis=0)
        spring = wp * wp * (m * bonds * bonds).sum() / (2.0 * KAPPA)
        centroid = self.pos.mean(0)
        self.obs = np.array([ke, 2.0 * ke / (3.0 * n * P * P * KB), spring, 1.5 * n * P * kt - spring / P,
                             1.5 * n * kt - ((self.pos - centroid[None]) * f).sum() / (2.0 * P), self.heat, 0.0, 0.0])
        if finish_only:
            self.v = v
            self.flags &= ~STARTED
            return
        v = v + h * a
        x, v = self._modes(self.C, self.pos), self._modes(self.C, v)
        x, v = self._free_ring(x, v)
        if self.thermostat == "pile_l":
            xi = self._gaussians()
            v1 = self.c1[:, None, None] * v + self.c2[:, None, None] * np.sqrt(P * kt * KAPPA / m) * xi
            self.pending = (m * (v1 * v1 - v * v)).sum() / (2.0 * KAPPA)
            v = v1
        x, v = self._free_ring(x, v)
        self.pos, self.v = self._modes(self.C.T, x), self._modes(self.C.T, v)
        self.flags |= STARTED
        self.n_steps += 1

    def reverse(self) -> None:
        """Turn every velocity round (at a synchronous point: after a finish_only call)."""
        assert not self.flags & STARTED
        self.v = -self.v
