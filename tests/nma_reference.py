"""Numpy restatement of the normal-mode family (m3g_nma_*, include/m3gnet_hip.h; torch_m3gnet.normal_modes): one structure, plain
fp64, np.exp phases, the definitions as they are written and none of the device's orders -- so the device is held to it within a
rounding bound, not bitwise.  `NmaReference` mirrors init / sample / the accumulators; `random_case` draws the synthetic structures
the tests share (random unitary E, which need not come from a dynamical matrix)."""
import numpy as np

KAPPA = 9.648533215665e-3   # A/fs^2 per eV/(A amu)
EPS = 2.2e-16


def supercell_cells(supercell) -> np.ndarray:
    """[N_c, 3] cell indices (l1, l2, l3) in the order l = (l1 c2 + l2) c3 + l3."""
    return np.stack(np.meshgrid(*(np.arange(int(n)) for n in supercell), indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float64)


def site_fractions(frac, supercell) -> np.ndarray:
    """f_j = f_b + (l1, l2, l3) of atom j = l n_u + b: [N_s, 3]."""
    return (np.asarray(frac, dtype=np.float64)[None, :, :] + supercell_cells(supercell)[:, None, :]).reshape(-1, 3)


class NmaReference:
    def __init__(self, lattice, frac, masses, supercell, qpoints, eigenvectors, n_lags, remove_com=True):
        self.frac_sites = site_fractions(frac, supercell)
        self.n_u, self.n_cells = len(frac), int(np.prod(supercell))
        self.r0 = self.frac_sites @ np.asarray(lattice, dtype=np.float64)
        self.mass = np.tile(np.asarray(masses, dtype=np.float64), self.n_cells)
        self.q = np.asarray(qpoints, dtype=np.float64).reshape(-1, 3)
        self.e = np.asarray(eigenvectors, dtype=np.complex128)
        self.phase = np.exp(-2j * np.pi * (self.q @ self.frac_sites.T))   # [Q, N_s]
        self.n_lags, self.remove_com = n_lags, remove_com
        shape = (len(self.q), 3 * self.n_u)
        self.n_samples, self.kinetic_sum, self.flags = 0, 0.0, 0
        self.qdot2_sum, self.q2_sum = np.zeros(shape), np.zeros(shape)
        self.acf = np.zeros(shape + (n_lags,), dtype=np.complex128)
        self.lag_count = np.zeros(n_lags, dtype=np.int64)
        self.history = []   # every accepted Qdot
        self.last_qdot, self.last_q = np.zeros(shape, dtype=np.complex128), np.zeros(shape, dtype=np.complex128)
        self.norm_v = self.norm_u = 0.0   # |sqrt(m) v|_2 and |sqrt(m) u|_2 of the last accepted sample, their largest, sums of their squares
        self.max_norm_v = self.max_norm_u = 0.0
        self.norm_v2_sum = self.norm_u2_sum = 0.0

    def project(self, x) -> np.ndarray:
        """[Q, 3 n_u] from per-atom vectors x [N_s, 3]: N_c^(-1/2) sum_j sqrt(m_j) exp(-2 pi i q.f_j) sum_a conj(E[3b+a, nu]) x[j, a]."""
        w = (self.phase[:, :, None] * (np.sqrt(self.mass)[:, None] * x)[None]).reshape(len(self.q), self.n_cells, 3 * self.n_u).sum(1)
        return np.einsum("qrn,qr->qn", self.e.conj(), w) / np.sqrt(self.n_cells)

    def sample(self, pos, vel, forces=None, kick=0.0):
        v = np.array(vel, dtype=np.float64)
        if forces is not None:
            v = v + kick * (KAPPA * np.asarray(forces, dtype=np.float64) / self.mass[:, None])
        u = np.asarray(pos, dtype=np.float64) - self.r0
        if self.flags or not (np.isfinite(v).all() and np.isfinite(u).all()):
            self.flags |= 1
            return
        u = u - (self.mass[:, None] * u).sum(0) / self.mass.sum()
        if self.remove_com:
            v = v - (self.mass[:, None] * v).sum(0) / self.mass.sum()
        qdot, q = self.project(v), self.project(u)
        self.history.append(qdot)
        self.n_samples += 1
        self.kinetic_sum += float((self.mass[:, None] * v * v).sum())
        self.qdot2_sum += np.abs(qdot) ** 2
        self.q2_sum += np.abs(q) ** 2
        for lag in range(min(self.n_lags, self.n_samples)):
            self.acf[:, :, lag] += self.history[-1 - lag].conj() * qdot
            self.lag_count[lag] += 1
        self.last_qdot, self.last_q = qdot, q
        self.norm_v, self.norm_u = float(np.sqrt((self.mass[:, None] * v * v).sum())), float(np.sqrt((self.mass[:, None] * u * u).sum()))
        self.max_norm_v, self.max_norm_u = max(self.max_norm_v, self.norm_v), max(self.max_norm_u, self.norm_u)
        self.norm_v2_sum += self.norm_v ** 2
        self.norm_u2_sum += self.norm_u ** 2


def random_unitary(rng, n: int) -> np.ndarray:
    q, r = np.linalg.qr(rng.normal(size=(n, n)) + 1j * rng.normal(size=(n, n)))
    return q * (np.diag(r) / np.abs(np.diag(r)))[None, :]


def all_qpoints(supercell) -> np.ndarray:
    return supercell_cells(supercell) / np.asarray(supercell, dtype=np.float64)


def random_case(seed: int, n_u: int, supercell, qpoints, n_species: int = 1) -> dict:
    """A synthetic structure: a triclinic unit cell, random sites and masses (`n_species` distinct values), random unitary E per q."""
    rng = np.random.default_rng(seed)
    lattice = 3.0 * np.eye(3) + rng.uniform(-0.4, 0.4, (3, 3))
    frac = rng.uniform(0.0, 1.0, (n_u, 3))
    masses = rng.uniform(10.0, 120.0, n_species)[np.arange(n_u) % n_species]
    q = np.asarray(qpoints, dtype=np.float64).reshape(-1, 3)
    eig = np.stack([random_unitary(rng, 3 * n_u) for _ in q])
    return {"lattice": lattice, "frac": frac, "masses": masses, "supercell": tuple(int(c) for c in supercell), "qpoints": q,
            "eigenvectors": eig, "n_atoms": n_u * int(np.prod(supercell))}


def random_frames(case: dict, seed: int, n_frames: int):
    """`n_frames` of (pos, vel, forces float32): sites plus displacements of 0.05 A (and a small drift of the whole cell), velocities of
    0.01 A/fs with a net momentum, forces of 1 eV/A."""
    rng = np.random.default_rng(seed)
    r0 = site_fractions(case["frac"], case["supercell"]) @ case["lattice"]
    out = []
    for k in range(n_frames):
        pos = r0 + rng.normal(0.0, 0.05, r0.shape) + 0.01 * (k + 1) * np.array([1.0, -2.0, 0.5])
        vel = rng.normal(0.0, 0.01, r0.shape) + np.array([0.003, 0.0, -0.002])
        out.append((pos, vel, rng.normal(0.0, 1.0, r0.shape).astype(np.float32)))
    return out
