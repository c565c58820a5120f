"""The thermodynamic fluctuation observables (torch_m3gnet.thermo, C ABI m3g_thermo_*) restated in numpy, generic over the floating
type (float64, longdouble): the formation of the row and of the tensor from either source of the kinetic part, the Welford update of
the mean and the 66 co-moments, the ring with its lag sums, and the skip rule -- include/m3gnet_hip.h states each of them, and this
file follows its words, not the kernels'.  `reverse` sums every sum backwards (a second, equally valid evaluation).  Beside every
row and tensor the sum of the absolute values of the terms it is made of is kept (`scale_x`, `scale_u`): the magnitude against which a
rounding error of that entry is measured (tests/thermo_cases.py)."""
import numpy as np

ROW, COMOMENTS, TENSOR = 11, 66, 7
NONFINITE = 1
KAPPA = 9.648533215665e-3   # A/fs^2 per eV/(A amu)
VOIGT = ((0, 0), (1, 1), (2, 2), (1, 2), (2, 0), (0, 1))
TRIU = tuple((i, j) for i in range(ROW) for j in range(i, ROW))   # row-major upper triangle: (i, j) at i * 11 - i (i - 1) / 2 + (j - i)
TRIU_I, TRIU_J = np.array([i for i, _ in TRIU]), np.array([j for _, j in TRIU])


def _sum(terms, reverse):
    terms = np.asarray(terms)
    return (terms[::-1] if reverse else terms).sum()


def det_terms(L):
    return (L[0, 0] * (L[1, 1] * L[2, 2] - L[1, 2] * L[2, 1]), -L[0, 1] * (L[1, 0] * L[2, 2] - L[1, 2] * L[2, 0]),
            L[0, 2] * (L[1, 0] * L[2, 1] - L[1, 1] * L[2, 0]))


def volume(L):
    a, b, c = det_terms(L)
    return abs(a + b + c)


def inverse(L):
    """From the adjugate over the determinant, as the init call forms it."""
    a, b, c = det_terms(L)
    det = a + b + c
    adj = np.array([[L[1, 1] * L[2, 2] - L[1, 2] * L[2, 1], L[0, 2] * L[2, 1] - L[0, 1] * L[2, 2], L[0, 1] * L[1, 2] - L[0, 2] * L[1, 1]],
                    [L[1, 2] * L[2, 0] - L[1, 0] * L[2, 2], L[0, 0] * L[2, 2] - L[0, 2] * L[2, 0], L[0, 2] * L[1, 0] - L[0, 0] * L[1, 2]],
                    [L[1, 0] * L[2, 1] - L[1, 1] * L[2, 0], L[0, 1] * L[2, 0] - L[0, 0] * L[2, 1], L[0, 0] * L[1, 1] - L[0, 1] * L[1, 0]]],
                   dtype=L.dtype)
    return adj / det


def strain(L, ref_inv, reverse=False):
    """(eps [6], scale [6]): the Green-Lagrange strain (A A^T - 1) / 2, A = L0^-1 L, in the order xx, yy, zz, yz, zx, xy."""
    dtype = L.dtype
    A = np.array([[_sum([ref_inv[i, k] * L[k, j] for k in range(3)], reverse) for j in range(3)] for i in range(3)], dtype=dtype)
    eps, scale = [], []
    for i, j in VOIGT:
        dot = _sum([A[i, k] * A[j, k] for k in range(3)], reverse)
        eps.append((dot - 1) / 2 if i == j else dot / 2)
        scale.append(float(sum(abs(A[i, k] * A[j, k]) for k in range(3)) + (1 if i == j else 0)) / 2)
    return np.array(eps, dtype=dtype), np.array(scale)


def kinetic_tensor(mass, vel, forces, kick, remove_com, dtype, reverse=False):
    """(K [6] in eV, scale [6], any non-finite velocity) from the rows of one structure: v = vel + kick kappa F / m where forces are
    given, R_c = sum (m v_a) v_b, and with remove_com minus Q_a Q_b / M."""
    m, v = np.asarray(mass, dtype=dtype), np.asarray(vel, dtype=dtype)
    if forces is not None:
        v = v + dtype(kick) * (dtype(KAPPA) * np.asarray(forces, dtype=dtype) / m[:, None])
    mv = m[:, None] * v
    K, scale = [], []
    M = _sum(m, reverse)
    Q = [_sum(mv[:, a], reverse) for a in range(3)]
    for a, b in VOIGT:
        R = _sum(mv[:, a] * v[:, b], reverse)
        big = float(np.abs(mv[:, a] * v[:, b]).astype(np.float64).sum())
        if remove_com:
            R = R - Q[a] * Q[b] / M
            big += float(abs(Q[a] * Q[b] / M))
        K.append(R / dtype(KAPPA))
        scale.append(big / KAPPA)
    return np.array(K, dtype=dtype), np.array(scale), not bool(np.isfinite(v.astype(np.float64)).all())


class Accumulator:
    """One structure: what the device keeps for it, and every row and tensor it was fed (`rows`, `tensors`, `skipped`)."""

    def __init__(self, mass, p_ext, reference_cell, n_lags, remove_com, dtype, reverse=False):
        self.dtype, self.reverse = dtype, reverse
        self.mass, self.p_ext = np.asarray(mass, dtype=np.float64), dtype(p_ext)
        self.ref_inv = inverse(np.asarray(reference_cell, dtype=dtype))
        self.G, self.remove_com = int(n_lags), bool(remove_com)
        self.n_samples = self.n_skipped = self.flags = 0
        self.mean, self.comoments = np.zeros(ROW, dtype), np.zeros(COMOMENTS, dtype)
        self.lag_uu, self.lag_now, self.lag_old = (np.zeros((self.G, TENSOR), dtype) for _ in range(3))
        self.lag_count = np.zeros(self.G, np.int64)
        self.ring = []   # the newest entry last
        self.rows, self.tensors, self.scale_x, self.scale_u, self.skipped = [], [], [], [], []

    def form(self, energy, stress, lattice, vel=None, forces=None, kick=0.0, kinetic=None, tensor=None):
        """(x, u or None, scale_x, scale_u, bad) of one sample; energy and stress are float32 values, the rest float64."""
        dtype = self.dtype
        L = np.asarray(lattice, dtype=dtype)
        sv = np.asarray(stress, dtype=np.float32).astype(dtype)
        e_pot = dtype(np.float32(energy))
        det = det_terms(L)
        vol, vol_scale = volume(L), float(sum(abs(t) for t in det))
        bad, u, scale_u = False, None, None
        if (vel is None) == (kinetic is None):
            raise ValueError("exactly one of vel and kinetic")
        if vel is not None:
            K, k_scale, bad = kinetic_tensor(self.mass, vel, forces, kick, self.remove_com, dtype, self.reverse)
            ke, ke_scale = ((K[0] + K[1]) + K[2]) / 2, float(k_scale[:3].sum()) / 2
            P = sv + K / vol
            p, p_scale = ((P[0] + P[1]) + P[2]) / 3, float(np.abs(sv[:3]).sum()) / 3 + 2 * ke_scale / (3 * float(vol))
            u, scale_u = np.concatenate([P, [p]]), np.concatenate([np.abs(sv).astype(np.float64) + k_scale / float(vol), [p_scale]])
        else:
            ke = dtype(kinetic)
            ke_scale = abs(float(ke))
            if tensor is not None:
                P = np.asarray(tensor, dtype=dtype)
                p, p_scale = ((P[0] + P[1]) + P[2]) / 3, float(np.abs(P[:3]).sum()) / 3
                u, scale_u = np.concatenate([P, [p]]), np.concatenate([np.abs(P).astype(np.float64), [p_scale]])
            else:
                trw = vol * ((sv[0] + sv[1]) + sv[2])
                p, p_scale = (trw + 2 * ke) / (3 * vol), float(np.abs(sv[:3]).sum()) / 3 + 2 * ke_scale / (3 * float(vol))
        eps, eps_scale = strain(L, self.ref_inv, self.reverse)
        h = (e_pot + ke) + self.p_ext * vol
        x = np.concatenate([[e_pot, ke, vol, h, p], eps]).astype(dtype)
        scale_x = np.concatenate([[abs(float(e_pot)), ke_scale, vol_scale, abs(float(e_pot)) + ke_scale + abs(float(self.p_ext)) * vol_scale,
                                   p_scale], eps_scale])
        bad = bad or not np.isfinite(x.astype(np.float64)).all() or (u is not None and not np.isfinite(u.astype(np.float64)).all())
        return x, u, scale_x, scale_u, bad

    def sample(self, *args, **kwargs):
        x, u, scale_x, scale_u, bad = self.form(*args, **kwargs)
        if self.G > 0 and u is None:
            raise ValueError("n_lags > 0 needs the pressure tensor")
        self.rows.append(x), self.tensors.append(u), self.scale_x.append(scale_x), self.scale_u.append(scale_u), self.skipped.append(bad)
        if bad:   # enters nothing; no lag may span the gap
            self.flags |= NONFINITE
            self.n_skipped += 1
            self.ring = []
            return
        n = self.n_samples + 1
        d = x - self.mean
        self.mean = self.mean + d / self.dtype(n)
        e = x - self.mean
        self.comoments = self.comoments + d[TRIU_I] * e[TRIU_J]
        self.n_samples = n
        if self.G > 0:
            self.ring = (self.ring + [u])[-self.G:]
            for lag in range(len(self.ring)):
                old = self.ring[-1 - lag]
                self.lag_uu[lag] += u * old
                self.lag_now[lag] += u
                self.lag_old[lag] += old
                self.lag_count[lag] += 1

    def ring_entry(self, lag):
        """The tensor `lag` samples back, NaN where the ring holds no such entry."""
        return self.ring[-1 - lag] if lag < len(self.ring) else np.full(TENSOR, np.nan)


def welford(rows, dtype=np.float64):
    """(mean, co-moments [66], n) of the rows by the recursion of the header alone (the host side of the MD tests)."""
    mean, co = np.zeros(ROW, dtype), np.zeros(COMOMENTS, dtype)
    for n, x in enumerate(np.asarray(rows, dtype=dtype), 1):
        d = x - mean
        mean = mean + d / dtype(n)
        e = x - mean
        co = co + d[TRIU_I] * e[TRIU_J]
    return mean, co, len(rows)
