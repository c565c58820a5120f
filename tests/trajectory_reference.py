"""Brute-force numpy restatement of the trajectory observables (torch_m3gnet.trajectory, csrc/m3g_trajectory.hip): the yardstick of
tests/test_gpu_trajectory.py and tests/test_trajectory_cpu.py.  One structure at a time, fp64 throughout.

Conventions (the ones of torch_m3gnet/trajectory.py's docstring).  H_ab[k]: UNORDERED pairs i < j of species a <= b (row-major upper
triangle) whose minimum-image distance r < r_max falls in bin int(r * bins / r_max); n samples, <V> = volume_sum / n, v_k the volume
of shell k, N_a atoms of species a, N in all:
    g_ab = <V> H_ab / (n N_a N_b v_k) (a != b),  g_aa = 2 <V> H_aa / (n N_a^2 v_k),  g_total = 2 <V> sum H / (n N^2 v_k),
    coordination[a][b] = running sum of the ordered a -> b pairs (H_ab, or 2 H_aa) / (n N_a).
msd[a][l] / vacf[a][l]: means over the atoms of species a and the samples with a frame l samples back of |r(t+l) - r(t)|^2 and
v(t+l) . v(t); with remove_com every frame first loses its mass-weighted centre-of-mass position and velocity; a sample with forces
stores v + kick * KAPPA * F / m."""
import numpy as np

KAPPA = 9.648533215665e-3   # A/fs^2 per eV/(A amu)
U = 2.0 ** -53              # unit roundoff of fp64


def pair_index(a, b, max_species):
    a, b = min(a, b), max(a, b)
    return sum(max_species - k for k in range(a)) + (b - a)


def perpendicular_widths(lattice):
    L = np.asarray(lattice, dtype=np.float64)
    vol = abs(np.linalg.det(L))
    return np.array([vol / np.linalg.norm(np.cross(L[(k + 1) % 3], L[(k + 2) % 3])) for k in range(3)])


def pair_distances(pos, lattice):
    """(i, j, r) of all pairs i < j: the minimum image by rounding the fractional difference."""
    pos, L = np.asarray(pos, dtype=np.float64), np.asarray(lattice, dtype=np.float64)
    i, j = np.triu_indices(len(pos), k=1)
    frac = pos @ np.linalg.inv(L)
    df = frac[j] - frac[i]
    df -= np.rint(df)
    return i, j, np.linalg.norm(df @ L, axis=1)


def histogram(pos, lattice, species, r_max, bins, max_species):
    """(H [P, bins] uint64, distance of the closest pair distance to a bin edge or to r_max -- the guard of exact comparisons)."""
    P = max_species * (max_species + 1) // 2
    H = np.zeros((P, bins), np.uint64)
    species = np.asarray(species)
    i, j, r = pair_distances(pos, lattice)
    near = np.isfinite(r) & (r < r_max + r_max / bins)
    x = r[near] * bins / r_max
    margin = float(np.abs(x - np.rint(x)).min() * r_max / bins) if near.any() else np.inf
    take = r < r_max   # (a NaN fails it)
    k = np.minimum((r[take] * bins / r_max).astype(np.int64), bins - 1)
    table = np.array([[pair_index(a, b, max_species) for b in range(max_species)] for a in range(max_species)], dtype=np.int64)
    rows = table[species[i[take]], species[j[take]]]
    np.add.at(H, (rows, k), 1)
    return H, margin


def normalise_rdf(H, counts, n_samples, volume_sum, r_max, max_species):
    counts = np.asarray(counts, dtype=np.float64)
    H = np.asarray(H, dtype=np.float64)
    bins = H.shape[1]
    edges = np.arange(bins + 1) * (r_max / bins)
    shell = 4.0 / 3.0 * np.pi * (edges[1:] ** 3 - edges[:-1] ** 3)
    v = volume_sum / n_samples
    n_sp = len(counts)
    g = np.zeros((n_sp, n_sp, bins))
    cn = np.zeros((n_sp, n_sp, bins))
    total = np.zeros(bins)
    for a in range(n_sp):
        for b in range(n_sp):
            h = H[pair_index(a, b, max_species)]
            if a == b:
                g[a, b] = 2.0 * v * h / (n_samples * counts[a] ** 2 * shell)
                cn[a, b] = np.cumsum(2.0 * h) / (n_samples * counts[a])
            else:
                g[a, b] = v * h / (n_samples * counts[a] * counts[b] * shell)
                cn[a, b] = np.cumsum(h) / (n_samples * counts[a])
            if a <= b:
                total += h
    return {"g": g, "coordination": cn, "g_total": 2.0 * v * total / (n_samples * counts.sum() ** 2 * shell)}


class Correlations:
    """Sliding-window MSD / VACF sums of one structure over a list of frames, with a worst-case bound on what fp64 rounding may
    make a different order of the same sums differ by (bound_msd, bound_vacf; n atoms, u = 2^-53):
      * a sum of n terms in another order: n u sum|terms|; a few roundings per term and the additions of the samples: + 32 u sum|terms|;
      * with remove_com each stored coordinate carries the error of the centre of mass, 2 (n + 2) u max|r| for both sides together
        (max|v| for velocities); the kick adds 4 u max|v|.  It enters |dr|^2 as 2 |dr| * 2 eps and v . v' as eps (|v| + |v'|).
    Why the centre-of-mass term is there at all: the sum sum m r runs over UNWRAPPED coordinates, whose size is that of the
    trajectory's offsets, not of the displacements (hundreds of A in the GPU tests), so its order-dependent rounding, n u max|r|, is
    far above n u sum|dr|^2 and does not cancel between two frames.  Without remove_com only the first line applies."""

    def __init__(self, masses, species, max_species, n_lags, remove_com):
        self.m = np.asarray(masses, dtype=np.float64)
        self.species = np.asarray(species)
        self.M, self.G, self.remove_com = max_species, n_lags, remove_com
        self.frames = []
        self.msd, self.vacf = np.zeros((max_species, n_lags)), np.zeros((max_species, n_lags))
        self.bound_msd, self.bound_vacf = np.zeros((max_species, n_lags)), np.zeros((max_species, n_lags))
        self.lag_count = np.zeros(n_lags, np.int64)

    def sample(self, pos, vel, forces=None, kick=0.0):
        r, v = np.array(pos, dtype=np.float64), np.array(vel, dtype=np.float64)
        if forces is not None:
            v = v + kick * (KAPPA * np.asarray(forces).astype(np.float64) / self.m[:, None])
        n = len(self.m)
        eps_r, eps_v = 0.0, 4.0 * U * np.abs(v).max()
        if self.remove_com:
            eps_r = 2.0 * (n + 2) * U * np.abs(r).max()
            eps_v += 2.0 * (n + 2) * U * np.abs(v).max()
            r = r - (self.m[:, None] * r).sum(0) / self.m.sum()
            v = v - (self.m[:, None] * v).sum(0) / self.m.sum()
        self.frames = (self.frames + [(r, v, eps_r, eps_v)])[-self.G:]
        for lag in range(len(self.frames)):
            r0, v0, er0, ev0 = self.frames[-1 - lag]
            dr = r - r0
            for a in range(self.M):
                sel = self.species == a
                sq, dot = (dr[sel] ** 2).sum(), np.abs(v[sel] * v0[sel]).sum()
                self.msd[a, lag] += sq
                self.vacf[a, lag] += (v[sel] * v0[sel]).sum()
                self.bound_msd[a, lag] += (n + 32) * U * sq + 4.0 * max(eps_r, er0) * np.abs(dr[sel]).sum()
                self.bound_vacf[a, lag] += (n + 32) * U * dot + max(eps_v, ev0) * (np.abs(v[sel]).sum() + np.abs(v0[sel]).sum())
            self.lag_count[lag] += 1
        return v


def normalise_correlations(msd_sum, vacf_sum, lag_count, counts):
    norm = np.asarray(counts, dtype=np.float64)[:, None] * np.asarray(lag_count, dtype=np.float64)[None, :]
    return np.asarray(msd_sum) / norm, np.asarray(vacf_sum) / norm
