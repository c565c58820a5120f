"""Numpy restatement of the scattering family (m3g_sq_*, include/m3gnet_hip.h; torch_m3gnet.scattering): one structure, plain loops
over samples, written from the conventions and not from the kernel.  Every function takes the floating type it computes in
(`np.float64` or `np.longdouble`), so the GPU test can measure the reference's own rounding by running it twice.

Conventions.  Cell L (rows = lattice vectors); Miller triple h != 0; q = 2 pi h L^-T, so q . r = 2 pi h . f with f = r L^-1.  Per
species a: rho_a(q) = sum_{j in a} exp(-i q . r_j), j_a(q) = sum_{j in a} v_j exp(-i q . r_j), j_L = qhat . j, j_T = j - qhat j_L.
v = vel, or vel + kick KAPPA F / m with forces; with remove_com r and v are relative to the mass-weighted centre of mass.  Phases:
f is reduced to f - rint(f) before h . f is formed, h . f is reduced again, and cos / sin only see 2 pi times a number in
[-1/2, 1/2].  Accumulated per q, pair a <= b (row-major upper triangle, `pair_index`) and lag l over a ring of the last n_lags samples:
    F  += Re[rho_a(t) rho_b*(t-l) + rho_b(t) rho_a*(t-l)] / 2
    CL += the same of j_L
    CT += 1/2 Re[j_T,a(t) . j_T,b*(t-l) + j_T,b(t) . j_T,a*(t-l)] / 2
with lag_count[l] the number of samples that had a frame l samples back."""
import numpy as np

KAPPA = 9.648533215665e-3   # A/fs^2 per eV/(A amu)


def pair_index(a, b, max_species):
    a, b = min(a, b), max(a, b)
    return a * max_species - a * (a - 1) // 2 + (b - a)


def pi(dtype):
    return dtype(4) * np.arctan(dtype(1))


def inverse(L, dtype):
    """L^-1 from the adjugate, in `dtype` (numpy.linalg has no long double)."""
    L = np.asarray(L, dtype=dtype)
    c = np.stack([np.cross(L[1], L[2]), np.cross(L[2], L[0]), np.cross(L[0], L[1])])   # rows: a1 x a2, a2 x a0, a0 x a1
    return (c / (L[0] @ c[0])).T   # f_k = r . c_k / det


def fractional(r, lattice, dtype, reverse=False):
    """f = r L^-1; `reverse`: as (r . c_k) / det, the division last -- the same numbers through other roundings."""
    if not reverse:
        return r @ inverse(lattice, dtype)
    L = np.asarray(lattice, dtype=dtype)
    c = np.stack([np.cross(L[1], L[2]), np.cross(L[2], L[0]), np.cross(L[0], L[1])])
    return (r @ c.T) / (L[0] @ c[0])


def cartesian_q(lattice, hkl, dtype=np.float64):
    return 2 * pi(dtype) * np.asarray(hkl, dtype=dtype).reshape(-1, 3) @ inverse(lattice, dtype).T


def entries(pos, vel, lattice, species, masses, hkl, max_species, remove_com, dtype=np.float64, forces=None, kick=0.0, reverse=False):
    """(rho [Q, M], j_L [Q, M], j_T [Q, M, 3]) complex of one frame; `reverse`: the rows summed in the opposite order and the fractional
    coordinates formed with the division last (another equally valid evaluation, for the margin of the GPU test)."""
    r, v, m = np.asarray(pos, dtype=dtype), np.asarray(vel, dtype=dtype), np.asarray(masses, dtype=dtype)
    species, hkl = np.asarray(species), np.asarray(hkl).reshape(-1, 3)
    if forces is not None:
        v = v + dtype(kick) * (dtype(KAPPA) * np.asarray(forces).astype(dtype) / m[:, None])
    if remove_com:
        r = r - (m[:, None] * r).sum(axis=0) / m.sum()
        v = v - (m[:, None] * v).sum(axis=0) / m.sum()
    f = fractional(r, lattice, dtype, reverse)
    f = f - np.rint(f)
    phase = hkl.astype(dtype) @ f.T   # [Q, n]
    phase = phase - np.rint(phase)
    w = np.cos(2 * pi(dtype) * phase) - 1j * np.sin(2 * pi(dtype) * phase)   # exp(-i q . r)
    rows = np.arange(len(r))[::-1] if reverse else np.arange(len(r))
    Q = len(hkl)
    rho = np.zeros((Q, max_species), dtype=w.dtype)
    j = np.zeros((Q, max_species, 3), dtype=w.dtype)
    for i in rows:   # (a plain loop: the order of the sum is the stated one)
        rho[:, species[i]] += w[:, i]
        j[:, species[i]] += w[:, i, None] * v[i][None, :]
    q = cartesian_q(lattice, hkl, dtype)
    qhat = q / np.sqrt((q * q).sum(axis=1))[:, None]
    jl = (j * qhat[:, None, :]).sum(axis=2)
    jt = j - qhat[:, None, :] * jl[:, :, None]
    return rho, jl, jt


def rounding_units(vel, species, masses, max_species, forces=None, kick=0.0):
    """([M], [M]): 2^-53 times the summed moduli of the terms of rho_a (the number of rows) and of j_a (sum |v_j|, before the centre of
    mass is removed: its subtraction rounds at the size of v itself).  The size below which an entry is rounding and nothing else."""
    v = np.asarray(vel, dtype=np.float64)
    if forces is not None:
        v = v + kick * (KAPPA * np.asarray(forces).astype(np.float64) / np.asarray(masses)[:, None])
    speed = np.sqrt((v * v).sum(axis=1))
    return (np.bincount(species, minlength=max_species) * 2.0 ** -53, np.bincount(species, weights=speed, minlength=max_species) * 2.0 ** -53)


class Accumulator:
    """The ring and the sums of one structure."""

    def __init__(self, species, masses, hkl, max_species, n_lags, remove_com, dtype=np.float64, reverse=False):
        self.species, self.masses, self.hkl = np.asarray(species), np.asarray(masses), np.asarray(hkl).reshape(-1, 3)
        self.M, self.G, self.remove_com, self.dtype, self.reverse = max_species, n_lags, remove_com, dtype, reverse
        Q, P = len(self.hkl), max_species * (max_species + 1) // 2
        self.f, self.cl, self.ct = (np.zeros((Q, P, n_lags), dtype=dtype) for _ in range(3))
        self.f_scale, self.cl_scale, self.ct_scale = (np.zeros((Q, P, n_lags), dtype=np.float64) for _ in range(3))
        self.f_floor, self.cl_floor, self.ct_floor = (np.zeros((Q, P, n_lags), dtype=np.float64) for _ in range(3))
        self.lag_count = np.zeros(n_lags, dtype=np.int64)
        self.frames, self.units = [], []   # newest last

    def sample(self, pos, vel, lattice, forces=None, kick=0.0):
        self.frames.append(entries(pos, vel, lattice, self.species, self.masses, self.hkl, self.M, self.remove_com, self.dtype, forces, kick,
                                   self.reverse))
        self.units.append(rounding_units(vel, self.species, self.masses, self.M, forces, kick))
        self.frames, self.units = self.frames[-self.G:], self.units[-self.G:]
        rho, jl, jt = self.frames[-1]
        ur, uj = self.units[-1]
        for lag in range(len(self.frames)):
            rho0, jl0, jt0 = self.frames[-1 - lag]
            ur0, uj0 = self.units[-1 - lag]
            self.lag_count[lag] += 1
            for a in range(self.M):
                for b in range(a, self.M):
                    p = pair_index(a, b, self.M)
                    self.f[:, p, lag] += (rho[:, a] * np.conj(rho0[:, b]) + rho[:, b] * np.conj(rho0[:, a])).real / 2
                    self.cl[:, p, lag] += (jl[:, a] * np.conj(jl0[:, b]) + jl[:, b] * np.conj(jl0[:, a])).real / 2
                    self.ct[:, p, lag] += ((jt[:, a] * np.conj(jt0[:, b])).sum(axis=1) + (jt[:, b] * np.conj(jt0[:, a])).sum(axis=1)).real / 4
                    # What a deviation of the sum is measured against: the products of the moduli behind every term (*_scale),
                    # and beside them (*_floor) what one rounding unit in each factor moves the term by, u_x |y| + u_y |x| + u_x u_y
                    # (rounding_units, four units each): a factor that is rounding and nothing else -- the velocity of a single
                    # atom seen from its own centre of mass -- has no relative accuracy to be held to.
                    for name, x, y, u, u0, vector in (("f", rho, rho0, ur, ur0, False), ("cl", jl, jl0, uj, uj0, False), ("ct", jt, jt0, uj, uj0, True)):
                        mod = (lambda z: np.sqrt((np.abs(z) ** 2).sum(axis=1)).astype(np.float64)) if vector else (lambda z: np.abs(z).astype(np.float64))
                        xa, xb, ya, yb = mod(x[:, a]), mod(x[:, b]), mod(y[:, a]), mod(y[:, b])
                        half = 4 if vector else 2
                        getattr(self, name + "_scale")[:, p, lag] += (xa * yb + xb * ya) / half
                        getattr(self, name + "_floor")[:, p, lag] += (4 * u[a] * yb + 4 * u0[b] * xa + 16 * u[a] * u0[b] +
                                                                      4 * u[b] * ya + 4 * u0[a] * xb + 16 * u[b] * u0[a]) / half


def static_structure_factor(frames_rho, n_atoms):
    """S(q) = < |sum_a rho_a(q)|^2 > / N over the given densities [n_frames][Q, M]."""
    total = [np.asarray(r).sum(axis=1) for r in frames_rho]
    return np.mean([t.real * t.real + t.imag * t.imag for t in total], axis=0) / n_atoms


def lattice_bound(n_atoms, hkl, max_shift):
    """|rho(h) - exact| at most, for atoms ON lattice sites shifted by up to `max_shift` lattice vectors: a fractional coordinate of
    modulus <= max_shift + 1 comes out of three products, two sums and a division (and carries the rounding of the position itself),
    8 roundings at most, so it is off by <= 8 (max_shift + 1) 2^-53; the phase 2 pi h . f by |h|_1 times that; each of the n_atoms unit
    terms by its phase error (|exp(ix) - exp(iy)| <= |x - y|), by 4 x 2^-53 for cos and sin themselves (2 ulp each), and the running
    sum of modulus <= n_atoms rounds n_atoms times."""
    h1 = np.abs(np.asarray(hkl)).sum(axis=1)
    return n_atoms * (2 * np.pi * h1 * 8 * (max_shift + 1) + 4 + n_atoms) * 2.0 ** -53
