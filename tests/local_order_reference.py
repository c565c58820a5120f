"""The local-order observables (torch_m3gnet.local_order, C ABI m3g_lo_*) restated in numpy, generic over the floating type (float64,
longdouble), independent of the device code: neighbours by brute force over the 27 images of the wrapped positions (no rint), its
own spherical harmonics, clusters by union-find.

Definitions.  Atom j != i is a neighbour of i when the minimum-image distance r_ij < r_cut (strict; all species count); N_b(i) is
their number.  Y_lm(rhat): orthonormal on the sphere, Condon-Shortley phase; only m = 0 .. l is kept, Y_l,-m = (-1)^m Y_lm*.
    q_lm(i)    = 1/N_b sum_{j in nb(i)} Y_lm(rhat_ij)  (j ascending)     q_l = sqrt(4 pi/(2l+1) (|q_l0|^2 + 2 sum_{m>0} |q_lm|^2))
    N_b = 0: q_lm = 0, q_l = 0
    qbar_lm(i) = (q_lm(i) + sum_{j in nb(i)} q_lm(j)) / (N_b(i) + 1)     qbar_l from qbar_lm likewise
    Q_lm       = sum_i N_b(i) q_lm(i) / sum_i N_b(i)                     Q_l likewise; 0 when the structure has no bond
    s_ij       = Re sum_{m=-L..L} q_Lm(i) q_Lm*(j) / (|q_L(i)| |q_L(j)|), |q_L(i)|^2 = sum_m |q_Lm(i)|^2, L = solid_degree
    the bond is connected when s_ij > solid_threshold (a zero norm: not connected); n_conn(i) counts them; atom i is solid-like when
    n_conn(i) >= solid_bonds; solid-like neighbours share a cluster, labelled by its smallest atom index; non-solid atoms carry -1.
Flags: CELL 1 (|det| < 1e-12 or a non-finite cell), RANGE 2 (r_cut > half the smallest perpendicular width, allowance 1 + 1e-12),
NEIGHBORS 4 (an atom with more than 32 neighbours), NONFINITE 8 (a non-finite distance, or r = 0).  A flagged sample enters no
histogram, sum or series row."""
import math

import numpy as np

CELL, RANGE, NEIGHBORS, NONFINITE = 1, 2, 4, 8
MAX_NEIGHBORS = 32
ORDERS = 13
IMAGES = np.array([[a, b, c] for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)])


def complex_of(dtype):
    return np.result_type(dtype, np.complex64)


def pi_of(dtype):
    return 4 * np.arctan(dtype(1))


def half_width(lattice):
    """Half the smallest perpendicular width of the cell (rows = lattice vectors)."""
    L = np.asarray(lattice, dtype=np.float64)
    cross = np.array([np.cross(L[(k + 1) % 3], L[(k + 2) % 3]) for k in range(3)])
    return 0.5 * abs(np.linalg.det(L)) / np.linalg.norm(cross, axis=1).max()


def cell_flags(lattice, r_cut):
    L = np.asarray(lattice, dtype=np.float64)
    if not np.isfinite(L).all() or not abs(np.linalg.det(L)) >= 1e-12:
        return CELL
    return 0 if r_cut <= half_width(L) * (1 + 1e-12) else RANGE


def bonds(pos, lattice, r_cut, dtype=np.longdouble, block=32):
    """Per atom (j ascending [N_b], unit vectors [N_b, 3], the smallest |r - r_cut| / r_cut over every image pair, any r == 0): the
    positions wrapped into the cell, then every one of the 27 neighbouring images tried; the nearest image decides."""
    L = np.asarray(lattice, dtype=dtype)
    inv = np.linalg.inv(np.asarray(lattice, dtype=np.float64)).astype(dtype)
    inv = inv @ (2 * np.eye(3, dtype=dtype) - L @ inv)   # one Newton step in `dtype`: the inverse to its precision
    f = np.asarray(pos, dtype=dtype) @ inv
    f = f - np.floor(f)
    n = len(f)
    shifts = IMAGES.astype(dtype) @ L   # [27, 3]
    cart = f @ L
    index, unit, guard, zero = [], [], np.inf, False
    for lo in range(0, n, block):
        hi = min(lo + block, n)
        d = cart[None, :, None, :] - cart[lo:hi, None, None, :] + shifts[None, None, :, :]   # [b, n, 27, 3]
        r = np.sqrt((d * d).sum(axis=-1))
        own = np.arange(lo, hi)
        r[own - lo, own, :] = np.inf   # images of the atom itself are no neighbours
        guard = min(guard, float(np.abs(r / dtype(r_cut) - 1).min()))
        zero = zero or bool((r == 0).any())
        best = r.argmin(axis=-1)
        rmin = np.take_along_axis(r, best[..., None], axis=-1)[..., 0]
        for a in range(hi - lo):
            js = np.nonzero(rmin[a] < dtype(r_cut))[0]
            index.append(js)
            unit.append(d[a, js, best[a, js]] / rmin[a, js][:, None])
    return index, unit, guard, zero


def ylm(l, unit, dtype=np.longdouble, route="cartesian"):
    """Y_lm of unit vectors [n, 3] for m = 0 .. l: [n, l + 1] complex.  route "cartesian": (x + i y)^m times P_l^m(z) / sin^m by its
    upward recurrence; "polar": sin = sqrt(x^2 + y^2), exp(i phi) = (x + i y) / sin, P_l^m(z) itself upward from P_m^m = (-1)^m (2m-1)!!
    sin^m, exp(i m phi) by powers -- another order of the same roundings."""
    u = np.asarray(unit, dtype=dtype).reshape(-1, 3)
    x, y, z = u[:, 0], u[:, 1], u[:, 2]
    out = np.zeros((len(u), l + 1), dtype=complex_of(dtype))
    four_pi = 4 * pi_of(dtype)
    if route == "polar":
        s = np.sqrt(x * x + y * y)
        safe = np.where(s > 0, s, dtype(1))
        phase = np.where(s > 0, (x + 1j * y) / safe, 1 + 0j).astype(out.dtype)
    for m in range(l + 1):
        dfact = dtype(1)
        for k in range(1, 2 * m, 2):
            dfact = dfact * k
        pmm = (-1) ** m * dfact
        if route == "polar":
            pmm = pmm * s ** m
        prev, p = None, pmm + 0 * z
        for ll in range(m + 1, l + 1):
            nxt = ((2 * ll - 1) * z * p - (ll + m - 1) * (prev if prev is not None else 0 * z)) / dtype(ll - m)
            prev, p = p, nxt
        ratio = dtype(math.factorial(l - m)) / dtype(math.factorial(l + m))
        norm = np.sqrt(dtype(2 * l + 1) / four_pi * ratio)
        out[:, m] = norm * p * ((x + 1j * y) ** m if route == "cartesian" else phase ** m)
    return out


def invariant(qlm, l, dtype):
    """sqrt(4 pi/(2l+1) sum_m |q_lm|^2) from the m >= 0 half [..., l + 1]."""
    power = np.abs(qlm[..., 0]) ** 2 + 2 * (np.abs(qlm[..., 1:]) ** 2).sum(axis=-1)
    return np.sqrt(4 * pi_of(dtype) / dtype(2 * l + 1) * power)


def clusters(n, index, solid):
    """Labels [n] by union-find over the solid-solid bonds: the smallest index of the cluster, -1 for non-solid atoms."""
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for i in range(n):
        if solid[i]:
            for j in index[i]:
                if solid[j]:
                    a, b = find(i), find(int(j))
                    if a != b:
                        parent[max(a, b)] = min(a, b)
    return np.array([find(i) if solid[i] else -1 for i in range(n)], dtype=np.int64)


def frame(pos, lattice, r_cut, degrees, solid_degree, solid_threshold, solid_bonds, dtype=np.longdouble, reverse=False, route="cartesian"):
    """Everything of one structure in one frame, as a dict: flags, n_neighbors, and unless a flag is raised qlm [n, D, 13] complex (zero
    beyond l), ql, qbar [n, D], s (one array of s_ij per atom), n_conn, solid, label, n_solid, n_clusters, largest_cluster, Q,
    mean_qbar [D], and the guards `r_guard` (relative, to r_cut) and `s_guard` (to the threshold).  reverse: every sum over neighbours
    runs backwards."""
    pos = np.asarray(pos)
    n, D = len(pos), len(degrees)
    flags = cell_flags(lattice, r_cut)
    if not np.isfinite(pos).all():
        flags |= NONFINITE
    if flags & (CELL | NONFINITE):
        return dict(flags=flags)
    index, unit, r_guard, zero = bonds(pos, lattice, r_cut, dtype)
    nb = np.array([len(js) for js in index], dtype=np.int64)
    flags |= (NONFINITE if zero else 0) | (NEIGHBORS if nb.max() > MAX_NEIGHBORS else 0)
    out = dict(flags=flags, n_neighbors=nb, r_guard=r_guard)
    if flags:
        return out
    ctype = complex_of(dtype)
    start = np.concatenate([[0], np.cumsum(nb)])[:-1]          # the first bond of every atom in the flat bond arrays
    owner, other = np.repeat(np.arange(n), nb), np.concatenate(index) if nb.sum() else np.zeros(0, np.int64)
    flat = np.concatenate(unit) if nb.sum() else np.zeros((0, 3), dtype)

    def rank(k):
        """(atoms with more than k neighbours, the flat row of their k-th bond in summing order)."""
        atoms = np.nonzero(nb > k)[0]
        return atoms, start[atoms] + (nb[atoms] - 1 - k if reverse else k)

    qlm = np.zeros((n, D, ORDERS), dtype=ctype)
    raw = np.zeros((n, D, ORDERS), dtype=ctype)   # N_b q_lm
    for d, l in enumerate(degrees):
        y = ylm(l, flat, dtype, route)
        for k in range(int(nb.max())):   # one neighbour after the other: the order of the sum is the order of the list
            atoms, rows = rank(k)
            raw[atoms, d, :l + 1] = raw[atoms, d, :l + 1] + y[rows]
        has = nb > 0
        qlm[has, d] = raw[has, d] / nb[has].astype(dtype)[:, None]
    ql = np.stack([invariant(qlm[:, d, :l + 1], l, dtype) for d, l in enumerate(degrees)], axis=1)
    qbar_lm = qlm.copy()
    for k in range(int(nb.max())):
        atoms, rows = rank(k)
        qbar_lm[atoms] = qbar_lm[atoms] + qlm[other[rows]]
    qbar_lm = qbar_lm / (nb + 1).astype(dtype)[:, None, None]
    qbar = np.stack([invariant(qbar_lm[:, d, :l + 1], l, dtype) for d, l in enumerate(degrees)], axis=1)
    ds, L = list(degrees).index(solid_degree), solid_degree
    v = qlm[:, ds, :L + 1]
    norm = np.sqrt(np.abs(v[:, 0]) ** 2 + 2 * (np.abs(v[:, 1:]) ** 2).sum(axis=1))
    dot = (v[owner, 0] * np.conj(v[other, 0])).real + 2 * (v[owner, 1:] * np.conj(v[other, 1:])).real.sum(axis=1)
    ok = (norm[owner] > 0) & (norm[other] > 0)
    sij = np.where(ok, dot / np.where(ok, norm[owner] * norm[other], 1), -np.inf)   # one per bond, in list order
    s_guard = float(np.abs(sij[ok] - dtype(solid_threshold)).min()) if ok.any() else np.inf
    n_conn = np.bincount(owner[sij > solid_threshold], minlength=n).astype(np.int64)
    s = np.split(sij, start[1:]) if n > 1 else [sij]
    solid = n_conn >= solid_bonds
    label = clusters(n, index, solid)
    sizes = np.bincount(label[label >= 0], minlength=n) if solid.any() else np.zeros(n, dtype=np.int64)
    bonds_all = int(nb.sum())
    Q = np.zeros(D, dtype=dtype)
    if bonds_all:
        for d, l in enumerate(degrees):
            Q[d] = invariant(raw[:, d, :l + 1].sum(axis=0) / dtype(bonds_all), l, dtype)
    out.update(qlm=qlm, ql=ql, qbar=qbar, s=s, n_conn=n_conn, solid=solid.astype(np.int64), label=label, n_solid=int(solid.sum()),
               n_clusters=int((sizes > 0).sum()), largest_cluster=int(sizes.max()) if n else 0, Q=Q, mean_qbar=qbar.sum(axis=0) / dtype(n),
               s_guard=s_guard)
    return out


def bin_of(q, bins):
    """The bin of q on [0, 1] cut into `bins`, the last one closed."""
    return np.clip(np.floor(np.asarray(q) * bins).astype(np.int64), 0, bins - 1)


def edge_guard(q, bins):
    """The distance of every q from its nearest INTERIOR bin edge k / bins, k = 1 .. bins - 1 (inf with one bin): the smallest."""
    if bins < 2:
        return np.inf
    x = np.asarray(q, dtype=np.float64).reshape(-1) * bins
    k = np.clip(np.round(x), 1, bins - 1)
    return float(np.abs(x - k).min() / bins) if len(x) else np.inf


class Accumulator:
    """One structure's accumulators over the frames fed to `sample`: what m3g_lo_read returns for it."""

    def __init__(self, species, n_species, r_cut, degrees, solid_degree, solid_threshold, solid_bonds, bins, series_cap, dtype=np.longdouble,
                 reverse=False, route="cartesian"):
        self.species, self.M, self.r_cut = np.asarray(species), n_species, r_cut
        self.degrees, self.solid = tuple(degrees), (solid_degree, solid_threshold, solid_bonds)
        self.B, self.K, self.dtype, self.reverse, self.route = bins, series_cap, dtype, reverse, route
        D = len(self.degrees)
        self.hist_q, self.hist_qbar = np.zeros((n_species, D, bins), np.int64), np.zeros((n_species, D, bins), np.int64)
        self.hist_nb = np.zeros((n_species, MAX_NEIGHBORS + 1), np.int64)
        self.moments = np.zeros((n_species, D, 4), dtype)
        self.series_counts, self.series_order = np.zeros((series_cap, 3), np.int64), np.zeros((series_cap, 2, D), dtype)
        self.n_samples = self.n_skipped = self.flags = 0
        self.frames = []

    def sample(self, pos, lattice):
        return self.add(frame(pos, lattice, self.r_cut, self.degrees, *self.solid, dtype=self.dtype, reverse=self.reverse, route=self.route))

    def add(self, fr):
        """One more sample whose frame has been evaluated already."""
        self.frames.append(fr)
        if fr["flags"]:
            self.flags |= fr["flags"]
            self.n_skipped += 1
            return fr
        for a in range(self.M):
            rows = self.species == a
            np.add.at(self.hist_nb[a], fr["n_neighbors"][rows], 1)
            for d in range(len(self.degrees)):
                np.add.at(self.hist_q[a, d], bin_of(fr["ql"][rows, d], self.B), 1)
                np.add.at(self.hist_qbar[a, d], bin_of(fr["qbar"][rows, d], self.B), 1)
                q, qb = fr["ql"][rows, d], fr["qbar"][rows, d]
                self.moments[a, d] += np.array([q.sum(), (q * q).sum(), qb.sum(), (qb * qb).sum()], dtype=self.dtype)
        if self.n_samples < self.K:
            self.series_counts[self.n_samples] = [fr["n_solid"], fr["n_clusters"], fr["largest_cluster"]]
            self.series_order[self.n_samples, 0], self.series_order[self.n_samples, 1] = fr["Q"], fr["mean_qbar"]
        self.n_samples += 1
        return fr
