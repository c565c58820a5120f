"""The inputs of the local-order tests, built once and never modified, their references in fp64 and in long double, and the rule that
turns the reference's own rounding into the tolerance of the device (`MARGIN`, `unit`, `deviation`: the rule of
tests/scattering_cases.py).

The batch holds the smallest shapes at which each kernel can go wrong (NAMES): one atom (no neighbour, everything 0); two atoms in a
left-handed cell (one bond each: q_l = 1 for every l); 257 atoms of three species, thermally perturbed fcc plus an interstitial in a
triclinic cell (a full 256-row chunk and a one-row chunk); 600 atoms in three chunks, stored in shuffled order: along the first axis of
the cell a perturbed-fcc slab that wraps the periodic boundary, random points with a minimum separation, a second, separate slab, and
random points again -- clusters that span the periodic boundary and the chunk boundaries, at least two of them, solid and non-solid
atoms; a dense random structure in which atoms have more than 32 neighbours (flagged and skipped); and the ideal lattices fcc 4x4x4
(256 atoms: exactly one chunk), bcc 3x3x3 with r_cut past the second shell (14 neighbours), hcp and simple cubic.  Five frames (the
ideal lattices stand still), positions shifted by up to +-40 lattice vectors, a series of three rows so that the cap is crossed, and
the degrees 4, 6 and 12: three of them and the largest l, the limits of the register arrays."""
import functools

import numpy as np

import local_order_reference as ref

NAMES = ["one", "two", "fcc257", "slabs600", "dense", "fcc", "bcc", "hcp", "sc"]
SIZES = [1, 2, 257, 600, 72, 256, 54, 96, 64]
R_CUT = [2.5, 3.2, 3.05, 3.05, 3.8, 3.05, 3.4, 3.0, 3.0]
IDEAL = [5, 6, 7, 8]          # their q_l sit on a point: no histogram comparison
FLAGGED = {4: ref.NEIGHBORS}   # structure: the flag every one of its samples raises
M = 3                         # max_species: only structure 2 holds all three
DEGREES = (4, 6, 12)
SOLID = (6, 0.5, 6)           # solid_degree, solid_threshold, solid_bonds (6: simple cubic has six neighbours)
BINS = 20
SERIES_CAP = 3
N_FRAMES = 5
GUARD = 1e-9
SEED = 7
# What the device may deviate from the long-double reference, in units of the largest deviation of the fp64 reference from it (per
# quantity; a per-atom value against 1, a sum against its number of terms).  The device sums the same terms in another, equally valid
# order (list order in registers, a tree inside a chunk, then chunk order; fused multiply-adds; another sqrt and division) and reaches
# the bond vectors through rint instead of 27 images.  8 is the margin of tests/scattering_cases.py, for the same reason;
# tests/test_local_order_cpu.py::test_margin_covers_another_fp64_evaluation holds a second fp64 evaluation of the reference
# (neighbours summed backwards, Y_lm in polar form) to a quarter of it.
MARGIN = 8.0
A_FCC = 3.6


def _fcc(n, a=A_FCC):
    base = np.array([[0, 0, 0], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5]])
    cells = np.array([[i, j, k] for i in range(n[0]) for j in range(n[1]) for k in range(n[2])])
    return ((cells[:, None, :] + base[None]).reshape(-1, 3)) * a, np.diag(np.array(n, dtype=np.float64) * a)


def _random_points(rng, count, lo, hi, lattice, others, min_sep):
    """`count` points with x in [lo, hi) of the orthorhombic cell, at least `min_sep` (minimum image) from each other and `others`."""
    box = np.diag(lattice)
    pts = [p for p in others]
    made = []
    while len(made) < count:
        p = np.array([rng.uniform(lo, hi), rng.uniform(0, box[1]), rng.uniform(0, box[2])])
        d = np.asarray(pts) - p if pts else np.zeros((0, 3))
        d -= np.round(d / box) * box
        if not len(d) or np.sqrt((d * d).sum(axis=1)).min() >= min_sep:
            pts.append(p)
            made.append(p)
    return np.array(made)


def _build(seed):
    rng = np.random.default_rng(seed)
    lats, pos, species = [], [], []
    # one atom; two atoms in a left-handed cell
    lats.append(np.eye(3) * 6.0), pos.append(np.array([[1.0, 2.0, 3.0]])), species.append(np.zeros(1, int))
    left = np.array([[0.3, 7.2, 0.1], [7.1, -0.2, 0.4], [0.2, 0.3, 7.6]])
    lats.append(left), pos.append(np.array([[0.2, 0.3, 0.1], [0.5, 0.45, 0.3]]) @ left), species.append(np.array([0, 1]))
    # 257: fcc 4x4x4 and an interstitial, sheared
    p, L = _fcc((4, 4, 4))
    p = np.concatenate([p, [[0.5 * A_FCC + 0.21, 0.13, -0.17]]])
    shear = np.array([[1.0, 0.03, 0.0], [0.0, 1.0, -0.04], [0.05, 0.0, 1.02]])
    lats.append(L @ shear), pos.append((p + rng.normal(0, 0.05, p.shape)) @ shear), species.append(rng.permutation(np.arange(257) % 3))
    # 600: slab A (3 cells, 192 atoms, six layers 9 A thick) around x = 0, 11 A apart slab B around x = 20; 108 random points in
    # either gap, 1.9 A from the slabs' surfaces and from each other
    slab, _ = _fcc((3, 4, 4))
    half, length, away = 1.25 * A_FCC, 40.0, 1.9
    L = np.diag([length, 4 * A_FCC, 4 * A_FCC])
    a_slab = slab + [-half, 0, 0]
    b_slab = slab + [0.5 * length - half, 0.3, 0.7]
    crystal = np.concatenate([a_slab, b_slab]) + rng.normal(0, 0.04, (384, 3))
    g1 = _random_points(rng, 108, half + away, 0.5 * length - half - away, L, list(crystal), away)
    g2 = _random_points(rng, 108, 0.5 * length + half + away, length - half - away, L, list(crystal) + list(g1), away)
    allp = np.concatenate([crystal, g1, g2])
    order = rng.permutation(600)
    lats.append(L), pos.append(allp[order]), species.append(np.arange(600) % 2)
    # dense: more than 32 neighbours
    lats.append(np.eye(3) * 8.0 + rng.normal(0, 0.05, (3, 3))), pos.append(rng.uniform(0, 8.0, (72, 3))), species.append(np.zeros(72, int))
    # ideal lattices
    p, L = _fcc((4, 4, 4))
    lats.append(L), pos.append(p), species.append(np.zeros(256, int))
    cells = np.array([[i, j, k] for i in range(3) for j in range(3) for k in range(3)], dtype=np.float64)
    lats.append(np.eye(3) * 3 * 2.87), pos.append(np.concatenate([cells, cells + 0.5]) * 2.87), species.append(np.zeros(54, int))
    a, c = 2.5, 2.5 * np.sqrt(8.0 / 3.0)
    hexa = np.array([[a, 0, 0], [-0.5 * a, 0.5 * np.sqrt(3.0) * a, 0], [0, 0, c]])
    cells = np.array([[i, j, k] for i in range(4) for j in range(4) for k in range(3)], dtype=np.float64)
    frac = np.concatenate([cells, cells + [1.0 / 3.0, 2.0 / 3.0, 0.5]])
    lats.append(hexa * np.array([[4.0], [4.0], [3.0]])), pos.append(frac @ hexa), species.append(np.zeros(96, int))
    cells = np.array([[i, j, k] for i in range(4) for j in range(4) for k in range(4)], dtype=np.float64)
    lats.append(np.eye(3) * 4 * 2.6), pos.append(cells * 2.6), species.append(np.zeros(64, int))
    assert [len(p) for p in pos] == SIZES and np.linalg.det(lats[1]) < 0
    shifted = [p + rng.integers(-40, 41, p.shape) @ L for p, L in zip(pos, lats)]
    frames = [np.concatenate(shifted)]
    moving = np.concatenate([np.full(n, 0.0 if s in IDEAL or s < 2 else 1.0) for s, n in enumerate(SIZES)])[:, None]
    for _ in range(N_FRAMES - 1):
        frames.append(frames[-1] + moving * rng.normal(0, 0.03, frames[-1].shape))
    return lats, species, frames


@functools.lru_cache(maxsize=None)
def batch():
    lats, species, frames = _build(SEED)
    for arr in lats + species + frames:
        arr.setflags(write=False)
    return dict(lats=np.stack(lats), species=species, pos=frames, offsets=np.concatenate([[0], np.cumsum(SIZES)]),
                r_cut=np.array(R_CUT))


@functools.lru_cache(maxsize=None)
def reference(dtype_name="longdouble", reverse=False, route="cartesian", n_frames=N_FRAMES):
    """One `Accumulator` per structure fed the first `n_frames` frames, in the given floating type; every frame is kept on it."""
    dtype = getattr(np, dtype_name)
    b, off = batch(), batch()["offsets"]
    out = []
    for s in range(len(SIZES)):
        acc = ref.Accumulator(b["species"][s], M, R_CUT[s], DEGREES, *SOLID, BINS, SERIES_CAP, dtype, reverse=reverse, route=route)
        for k in range(n_frames):
            if k and (s in IDEAL or s < 2):   # (they stand still: the frame is the one before)
                acc.add(acc.frames[-1])
                continue
            acc.sample(b["pos"][k][off[s]:off[s + 1]], b["lats"][s])
        out.append(acc)
    return out


def check_guards():
    """The discrete outputs are unambiguous: every pair distance is GUARD (relative) away from r_cut, every s_ij from the threshold,
    every q_l and qbar_l of a non-ideal structure from its nearest interior histogram edge; the 600-atom structure has at least two
    clusters, solid and non-solid atoms; the dense one is flagged in every frame.  Returns the smallest guards seen."""
    worst = dict(r=np.inf, s=np.inf, edge=np.inf)
    for s, acc in enumerate(reference("longdouble")):
        for fr in acc.frames:
            assert fr["flags"] == FLAGGED.get(s, 0), (s, fr["flags"])
            worst["r"] = min(worst["r"], fr["r_guard"])
            if fr["flags"]:
                continue
            worst["s"] = min(worst["s"], fr["s_guard"])
            if s not in IDEAL:
                worst["edge"] = min(worst["edge"], ref.edge_guard(fr["ql"], BINS), ref.edge_guard(fr["qbar"], BINS))
            if NAMES[s] == "slabs600":
                assert fr["n_clusters"] >= 2 and 0 < fr["n_solid"] < 600 and fr["largest_cluster"] > 100, (fr["n_clusters"], fr["n_solid"])
        if s in FLAGGED:
            assert max(fr["n_neighbors"].max() for fr in acc.frames) > ref.MAX_NEIGHBORS
    assert min(worst.values()) >= GUARD, worst
    return worst


def long_double_is_wider():
    return np.finfo(np.longdouble).eps < np.finfo(np.float64).eps


QUANTITIES = ("qlm", "ql", "qbar", "moments", "Q", "mean_qbar")
CLEAN = [s for s in range(len(SIZES)) if s not in FLAGGED]


def quantity(acc, name, k=N_FRAMES - 1):
    """(values, scale) of a quantity of one structure's accumulator: the per-atom arrays of frame `k` against 1, the moment sums
    against their number of terms (atoms of the species times samples), the series against 1."""
    if name in ("qlm", "ql", "qbar"):
        val = acc.frames[k][name]
        return val, np.ones(val.shape)
    if name == "moments":
        terms = np.bincount(acc.species, minlength=acc.M).astype(np.float64) * acc.n_samples
        return acc.moments, np.broadcast_to(terms[:, None, None], acc.moments.shape)
    val = acc.series_order[:, ("Q", "mean_qbar").index(name)]
    return val, np.ones(val.shape)


def scaled(dev, scale):
    """The largest |dev| / scale over the elements with scale > 0; elements of scale 0 (a species the structure does not hold) must not
    deviate at all."""
    dev, scale = np.abs(np.asarray(dev)).astype(np.float64), np.asarray(scale, dtype=np.float64)
    if not np.isfinite(dev).all() or (dev[scale == 0] != 0).any():
        return np.inf
    return float((dev[scale > 0] / scale[scale > 0]).max()) if (scale > 0).any() else 0.0


def deviation(accs, name, k=N_FRAMES - 1, got=None):
    """The largest scaled deviation from the long-double reference of `accs` (accumulators, one per structure), or of `got` ({structure:
    the device's array}), over the structures that raise no flag."""
    worst = 0.0
    hi = reference("longdouble")
    for s in CLEAN:
        want, scale = quantity(hi[s], name, k)
        have = quantity(accs[s], name, k)[0] if got is None else got[s]
        worst = max(worst, scaled(np.asarray(have) - want, scale))
    return worst


@functools.lru_cache(maxsize=None)
def unit(name, k=N_FRAMES - 1):
    """The largest scaled deviation of the fp64 reference from the long-double one, over the batch: the unit of `MARGIN`."""
    assert long_double_is_wider(), "np.longdouble is no wider than fp64 here: the reference cannot measure its own rounding"
    worst = deviation(reference("float64"), name, k)
    assert 0.0 < worst < np.inf
    return worst
