"""The inputs of the scattering tests, built once and never modified: the batch of tests/test_gpu_trajectory.py (1, 2, 3, 257 and 600
atoms in a cubic, an orthorhombic, a left-handed, a triclinic and a perturbed cubic cell; 1, 2, 3, 2 and 3 species) with 1, 3, 65, 257
and 0 q-vectors of indices up to +-16, eleven frames of unwrapped positions shifted by up to 40 lattice vectors, odd samples kicked
with float32 forces; the references of it in fp64 and in long double; and the rule that turns the reference's own rounding into the
tolerance of the device (`MARGIN`, `unit`, `deviation`)."""
import functools

import numpy as np

import scattering_reference as ref

SIZES = [1, 2, 3, 257, 600]   # one row; ...; a full 256-row chunk + a one-row chunk; three chunks, the last part-filled
NSPEC = [1, 2, 3, 2, 3]
NQ = [1, 3, 65, 257, 0]       # one vector; ...; a q-tile boundary crossed at any width up to 256; a structure with none
M = 3                         # max_species: structures 0, 1 and 3 have absent species
H_MAX = 16
N_LAGS = 4
N_FRAMES = 11                 # the ring of 4 wraps nearly three times
KICK = 0.7
SEED = 1
# What the device may deviate from the long-double reference, in units of the largest deviation of the fp64 reference from it (per
# quantity, each element measured against its own scale: `quantity`).  The device sums the same terms in another, equally valid order
# (row order inside a chunk, then chunk order; fused multiply-adds) and calls another sincospi; 8 is what such differences are
# expected to stay within.  tests/test_scattering_cpu.py::test_margin_covers_another_fp64_order holds a second fp64 evaluation of
# the reference (rows summed backwards, fractional coordinates formed with the division last) to the same rule, on this seed: it
# stays below 2 units, which leaves the device a factor of four over what one other order was seen to need.
MARGIN = 8.0


@functools.lru_cache(maxsize=None)
def batch():
    rng = np.random.default_rng(SEED)
    lats = [np.eye(3) * 10.4, np.diag([10.0, 11.0, 12.0]),
            np.array([[0.3, 10.2, 0.1], [10.1, -0.2, 0.4], [0.2, 0.3, 10.6]]),          # rows 0 and 1 swapped: det < 0
            np.array([[9.9, 0.0, 0.0], [2.0, 10.1, 0.0], [1.5, -1.2, 10.3]]),
            np.eye(3) * 9.0 + rng.normal(0, 0.05, (3, 3))]
    assert np.linalg.det(lats[2]) < 0
    species = [rng.permutation(np.arange(n) % k) for n, k in zip(SIZES, NSPEC)]
    masses = [rng.uniform(1.0, 200.0, n) for n in SIZES]
    pos0 = [(rng.uniform(0, 1, (n, 3)) + rng.integers(-40, 41, (n, 3))) @ L for n, L in zip(SIZES, lats)]
    n = sum(SIZES)
    pos = [np.concatenate(pos0)]
    for _ in range(N_FRAMES - 1):
        pos.append(pos[-1] + rng.normal(0, 0.1, (n, 3)))
    vel = [rng.normal(0, 0.01, (n, 3)) for _ in range(N_FRAMES)]
    forces = [rng.normal(0, 0.5, (n, 3)).astype(np.float32) for _ in range(N_FRAMES)]
    hkl = []
    for k in NQ:   # distinct non-zero triples; the first of every list carries the largest index
        h = np.zeros((0, 3), np.int32)
        while len(h) < k:
            new = rng.integers(-H_MAX, H_MAX + 1, (2 * k + 8, 3)).astype(np.int32)
            h = np.unique(np.concatenate([h, new[np.abs(new).sum(axis=1) > 0]]), axis=0)
        h = h[rng.permutation(len(h))[:k]]
        if k:
            h[0] = [H_MAX, -H_MAX, 1]
        hkl.append(np.ascontiguousarray(h))
    for arr in pos + vel + forces + lats + species + masses + hkl:
        arr.setflags(write=False)
    return dict(lats=np.stack(lats), species=species, masses=masses, pos=pos, vel=vel, forces=forces, hkl=hkl,
                offsets=np.concatenate([[0], np.cumsum(SIZES)]), q_offsets=np.concatenate([[0], np.cumsum(NQ)]))


def kicked(k, kick_all=False):
    return kick_all or k % 2 == 1


@functools.lru_cache(maxsize=None)
def reference(remove_com, dtype_name="longdouble", reverse=False, n_frames=N_FRAMES, kick_all=False):
    """One `Accumulator` per structure fed the first `n_frames` frames (frames kept: the last N_LAGS), in the given floating type."""
    dtype = getattr(np, dtype_name)
    b, off = batch(), batch()["offsets"]
    out = []
    for s in range(len(SIZES)):
        acc = ref.Accumulator(b["species"][s], b["masses"][s], b["hkl"][s], M, N_LAGS, remove_com, dtype, reverse=reverse)
        rows = slice(off[s], off[s + 1])
        for k in range(n_frames):
            acc.sample(b["pos"][k][rows], b["vel"][k][rows], b["lats"][s], b["forces"][k][rows] if kicked(k, kick_all) else None, KICK)
        out.append(acc)
    return out


def long_double_is_wider():
    return np.finfo(np.longdouble).eps < np.finfo(np.float64).eps


QUANTITIES = ("rho", "jl", "jt", "f", "cl", "ct")


def quantity(acc, name, lag=0):
    """(values, scale, floor) of a quantity of one structure's accumulator: a ring entry `lag` samples back measured against the number
    of rows summed, a correlation sum against the summed products of the moduli of its factors, above the floor of
    scattering_reference.Accumulator (what one rounding unit in each factor moves the sum by)."""
    if name in ("rho", "jl", "jt"):
        val = acc.frames[-1 - lag][("rho", "jl", "jt").index(name)]
        rows = np.bincount(acc.species, minlength=acc.M).astype(np.float64)
        return val, np.broadcast_to(rows.reshape((1, acc.M) + (1,) * (val.ndim - 2)), val.shape), 0.0
    return getattr(acc, name), getattr(acc, name + "_scale"), getattr(acc, name + "_floor")


def scaled(dev, scale, floor=0.0):
    """The largest (|dev| - floor) / scale over the elements with scale > 0; elements of scale 0 must stay within the floor (which is 0
    for a species the structure does not hold: those must not deviate at all)."""
    dev, scale = np.abs(np.asarray(dev)).astype(np.float64), np.asarray(scale, dtype=np.float64)
    excess = np.maximum(dev - floor, 0.0)
    if not np.isfinite(dev).all() or (excess[scale == 0] != 0).any():
        return np.inf
    return float((excess[scale > 0] / scale[scale > 0]).max()) if (scale > 0).any() else 0.0


def deviation(accs, name, remove_com, lag=0, got=None):
    """The largest scaled deviation from the long-double reference of `accs` (accumulators, one per structure), or of `got` (the device's
    arrays, one per structure)."""
    worst = 0.0
    for s, hi in enumerate(reference(remove_com, "longdouble")):
        want, scale, floor = quantity(hi, name, lag)
        have = quantity(accs[s], name, lag)[0] if got is None else got[s]
        worst = max(worst, scaled(have - want, scale, floor))
    return worst


@functools.lru_cache(maxsize=None)
def unit(remove_com, name, lag=0):
    """The largest scaled deviation of the fp64 reference from the long-double one, over the batch: the unit of `MARGIN`."""
    assert long_double_is_wider(), "np.longdouble is no wider than fp64 here: the reference cannot measure its own rounding"
    worst = deviation(reference(remove_com, "float64"), name, remove_com, lag)
    assert 0.0 < worst < np.inf
    return worst
