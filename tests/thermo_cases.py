"""The inputs of the thermo tests, built once and never modified, their references in fp64 and in long double, and the rule that turns
the reference's own rounding into the tolerance of the device (`MARGIN`, `unit`, `deviation`: the rule of tests/scattering_cases.py and
tests/local_order_cases.py).

The batch holds the smallest shapes at which the kernels can go wrong (NAMES): one atom (the kinetic tensor is one term; with
remove_com it is zero up to rounding); two atoms in a left-handed cell (V is the absolute value of the determinant); 257 atoms in a
triclinic cell (a full 256-row chunk and a one-row chunk); 600 atoms (three chunks, the last part-filled).  Eleven frames with a cell
that changes in every frame, random velocities, float32 forces, stresses and energies, odd frames kicked (even ones without forces),
n_lags = 4 so that the ring wraps more than twice (1 and 0 beside it), and a NaN energy of the 257-atom structure in frame 5: that
sample is skipped, the flag set, its ring emptied."""
import functools

import numpy as np

import thermo_reference as ref

NAMES = ["one", "two", "tri257", "big600"]
SIZES = [1, 2, 257, 600]
N_FRAMES = 11
N_LAGS = 4
NAN_AT = (2, 5)   # (structure, frame) of the NaN energy
KICK = 0.5        # fs: the completion of odd frames
P_EXT = [0.0, 0.01, -0.002, 0.004]   # eV/A^3
SEED = 11
# What the device may deviate from the long-double reference, in units of the largest deviation of the fp64 reference from it (per
# quantity, every entry against the sum of the absolute values of its terms).  The device sums the same terms in another, equally
# valid order (a tree inside a chunk, then chunk order, a butterfly over the lanes) and may fuse a multiplication with the addition
# that follows it.  8 is the margin of tests/scattering_cases.py, for the same reason;
# tests/test_thermo_cpu.py::test_margin_covers_another_fp64_evaluation holds a second fp64 evaluation (every sum backwards) to a
# quarter of it.
MARGIN = 8.0
QUANTITIES = ("rows", "tensors", "mean", "comoments", "lag_uu", "lag_now", "lag_old")


def _build(seed):
    rng = np.random.default_rng(seed)
    cells = [np.eye(3) * 6.0, np.array([[0.3, 7.2, 0.1], [7.1, -0.2, 0.4], [0.2, 0.3, 7.6]]),
             np.diag([14.4, 14.4, 14.7]) @ np.array([[1.0, 0.03, 0.0], [0.0, 1.0, -0.04], [0.05, 0.0, 1.02]]), np.diag([40.0, 14.4, 14.4])]
    assert np.linalg.det(cells[1]) < 0
    n = sum(SIZES)
    masses = rng.uniform(1.0, 200.0, n)
    frames = []
    for k in range(N_FRAMES):
        lats = np.stack([L @ (np.eye(3) + rng.normal(0, 0.01, (3, 3))) for L in cells])
        energies = np.array([-3.5 * m for m in SIZES]) + rng.normal(0, 0.05, len(SIZES)) * np.sqrt(SIZES)
        fr = dict(lattice=lats, vel=rng.normal(0, 0.004, (n, 3)), forces=rng.normal(0, 1.0, (n, 3)).astype(np.float32),
                  stresses=rng.normal(0, 0.01, (len(SIZES), 6)).astype(np.float32), energies=energies.astype(np.float32))
        if k == NAN_AT[1]:
            fr["energies"][NAN_AT[0]] = np.nan
        frames.append(fr)
    return np.stack(cells), masses, frames


@functools.lru_cache(maxsize=None)
def batch():
    cells, masses, frames = _build(SEED)
    for arr in [cells, masses] + [a for fr in frames for a in fr.values()]:
        arr.setflags(write=False)
    return dict(cells=cells, masses=masses, frames=frames, offsets=np.concatenate([[0], np.cumsum(SIZES)]))


def kicked(k, kick_all=False):
    return kick_all or k % 2 == 1


@functools.lru_cache(maxsize=None)
def reference(dtype_name="longdouble", reverse=False, n_lags=N_LAGS, remove_com=False, kick_all=False, mode="a"):
    """One `Accumulator` per structure fed the eleven frames in the given floating type.  mode "a": velocities; "b": the kinetic
    energy and the tensor of the long-double mode-(a) reference, rounded to fp64 (what the device is fed in that mode); "b0": the
    kinetic energy alone (n_lags must be 0)."""
    dtype = getattr(np, dtype_name)
    b, off = batch(), batch()["offsets"]
    src = reference("longdouble", False, n_lags, remove_com, kick_all) if mode != "a" else None
    out = []
    for s in range(len(SIZES)):
        acc = ref.Accumulator(b["masses"][off[s]:off[s + 1]], P_EXT[s], b["cells"][s], n_lags, remove_com, dtype, reverse=reverse)
        for k, fr in enumerate(b["frames"]):
            rows = slice(off[s], off[s + 1])
            common = (fr["energies"][s], fr["stresses"][s], fr["lattice"][s])
            if mode == "a":
                acc.sample(*common, vel=fr["vel"][rows], forces=fr["forces"][rows] if kicked(k, kick_all) else None, kick=KICK)
            else:
                ke, tensor = fed(src[s], k)
                acc.sample(*common, kinetic=ke, tensor=tensor if mode == "b" else None)
        out.append(acc)
    return out


def fed(acc, k):
    """(ke, P [6]) of frame k of a mode-(a) accumulator as fp64: the inputs of mode (b)."""
    return float(acc.rows[k][1]), acc.tensors[k][:6].astype(np.float64)


def long_double_is_wider():
    return np.finfo(np.longdouble).eps < np.finfo(np.float64).eps


def _column_scales(acc):
    """(S_x [11], S_u [7]): per entry the largest term magnitude over the frames of the structure that were kept."""
    kept = [k for k, bad in enumerate(acc.skipped) if not bad]
    sx = np.max([acc.scale_x[k] for k in kept], axis=0)
    su = np.max([acc.scale_u[k] for k in kept], axis=0) if acc.scale_u[kept[0]] is not None else None
    return sx, su


def quantity(acc, name):
    """(values, scale) of a quantity of one structure's accumulator.  rows / tensors: [frames, 11 / 7] of the kept frames against the
    term magnitudes of their entries; the mean against them too; a co-moment (i, j) against n S_i S_j; the lag sums against
    lag_count times S_c^2 (uu) or S_c (now, old)."""
    kept = [k for k, bad in enumerate(acc.skipped) if not bad]
    sx, su = _column_scales(acc)
    if name == "rows":
        return np.stack([acc.rows[k] for k in kept]), np.broadcast_to(sx, (len(kept), ref.ROW))
    if name == "tensors":
        return np.stack([acc.tensors[k] for k in kept]), np.broadcast_to(su, (len(kept), ref.TENSOR))
    if name == "mean":
        return acc.mean, sx
    if name == "comoments":
        return acc.comoments, np.array([acc.n_samples * sx[i] * sx[j] for i, j in ref.TRIU])
    count = acc.lag_count[:, None].astype(np.float64)
    return getattr(acc, name), count * (su[None, :] ** 2 if name == "lag_uu" else su[None, :])


def scaled(dev, scale):
    """The largest |dev| / scale over the elements with scale > 0; elements of scale 0 must not deviate at all."""
    dev, scale = np.abs(np.asarray(dev)).astype(np.float64), np.asarray(scale, dtype=np.float64)
    if not np.isfinite(dev).all() or (dev[scale == 0] != 0).any():
        return np.inf
    return float((dev[scale > 0] / scale[scale > 0]).max()) if (scale > 0).any() else 0.0


def deviation(accs, name, got=None, **key):
    """The largest scaled deviation from the long-double reference `reference("longdouble", **key)` of `accs` (accumulators, one per
    structure) or of `got` ({structure: the device's array, shaped as `quantity` returns it})."""
    worst = 0.0
    for s, hi in enumerate(reference("longdouble", **key)):
        want, scale = quantity(hi, name)
        have = quantity(accs[s], name)[0] if got is None else got[s]
        worst = max(worst, scaled(np.asarray(have) - want, scale))
    return worst


@functools.lru_cache(maxsize=None)
def unit(name, **key):
    """The largest scaled deviation of the fp64 reference from the long-double one, over the batch: the unit of `MARGIN`.  A
    quantity whose unit comes out 0 is compared exactly."""
    assert long_double_is_wider(), "np.longdouble is no wider than fp64 here: the reference cannot measure its own rounding"
    worst = deviation(reference("float64", **key), name, **key)
    assert worst < np.inf
    return worst


def within(dev, one_unit, margin=MARGIN):
    """The gate: at most `margin` units, or no deviation at all where the unit is 0."""
    return dev <= margin * one_unit
