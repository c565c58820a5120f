"""Collective-variable biasing without a GPU: the restatement (tests/meta_reference.py) against finite differences and closed forms,
the host post-processing (free_energy, wham), the algorithm on a double well, the inputs of the GPU tests, and every argument check
of the host layer and of the C ABI (m3g_meta_init validates before any HIP call, so a made-up device pointer is never touched)."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import meta_cases as mc
import meta_reference as mr

ROOT = Path(__file__).resolve().parent.parent
TRICLINIC = np.array([[9.0, 0.4, -0.3], [0.8, 8.5, 0.2], [-0.5, 0.6, 9.5]])


def _lib():
    from torch_m3gnet import _lib as l

    return l, l.load_library()


def test_header_prototypes_are_bound_and_exported_and_the_abi_version_stays():
    _l, lib = _lib()
    header = (ROOT / "include" / "m3gnet_hip.h").read_text()
    declared = set(re.findall(r"\b(m3g_meta_[a-z_]+)\s*\(", header)) - {"m3g_meta_params"}
    assert declared == {"m3g_meta_state_bytes", "m3g_meta_state_view", "m3g_meta_init", "m3g_meta_bias", "m3g_meta_set_hills", "m3g_meta_read"}
    for name in declared:
        assert re.search(rf"\bint {name}\(", header) and hasattr(lib, name) and name in _l.SYMBOLS, name
    assert "#define M3G_ABI_VERSION 11" in header and _l.ABI_VERSION == 11
    assert C.sizeof(_l.M3GMetaParams) == 112
    for name, value in (("M3G_META_MAX_CV", _l.META_MAX_CV), ("M3G_META_OBS", _l.META_OBS), ("M3G_META_ERROR", _l.META_ERROR),
                        ("M3G_META_FULL", _l.META_FULL), ("M3G_CV_DISTANCE", _l.CV_DISTANCE), ("M3G_CV_PROJECTION", _l.CV_PROJECTION),
                        ("M3G_CV_COORDINATION", _l.CV_COORDINATION)):
        assert re.search(rf"#define {name} {value}\b", header), name


def _fd(f, pos, h=1e-6):
    g = np.zeros_like(pos)
    for i in range(len(pos)):
        for a in range(3):
            up, dn = pos.copy(), pos.copy()
            up[i, a] += h
            dn[i, a] -= h
            g[i, a] = (f(up) - f(dn)) / (2.0 * h)
    return g


def _small_case():
    """Eight atoms in a triclinic cell: atoms 0 and 1 straddle r_cut = 3 A with atom 2 (2.9 and 3.1 A away), atoms 3 and 4 are 2.2 A
    apart ACROSS the cell boundary (their unwrapped positions lie a lattice vector and more apart), the rest sit at random."""
    rng = np.random.default_rng(8)
    pos = rng.uniform(0.2, 0.8, (8, 3)) @ TRICLINIC
    pos[2] = np.array([4.0, 4.0, 4.0])
    pos[0], pos[1] = pos[2] + np.array([2.9, 0.0, 0.0]), pos[2] + np.array([0.0, -3.1, 0.0])
    pos[3] = np.array([0.3, 4.0, 1.0])
    pos[4] = pos[3] + np.array([-1.5, 1.0, 1.2]) + TRICLINIC[0] - 2.0 * TRICLINIC[1]
    weights = rng.uniform(1.0, 60.0, 8)
    membership = np.array([1, 1, 2, 3, 3, 2, 1, 0], dtype=np.uint8)
    return pos, weights, membership


@pytest.mark.parametrize("kind", ["distance", "projection", "coordination"])
def test_gradient_of_each_cv_meets_central_differences(kind):
    pos, w, m = _small_case()
    n = np.array([1.0, -2.0, 0.5])
    cv = mr.Cv(mc.KIND_IDS[kind], m, direction=n / np.linalg.norm(n), p=4, r0=2.0, r_cut=3.0)
    value = lambda x: mr.evaluate([cv], x, TRICLINIC, w, np.array([[0.1, 0.2, 0.3]]))["s"][0]   # noqa: E731
    ev = mr.evaluate([cv], pos, TRICLINIC, w, np.array([[0.1, 0.2, 0.3]]))
    num = _fd(value, pos)
    # central differences at h = 1e-6: truncation h^2 f''' / 6 ~ 1e-12, rounding 2^-52 |f| / h ~ 1e-9 for values of order 1 .. 10
    assert np.abs(num - ev["grad"][0]).max() < 2e-8 * max(1.0, abs(ev["s"][0])), np.abs(num - ev["grad"][0]).max()
    assert np.abs(ev["grad"][0]).max() > 1e-3 and not ev["grad"][0][7].any()
    if kind == "coordination":
        assert abs(mr.min_image_distance(pos, TRICLINIC, 0, 2) - 2.9) < 1e-12 and abs(mr.min_image_distance(pos, TRICLINIC, 1, 2) - 3.1) < 1e-12
        assert abs(mr.min_image_distance(pos, TRICLINIC, 3, 4) - np.linalg.norm([-1.5, 1.0, 1.2])) < 1e-12 < np.linalg.norm(pos[3] - pos[4]) - 15.0
        only = lambda a, b: mr.coordination(mr.Cv(mr.COORDINATION, np.eye(8, dtype=np.uint8)[a] + 2 * np.eye(8, dtype=np.uint8)[b], p=4, r0=2.0, r_cut=3.0),   # noqa: E731
                                            pos, TRICLINIC)
        (inside, g_in), (outside, g_out), (across, g_across) = only(0, 2), only(1, 2), only(3, 4)
        assert inside[0] > 0.0 and g_in[0].any() and np.array_equal(g_in[0], -g_in[2])      # 2.9 A: inside r_cut, equal and opposite rows
        assert not outside.any() and not g_out.any()                                        # 3.1 A: outside
        assert across[3] > 0.1 and g_across[4].any()                                        # the pair across the boundary counts


def test_gradient_of_the_total_bias_meets_central_differences():
    """Two CVs, restraint, an active lower and an active upper wall and 40 hills: forces_out = forces - dV/dx against the central
    difference of V from the obs row, through float32 forces of zero (so the rounding of forces_out is 2^-24 relative)."""
    pos, w, m = _small_case()
    cvs = [mr.Cv(mr.COORDINATION, m, p=2, r0=2.0, r_cut=3.0), mr.Cv(mr.DISTANCE, m)]
    s = mr.evaluate(cvs, pos, TRICLINIC, w)["s"]
    rng = np.random.default_rng(2)
    walker = dict(lattice=TRICLINIC, weights=w, centre=s + [0.2, -0.3], kappa=np.array([0.7, 1.3]),
                  walls=np.array([[s[0] + 0.05, 2.0, s[0] + 9.0, 1.0], [s[1] - 9.0, 1.0, s[1] - 0.04, 3.0]]))
    group = mr.Group(cvs, [walker], [0.3, 0.2], 0.1, 0.5, 64)
    group.set_hills(s[None, :] + rng.normal(0.0, 0.3, (40, 2)), rng.uniform(0.01, 0.1, 40))
    zero = np.zeros((8, 3), dtype=np.float32)
    (obs, f_out, _), = group.bias([pos], [zero])
    value = lambda x: group.bias([x], [zero])[0][0][2]   # noqa: E731
    num = _fd(value, pos)
    assert obs[3] > 0.05 and obs[4] > 0.01 and np.abs(f_out).max() > 1e-2
    assert np.abs(-num - f_out).max() < 1e-6 * np.abs(f_out).max() + 2e-8, np.abs(-num - f_out).max()


def test_well_tempered_heights_at_a_fixed_point_follow_the_closed_recursion():
    """A walker that does not move deposits every hill at its own CV, where each weighs exp(0) = 1: V_n = sum_{i<n} w_i and
    w_n = w0 exp(-V_n inv_kdt), in both cases to the rounding of the sum (lane-strided here, serial there)."""
    pos, w, m = _small_case()
    for inv_kdt in (0.0, 2.5):
        group = mr.Group([mr.Cv(mr.DISTANCE, m)], [dict(lattice=TRICLINIC, weights=w)], [0.2], 0.3, inv_kdt, 100)
        got = [group.bias([pos], [np.zeros((8, 3), dtype=np.float32)], deposit=True)[0][0][7] for _ in range(100)]
        total, want = 0.0, []
        for _ in range(100):
            want.append(0.3 * np.exp(-total * inv_kdt))
            total += want[-1]
        assert np.allclose(got, want, rtol=1e-13, atol=0.0) and np.array_equal(group.heights, got) and group.n_hills == 100
        assert (np.diff(got) < 0).all() if inv_kdt else (np.array(got) == 0.3).all()
    out = group.bias([pos], [np.zeros((8, 3), dtype=np.float32)], deposit=True)     # the list is full: flagged, nothing appended
    assert group.flags == [mr.FULL] and group.n_hills == 100 and out[0][0][7] == 0.0


def test_free_energy_is_the_scaled_negative_bias_with_its_minimum_at_zero():
    from torch_m3gnet.metadynamics import Hills, free_energy_scale, hills_bias

    rng = np.random.default_rng(0)
    centres, heights, grid = rng.normal(0.0, 1.0, (30, 1)), rng.uniform(0.01, 0.1, 30), np.linspace(-3.0, 3.0, 61)
    v = hills_bias(grid, centres, heights, [0.4])
    brute = np.array([(heights * np.exp(-0.5 * ((x - centres[:, 0]) / 0.4) ** 2)).sum() for x in grid])
    assert np.allclose(v, brute, rtol=1e-13)
    assert free_energy_scale(300.0, None) == 1.0 and free_energy_scale(300.0, 10.0) == 10.0 / 9.0
    for gamma, scale in ((None, 1.0), (10.0, 10.0 / 9.0), (2.0, 2.0)):
        f = Hills(centres, heights, [0.4], 300.0, gamma).free_energy(grid)
        assert f.min() == 0.0 and np.allclose(f, scale * (v.max() - v), rtol=1e-12, atol=1e-15)
    two = hills_bias(np.array([[0.0, 0.0], [1.0, 2.0]]), [[0.0, 0.0]], [1.0], [1.0, 2.0])
    assert np.allclose(two, [1.0, np.exp(-1.0)])


def test_wham_recovers_a_quartic_double_well_from_exact_samples():
    """U(s) = 4 kT (s^2 - 1)^2, 15 windows at -1.4 .. 1.4 with kappa = 80 kT, N = 20,000 samples per window drawn from each window's
    biased Boltzmann density by inverting its cumulative sum on a grid of 1e-4 (exact up to that grid).  Bound: a bin that holds n
    samples in all has a relative counting error 1 / sqrt(n) in p, kT / sqrt(n) in F; 300 bins of 0.01 over -1.5 .. 1.5 and 300,000
    samples put n_min (counted below) in the emptiest bin compared (those within -1.3 .. 1.3), and the largest of 260 such errors
    is under 4.5 standard deviations.  To that comes the histogram's own error: a bin's count is the integral of g_w = p exp(-beta
    w_w) over the bin where WHAM takes g_w at the centre times the width, a relative error of width^2 / 24 g_w'' / g_w with
    g_w'' / g_w = (beta (U' + w_w'))^2 - beta (U'' + kappa).  On |s| <= 1.3, beta |U'| <= 14.4 and beta U'' <= 65; a window 0.5 and
    more from the bin weighs below exp(-80 0.25 / 2) = exp(-10) there, so beta |w_w'| <= 40: |g'' / g| <= 54.4^2 + 145 = 3,100, times
    1e-4 / 24 = 0.013 kT.  Both after removing the mean difference."""
    from torch_m3gnet.dynamics import KB
    from torch_m3gnet.metadynamics import wham

    T = 290.0
    kt = KB * T
    u = lambda s: 4.0 * kt * (s * s - 1.0) ** 2   # noqa: E731
    centres, kappas = np.linspace(-1.4, 1.4, 15), np.full(15, 80.0 * kt)
    fine = np.arange(-2.5, 2.5, 1e-4)
    rng = np.random.default_rng(17)
    samples = []
    for c, k in zip(centres, kappas):
        cdf = np.cumsum(np.exp(-(u(fine) + 0.5 * k * (fine - c) ** 2) / kt))
        samples.append(fine[np.searchsorted(cdf, rng.uniform(0.0, cdf[-1], 20000))])
    out = wham(samples, centres, kappas, T, np.linspace(-1.5, 1.5, 301))
    keep = np.abs(out["s"]) < 1.3
    n_min = np.histogram(np.concatenate(samples), np.linspace(-1.5, 1.5, 301))[0][keep].min()
    diff = (out["free_energy"] - u(out["s"]))[keep]
    diff -= diff.mean()
    bound = (4.5 / np.sqrt(n_min) + 0.013) * kt
    print(f"wham: max |F - U| = {np.abs(diff).max() / kt:.4f} kT over {keep.sum()} bins, bound {bound / kt:.4f} kT (n_min = {n_min}), {out['iterations']} iterations")
    assert n_min > 300 and np.abs(diff).max() <= bound
    barrier = out["free_energy"][np.abs(out["s"]).argmin()] - out["free_energy"][keep].min()
    assert abs(barrier - 4.0 * kt) <= 2.0 * bound
    assert out["offsets"][0] == 0.0 and np.allclose(out["offsets"], out["offsets"][::-1], atol=0.2 * kt)   # a symmetric well: mirrored windows, equal offsets
    assert abs(out["probability"].sum() - 1.0) < 1e-12


def test_restatement_metadynamics_fills_a_double_well_to_its_barrier():
    """Two particles on a line, U(d) = 5 kT ((d - 2)^2 - 1)^2 in their distance d (wells at 1 and 3, barrier 5 kT at 2), overdamped
    Langevin dynamics, well-tempered metadynamics on the DISTANCE CV through the restatement: gamma = 10, hills of 0.5 kT and width
    0.15 every 10th of 8,000 steps.  The estimate -gamma / (gamma - 1) V_hills must show the barrier.  Bound: at convergence
    V_hills ~ 0.9 x 5 kT at the bottom, so the hills still arriving are 0.5 kT exp(-4.5 / 9) = 0.3 kT high; neighbouring hills (spacing
    well under the width) overlap several-fold, so the estimate carries a roughness of a few such heights: 1 kT on either of the two
    levels whose difference the barrier is, 1.5 kT allowed."""
    kt, barrier, gamma = 1.0, 5.0, 10.0
    m = np.array([1, 2], dtype=np.uint8)
    lattice = np.eye(3) * 50.0
    group = mr.Group([mr.Cv(mr.DISTANCE, m)], [dict(lattice=lattice, weights=np.ones(2), walls=np.array([[0.4, 50.0, 3.6, 50.0]]))], [0.15],
                     0.5 * kt, 1.0 / ((gamma - 1.0) * kt), 800)
    rng = np.random.default_rng(1)
    pos = np.array([[10.0, 10.0, 10.0], [11.0, 10.0, 10.0]])
    dt, visited = 2e-3, []
    for k in range(1, 8001):
        d = pos[1, 0] - pos[0, 0]
        du = barrier * 4.0 * ((d - 2.0) ** 2 - 1.0) * (d - 2.0)
        f = np.zeros((2, 3), dtype=np.float32)
        f[0, 0], f[1, 0] = du, -du
        (obs, f_out, _), = group.bias([pos], [f], deposit=(k % 10 == 0))
        pos[:, 0] += dt * f_out[:, 0].astype(np.float64) / kt + np.sqrt(2.0 * dt) * rng.normal(size=2)
        visited.append(obs[0])
    visited = np.array(visited)
    assert group.n_hills == 800 and visited.min() < 1.2 and visited.max() > 2.8      # both wells were visited
    grid = np.linspace(0.8, 3.2, 49)
    v, _, _, _ = zip(*[mr.hills_sum([x], group.centres, group.heights, [0.15]) for x in grid])
    f_est = -gamma / (gamma - 1.0) * np.array(v)
    f_est -= f_est.min()
    top = f_est[np.abs(grid - 2.0) < 0.11].max()
    wells = max(f_est[np.abs(grid - 1.0) < 0.16].min(), f_est[np.abs(grid - 3.0) < 0.16].min())
    print(f"double well: barrier {top - wells:.2f} kT from {group.n_hills} hills (known: 5 kT)")
    assert abs((top - wells) - barrier) <= 1.5, (top, wells)


def test_the_gpu_cases_hold_the_edges_they_are_built_for():
    for idx, n in enumerate(mc.SIZES):
        lattice, pos, w, membership, forces, _ = mc.structure(idx)
        volume = abs(np.linalg.det(lattice))
        width = min(volume / np.linalg.norm(np.cross(lattice[(a + 1) % 3], lattice[(a + 2) % 3])) for a in range(3))
        assert max(mc.R_CUT) <= 0.5 * width and len(pos) == n and forces.dtype == np.float32
        frac = pos @ np.linalg.inv(lattice)
        assert n < 8 or (frac.min() < -1.5 and frac.max() > 2.5)                      # spread over -2 .. 3 cells
        for k in range(2):
            assert (membership[k] & 1).any() and (membership[k] & 2).any()
        assert n < 200 or all((membership == v).any() for v in range(4))
    assert np.array_equal(mc.structure(3, 0)[3], mc.structure(3, 1)[3]) and not np.array_equal(mc.structure(3, 0)[1], mc.structure(3, 1)[1])
    lattice, pos = mc.structure(0)[:2]
    assert mr.min_image_distance(pos, lattice, 0, 1) < 3.0 < np.linalg.norm(pos[0] - pos[1]) - 10.0   # the pair is close only across the boundary
    assert [(n - 1) // 256 + 1 for n in mc.SIZES] == [1, 1, 2, 3] and mc.SIZES[2] % 256 == 1
    for n in mc.DIRECTIONS:
        assert abs(n @ n - 1.0) < 1e-15


# ---- the C ABI's checks: before any HIP call, so a made-up device pointer is never touched ---------------------------------------
@pytest.mark.parametrize("name,change,reason", mc.REFUSALS, ids=[r[0] for r in mc.REFUSALS])
def test_c_abi_init_refuses(name, change, reason):
    _l, lib = _lib()
    args = mc.init_arguments()
    change(args)
    assert mc.call_init(lib, _l, args, C.c_void_p(256), 1 << 30) == _l.M3G_ERR_VALUE, name
    assert reason in lib.m3g_last_error() and lib.m3g_last_error().startswith(b"m3g_meta_init:"), lib.m3g_last_error()


def test_c_abi_refuses_null_pointers_short_buffers_and_bad_hill_lists():
    _l, lib = _lib()
    d, big = C.c_void_p(256), 1 << 30
    good = mc.init_arguments()
    assert mc.call_init(lib, _l, good, d, 64) == _l.M3G_ERR_SIZE and b"too small" in lib.m3g_last_error()
    assert mc.call_init(lib, _l, good, None, big) == _l.M3G_ERR_VALUE
    p = _l.M3GMetaParams(n_cv=1, reserved=0, max_hills=4)
    nbytes = C.c_size_t()
    assert lib.m3g_meta_state_bytes(5, 2, 2, 1, 4, C.byref(nbytes)) == _l.M3G_OK
    for bad in ((0, 1, 1, 1, 4), (5, 6, 1, 1, 4), (5, 2, 3, 1, 4), (5, 2, 0, 1, 4), (5, 2, 2, 0, 4), (5, 2, 2, 3, 4), (5, 2, 2, 1, -1)):
        assert lib.m3g_meta_state_bytes(*bad, C.byref(nbytes)) == _l.M3G_ERR_VALUE, bad
    assert lib.m3g_meta_state_bytes(5, 2, 2, 1, 4, None) == _l.M3G_ERR_VALUE
    assert lib.m3g_meta_state_view(5, 2, 2, 1, 4, None) == _l.M3G_ERR_VALUE
    assert lib.m3g_meta_bias(C.byref(p), 5, 2, 2, d, big, None, d, d, 0, None, None) == _l.M3G_ERR_VALUE
    assert lib.m3g_meta_bias(C.byref(p), 5, 2, 2, d, 64, d, d, d, 0, None, None) == _l.M3G_ERR_SIZE
    assert lib.m3g_meta_bias(None, 5, 2, 2, d, big, d, d, d, 0, None, None) == _l.M3G_ERR_VALUE
    assert lib.m3g_meta_read(C.byref(p), 5, 2, 2, d, 64, None, None, None, None, None, None) == _l.M3G_ERR_SIZE
    groups, centres, heights = np.array([0, 2], dtype=np.int64), np.zeros((1, 4, 1)), np.zeros((1, 4))
    for counts, reason in (([5], b"multiple"), ([3], b"multiple"), ([-2], b"multiple")):
        c = np.array(counts, dtype=np.int64)
        assert lib.m3g_meta_set_hills(C.byref(p), 5, 2, 1, d, big, groups.ctypes.data, c.ctypes.data, centres.ctypes.data, heights.ctypes.data,
                                      None) == _l.M3G_ERR_VALUE and reason in lib.m3g_last_error()
    heights[0, 1] = np.nan
    c = np.array([2], dtype=np.int64)
    assert lib.m3g_meta_set_hills(C.byref(p), 5, 2, 1, d, big, groups.ctypes.data, c.ctypes.data, centres.ctypes.data, heights.ctypes.data,
                                  None) == _l.M3G_ERR_VALUE and b"not finite" in lib.m3g_last_error()


def test_c_abi_state_bytes_grow_with_every_size():
    _l, lib = _lib()
    sizes = {}
    for args in [(2, 1, 1, 1, 0), (10000, 1, 1, 1, 0), (10000, 100, 1, 1, 0), (10000, 100, 50, 1, 0), (10000, 100, 50, 2, 0), (10000, 100, 50, 2, 1000)]:
        nbytes = C.c_size_t()
        assert lib.m3g_meta_state_bytes(*args, C.byref(nbytes)) == _l.M3G_OK
        sizes[args] = nbytes.value
    values = list(sizes.values())
    assert all(a < b for a, b in zip(values, values[1:])), sizes
    assert values[-1] - values[-2] >= 50 * 1000 * 3 * 8          # the hills: centres [G, max_hills, n_cv] and heights
    at = C.c_size_t()
    assert lib.m3g_meta_state_view(10000, 100, 50, 2, 1000, C.byref(at)) == _l.M3G_OK and 0 < at.value < values[-1] - 2 * 10000 * 24


def test_host_layer_argument_validation():
    from torch_m3gnet import metadynamics as md
    from torch_m3gnet.model.build import build_model

    cv = md.projection([0], [1, 2], [0.0, 3.0, 4.0])
    assert cv.direction == (0.0, 0.6, 0.8) and cv.origin is None and md.projection([0], [], [1, 0, 0]).b == ()
    assert md.coordination([0], [1], 2.0).r_cut == 5.0 and md.coordination([0], [1], 2.0).p == 3 and md.distance(range(2), [5]).a == (0, 1)
    for make in (lambda: md.distance([], [1]), lambda: md.distance([0], []), lambda: md.distance([0, 0], [1]), lambda: md.distance([-1], [1]),
                 lambda: md.distance([0.5], [1]), lambda: md.distance([True], [1]), lambda: md.projection([], [1], [1, 0, 0]),
                 lambda: md.projection([0], [1], [0, 0, 0]), lambda: md.projection([0], [1], [1, 0]), lambda: md.projection([0], [1], [np.nan, 0, 1]),
                 lambda: md.projection([0], [1], [1, 0, 0], origin=[0, 1]), lambda: md.projection([0], [1], [1, 0, 0], origin=[0, np.inf, 0]),
                 lambda: md.coordination([0], [1], 0.0), lambda: md.coordination([0], [1], 2.0, p=0), lambda: md.coordination([0], [1], 2.0, p=7),
                 lambda: md.coordination([0], [1], 2.0, p=2.0), lambda: md.coordination([0], [1], 2.0, r_cut=-1.0), lambda: md.coordination([0], [], 2.0)):
        with pytest.raises(ValueError):
            make()
    model = build_model(5.0, 4.0, 3, 3, 95, 16, 1)
    good = dict(cvs=cv, temperature=300.0, height=0.01, sigma=[0.1], pace=10)
    meta = md.Metadynamics(model, **good)
    assert (meta.walkers, meta.bias_factor, meta.pace, meta.walls) == (1, None, 10, None)
    for kw in (dict(cvs=[]), dict(cvs=[cv, cv, cv]), dict(cvs="distance"), dict(temperature=0.0), dict(height=-1.0), dict(sigma=[0.1, 0.2]),
               dict(sigma=[0.0]), dict(sigma=[np.nan]), dict(pace=0), dict(pace=2.5), dict(bias_factor=1.0), dict(bias_factor=np.inf),
               dict(walkers=0), dict(walls=np.zeros((3, 4))), dict(timestep=0.0), dict(friction=-0.1)):
        with pytest.raises(ValueError):
            md.Metadynamics(model, **{**good, **kw})
    with pytest.raises(TypeError):
        md.Metadynamics(model.model, **good)
    ok = dict(cv=cv, centres=[0.0, 0.1], kappa=2.0, temperature=300.0)
    assert md.UmbrellaSampling(model, **ok).kappa.tolist() == [2.0, 2.0]
    for kw in (dict(cv=[cv, cv]), dict(centres=[]), dict(centres=[np.nan]), dict(kappa=[1.0, 2.0, 3.0]), dict(kappa=-1.0), dict(temperature=-5.0)):
        with pytest.raises(ValueError):
            md.UmbrellaSampling(model, **{**ok, **kw})
    # counted in run() before anything touches the device
    lat, pos, z = np.eye(3) * 5.0, np.zeros((2, 3)) + [[0.0], [2.5]], np.array([29, 29])
    for kw in (dict(steps=-1), dict(steps=1.5), dict(equilibration=-1), dict(loginterval=0)):
        with pytest.raises(ValueError):
            meta.run([lat], [pos], [z], **{**dict(steps=10), **kw})
    # the thin layer's own checks, before the state is allocated
    base = dict(offsets=[0, 3], lattices=np.eye(3)[None] * 9.0, cvs=cv, weights=np.ones(3), sigma=[0.1])
    for kw in (dict(offsets=[0]), dict(lattices=np.eye(3)), dict(weights=np.ones(4)), dict(max_hills=-1), dict(group_offsets=[0]),
               dict(cvs=md.distance([0], [3])), dict(sigma=[0.1, 0.2]), dict(centres=np.zeros((2, 2))), dict(walls=np.zeros(3)),
               dict(membership=np.zeros((2, 3), dtype=np.uint8))):
        with pytest.raises(ValueError):
            md.BiasState(**{**base, **kw})
    s = [np.array([0.0, 0.1]), np.array([0.2])]
    for args in ((s, [0.0], [1.0, 1.0], 300.0, 10), (s, [0.0, 0.1], [1.0, -1.0], 300.0, 10), (s, [0.0, 0.1], [1.0, 1.0], 0.0, 10),
                 (s, [0.0, 0.1], [1.0, 1.0], 300.0, 0), (s, [0.0, 0.1], [1.0, 1.0], 300.0, [0.0, 0.0, 1.0]), ([s[0], np.array([])], [0.0, 0.1], [1.0, 1.0], 300.0, 10),
                 (s, [0.0, 0.1], [1.0, 1.0], 300.0, [5.0, 6.0])):
        with pytest.raises(ValueError):
            md.wham(*args)
