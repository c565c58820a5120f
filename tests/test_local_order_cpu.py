"""Local-order observables without a GPU: the restatement (tests/local_order_reference.py) against closed forms and known values, its
invariance under rigid rotations and lattice-vector shifts; the guards of the test batch (tests/local_order_cases.py) and the margin
the GPU test allows the device, held to a second fp64 evaluation; the host post-processing on synthetic accumulators and the forms of
`r_cut`; the export surface; every refusal of the C ABI that precedes its first HIP call (status and message pinned, as
tests/test_entry_refusals_cpu.py does); and the `observables` argument of MolecularDynamics.run."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import local_order_cases as lc
import local_order_reference as ref

ROOT = Path(__file__).resolve().parent.parent
DUMMY, BIG = C.c_void_p(256), 1 << 30
M3G_OK, M3G_ERR_VALUE, M3G_ERR_SIZE = 0, 1, 3
IDEAL = {name: lc.NAMES.index(name) for name in ("fcc", "bcc", "hcp", "sc")}


def _lib():
    from torch_m3gnet import _lib as l

    return l, l.load_library()


def _last(s):
    return lc.reference("longdouble")[s].frames[-1]


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def test_closed_forms_of_fcc_simple_cubic_and_a_single_bond():
    fcc, sc, two = _last(IDEAL["fcc"]), _last(IDEAL["sc"]), _last(lc.NAMES.index("two"))
    assert (fcc["n_neighbors"] == 12).all() and (sc["n_neighbors"] == 6).all() and (two["n_neighbors"] == 1).all()
    for fr, q4, q6 in ((fcc, np.sqrt(7.0 / 192.0), np.sqrt(169.0 / 512.0)), (sc, np.sqrt(7.0 / 12.0), np.sqrt(1.0 / 8.0))):
        assert np.abs(fr["ql"][:, 0] - q4).max() < 1e-12 and np.abs(fr["ql"][:, 1] - q6).max() < 1e-12
        assert np.abs(fr["Q"][:2] - [q4, q6]).max() < 1e-12
    assert np.abs(two["ql"] - 1).max() < 1e-12 and np.abs(two["qbar"] - 1).max() < 1e-12   # one bond: q_l = 1 for every l
    one = _last(0)
    assert (one["n_neighbors"] == 0).all() and (one["ql"] == 0).all() and (one["qbar"] == 0).all() and (one["Q"] == 0).all()
    assert one["n_solid"] == 0 and one["label"][0] == -1


def test_known_values_of_hcp_and_bcc_with_both_shells():
    hcp, bcc = _last(IDEAL["hcp"]), _last(IDEAL["bcc"])
    assert (hcp["n_neighbors"] == 12).all() and (bcc["n_neighbors"] == 14).all()
    assert np.abs(hcp["ql"][:, :2] - [0.097222, 0.484762]).max() < 1e-6
    assert np.abs(bcc["ql"][:, :2] - [0.036370, 0.510688]).max() < 1e-6


def test_ideal_lattices_are_one_solid_cluster():
    for name, s in IDEAL.items():
        fr = _last(s)
        n = lc.SIZES[s]
        assert np.abs(np.concatenate(fr["s"]) - 1).max() < 1e-12, name
        assert (fr["solid"] == 1).all() and (fr["label"] == 0).all(), name
        assert (fr["n_solid"], fr["n_clusters"], fr["largest_cluster"]) == (n, 1, n), name
        assert np.abs(fr["qbar"] - fr["ql"]).max() < 1e-12, name   # every atom alike: the average changes nothing


def _structure(s, k=0):
    b = lc.batch()
    return b["pos"][k][b["offsets"][s]:b["offsets"][s + 1]], b["lats"][s]


def _same_frame(a, b, tol=1e-9):
    assert np.array_equal(a["n_neighbors"], b["n_neighbors"]) and np.array_equal(a["label"], b["label"])
    assert np.array_equal(a["n_conn"], b["n_conn"]) and np.array_equal(a["solid"], b["solid"])
    for key in ("ql", "qbar", "Q", "mean_qbar"):
        assert np.abs(a[key] - b[key]).max() < tol, key
    assert np.abs(np.concatenate(a["s"]) - np.concatenate(b["s"])).max() < tol


def test_invariants_under_a_rigid_rotation_and_lattice_shifts():
    """q_l, qbar_l, s_ij and the labels do not see a rotation of cell and positions, nor a shift of atoms by lattice vectors (q_lm does
    see the rotation: it is not compared)."""
    rng = np.random.default_rng(3)
    s = lc.NAMES.index("fcc257")
    pos, L = _structure(s)
    args = (lc.R_CUT[s], lc.DEGREES, *lc.SOLID)
    plain = ref.frame(pos, L, *args, dtype=np.float64)
    rot, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    rot *= np.sign(np.linalg.det(rot))
    turned = ref.frame(pos @ rot, L @ rot, *args, dtype=np.float64)
    _same_frame(plain, turned)
    assert np.abs(plain["qlm"] - turned["qlm"]).max() > 1e-3
    moved = ref.frame(pos + rng.integers(-3, 4, pos.shape) @ L, L, *args, dtype=np.float64)
    _same_frame(plain, moved)
    assert np.abs(plain["qlm"] - moved["qlm"]).max() < 1e-9


def test_polar_and_cartesian_harmonics_agree_and_are_orthonormal():
    rng = np.random.default_rng(0)
    u = rng.normal(size=(50, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    u = np.concatenate([u, [[0, 0, 1.0], [0, 0, -1.0], [1.0, 0, 0]]])   # a bond along +-z is an ordinary input
    for l in (1, 4, 6, 12):
        a, b = ref.ylm(l, u, np.float64, "cartesian"), ref.ylm(l, u, np.float64, "polar")
        assert np.abs(a - b).max() < 1e-13
        # the addition theorem at equal arguments: sum_m |Y_lm|^2 = (2l + 1) / 4 pi
        assert np.abs(np.abs(a[:, 0]) ** 2 + 2 * (np.abs(a[:, 1:]) ** 2).sum(axis=1) - (2 * l + 1) / (4 * np.pi)).max() < 1e-13
    assert abs(ref.ylm(1, [[0, 0, 1.0]], np.float64)[0, 0] - np.sqrt(3 / (4 * np.pi))) < 1e-15
    assert abs(ref.ylm(1, [[1.0, 0, 0]], np.float64)[0, 1] + np.sqrt(3 / (8 * np.pi))) < 1e-15   # Condon-Shortley: Y_11 < 0 on +x


def test_the_guards_of_the_cases_hold():
    worst = lc.check_guards()
    print("smallest guards:", worst)
    hi = lc.reference("longdouble")
    assert [a.n_samples for a in hi] == [0 if s in lc.FLAGGED else lc.N_FRAMES for s in range(len(lc.SIZES))]
    assert [a.n_skipped for a in hi] == [lc.N_FRAMES if s in lc.FLAGGED else 0 for s in range(len(lc.SIZES))]
    # the discrete outputs of the fp64 evaluation are those of the long-double one
    for a, b in zip(hi, lc.reference("float64")):
        assert np.array_equal(a.hist_q, b.hist_q) and np.array_equal(a.hist_qbar, b.hist_qbar) and np.array_equal(a.hist_nb, b.hist_nb)
        assert np.array_equal(a.series_counts, b.series_counts) and a.flags == b.flags
        for fa, fb in zip(a.frames, b.frames):
            if not fa["flags"]:
                assert np.array_equal(fa["label"], fb["label"]) and np.array_equal(fa["n_conn"], fb["n_conn"])
    slabs = hi[lc.NAMES.index("slabs600")]
    assert slabs.series_counts[:, 1].min() >= 2 and (slabs.series_order[lc.SERIES_CAP - 1] != 0).all()


def test_margin_covers_another_fp64_evaluation():
    """A second fp64 evaluation of the reference -- neighbours summed backwards, Y_lm in polar form -- stays within a quarter of
    MARGIN units of the long-double one, per quantity."""
    assert lc.long_double_is_wider()
    other = lc.reference("float64", True, "polar")
    for name in lc.QUANTITIES:
        ratio = lc.deviation(other, name) / lc.unit(name)
        print(f"{name}: unit {lc.unit(name):.3e}, the second evaluation at {ratio:.3f} units")
        assert ratio <= lc.MARGIN / 4, (name, ratio)


# ---- host logic ----------------------------------------------------------------------------------------------------------------------
def test_results_from_synthetic_accumulators():
    from torch_m3gnet.local_order import decode_flags, local_order_from_sums

    rng = np.random.default_rng(1)
    counts, n_samples, bins, D, cap = np.array([3, 5]), 4, 10, 2, 3
    values = [rng.uniform(0, 1, (n_samples * c, D, 2)) for c in counts]   # (q, qbar) of every atom and sample
    hist_q = np.array([[np.histogram(v[:, d, 0], bins, (0, 1))[0] for d in range(D)] for v in values])
    hist_qbar = np.array([[np.histogram(v[:, d, 1], bins, (0, 1))[0] for d in range(D)] for v in values])
    moments = np.array([[[v[:, d, 0].sum(), (v[:, d, 0] ** 2).sum(), v[:, d, 1].sum(), (v[:, d, 1] ** 2).sum()] for d in range(D)] for v in values])
    hist_nb = np.zeros((2, 33), np.int64)
    hist_nb[0, 12], hist_nb[1, 11], hist_nb[1, 12] = 12, 8, 12
    series_counts = np.array([[4, 1, 4], [6, 2, 5], [8, 1, 8]])
    series_order = rng.uniform(0, 1, (cap, 2, D))
    out = local_order_from_sums(hist_q, hist_qbar, hist_nb, moments, series_counts, series_order, n_samples, counts, 10, 2.0)
    for a, v in enumerate(values):
        assert np.allclose(out["q_mean"][a], v[:, :, 0].mean(axis=0)) and np.allclose(out["q_var"][a], v[:, :, 0].var(axis=0))
        assert np.allclose(out["qbar_mean"][a], v[:, :, 1].mean(axis=0)) and np.allclose(out["qbar_var"][a], v[:, :, 1].var(axis=0))
    assert np.allclose(out["q_hist"].sum(axis=-1) / bins, 1) and np.allclose(out["qbar_hist"].sum(axis=-1) / bins, 1)
    assert np.allclose(out["bin_centres"], np.arange(bins) / bins + 0.05) and np.allclose(out["coordination_hist"].sum(axis=-1), 1)
    assert out["coordination_hist"][1, 11] == 0.4
    assert list(out["step"]) == [0, 10, 20] and list(out["time"]) == [0, 20, 40] and list(out["n_solid"]) == [4, 6, 8]   # the cap
    assert np.allclose(out["solid_fraction"], [0.5, 0.75, 1.0]) and list(out["largest_cluster"]) == [4, 5, 8]
    assert np.array_equal(out["Q"], series_order[:, 0]) and np.array_equal(out["mean_qbar"], series_order[:, 1])
    short = local_order_from_sums(hist_q, hist_qbar, hist_nb, moments, series_counts, series_order, 2, counts, 10, 2.0)
    assert list(short["n_clusters"]) == [1, 2]
    assert decode_flags(0) == dict(cell=False, range=False, neighbors=False, nonfinite=False)
    assert decode_flags(4 | 1) == dict(cell=True, range=False, neighbors=True, nonfinite=False)


def test_the_forms_of_r_cut_and_the_argument_checks():
    from torch_m3gnet.local_order import LocalOrderObservables, cutoffs_of

    z = [np.array([29, 29, 13]), np.array([13, 13, 29, 13]), np.array([29, 13])]
    assert list(cutoffs_of(3.0, z)) == [3.0, 3.0, 3.0] and list(cutoffs_of([3.0, 3.5, 2.0], z)) == [3.0, 3.5, 2.0]
    assert list(cutoffs_of({29: 3.1, 13: 3.4}, z)) == [3.1, 3.4, 3.4]   # the majority species; the smaller number among equals
    for bad in ([3.0, 3.5], {29: 3.1}, -1.0, [[3.0]]):
        with pytest.raises(ValueError):
            cutoffs_of(bad, z)
    obs = LocalOrderObservables({29: 3.1, 13: 3.4}, degrees=(6,), solid_degree=6)
    assert obs.degrees == (6,) and obs.sample_interval == 10 and obs.max_samples == 4096 and obs.hist_bins == 100
    for bad in (dict(r_cut=0.0), dict(r_cut=3.0, degrees=(4, 13)), dict(r_cut=3.0, degrees=(4, 4, 6)), dict(r_cut=3.0, degrees=(2, 4, 6, 8)),
                dict(r_cut=3.0, degrees=(4, 8)), dict(r_cut=3.0, solid_threshold=1.5), dict(r_cut=3.0, solid_bonds=0),
                dict(r_cut=3.0, solid_bonds=33), dict(r_cut=3.0, hist_bins=1025), dict(r_cut=3.0, sample_interval=0),
                dict(r_cut=3.0, max_samples=65537)):
        with pytest.raises(ValueError):
            LocalOrderObservables(**bad)
    with pytest.raises(ValueError, match="at most 4"):   # refused on the host, before any device is touched
        LocalOrderObservables(3.0).begin([np.eye(3) * 9.0], [np.arange(5) + 1], None, "cuda")


# ---- the export surface ------------------------------------------------------------------------------------------------------------
def test_header_prototypes_are_bound_and_exported_and_the_abi_version_stays():
    _l, lib = _lib()
    header = (ROOT / "include" / "m3gnet_hip.h").read_text()
    declared = set(re.findall(r"\b(m3g_lo_[a-z_]+)\s*\(", header))
    assert declared == {"m3g_lo_state_bytes", "m3g_lo_init", "m3g_lo_sample", "m3g_lo_read", "m3g_lo_frame"}
    for name in declared:
        assert re.search(rf"\bint {name}\(", header) and hasattr(lib, name) and name in _l.SYMBOLS, name
    assert "#define M3G_ABI_VERSION 11" in header and _l.ABI_VERSION == 11
    assert C.sizeof(_l.M3GLoSizes) == 32 and C.sizeof(_l.M3GLoParams) == 32
    for name, value in (("M3G_LO_MAX_DEGREE", _l.LO_MAX_DEGREE), ("M3G_LO_MAX_DEGREES", _l.LO_MAX_DEGREES),
                        ("M3G_LO_MAX_NEIGHBORS", _l.LO_MAX_NEIGHBORS), ("M3G_LO_MAX_SPECIES", _l.LO_MAX_SPECIES),
                        ("M3G_LO_MAX_BINS", _l.LO_MAX_BINS), ("M3G_LO_MAX_SERIES", _l.LO_MAX_SERIES), ("M3G_LO_CELL", _l.LO_CELL),
                        ("M3G_LO_RANGE", _l.LO_RANGE), ("M3G_LO_NEIGHBORS", _l.LO_NEIGHBORS), ("M3G_LO_NONFINITE", _l.LO_NONFINITE)):
        assert re.search(rf"#define {name} {value}\b", header), name
    assert (_l.LO_CELL, _l.LO_RANGE, _l.LO_NEIGHBORS, _l.LO_NONFINITE) == (ref.CELL, ref.RANGE, ref.NEIGHBORS, ref.NONFINITE)
    assert _l.LO_MAX_NEIGHBORS == ref.MAX_NEIGHBORS and _l.LO_MAX_DEGREE + 1 == ref.ORDERS


# ---- refusals: all of them answered on the host, before any HIP call -------------------------------------------------------------------
N, S = 3, 1


def _sizes(**kw):
    _l, _ = _lib()
    return _l.M3GLoSizes(**{**dict(n_atoms=N, n_structs=S, max_species=2, n_degrees=2, hist_bins=10, series_cap=4), **kw})


def _params(degrees=(4, 6, 0), solid_degree=6, solid_bonds=7, solid_threshold=0.5):
    _l, _ = _lib()
    return _l.M3GLoParams((C.c_int32 * 3)(*degrees), solid_degree, solid_bonds, solid_threshold)


def _state_bytes(sizes):
    _, lib = _lib()
    n = C.c_size_t()
    assert lib.m3g_lo_state_bytes(C.byref(sizes), C.byref(n)) == M3G_OK
    return n.value


def _init(**over):
    _, lib = _lib()
    a = dict(sizes=_sizes(), params=_params(), offsets=np.array([0, N], np.int64), species=np.array([0, 1, 0], np.int32),
             r_cut=np.array([3.0]), state=DUMMY, nbytes=BIG)
    a.update(over)
    ptr = lambda x: None if x is None else x.ctypes.data
    rc = lib.m3g_lo_init(C.byref(a["sizes"]), C.byref(a["params"]), ptr(a["offsets"]), ptr(a["species"]), ptr(a["r_cut"]), a["state"],
                         a["nbytes"], None)
    return rc, lib.m3g_last_error().decode()


def test_init_refusals_are_pinned():
    need = _state_bytes(_sizes())
    cases = [
        (dict(state=None), M3G_ERR_VALUE, "m3g_lo_init: null argument"),
        (dict(r_cut=None), M3G_ERR_VALUE, "m3g_lo_init: null argument"),
        (dict(species=None), M3G_ERR_VALUE, "m3g_lo_init: null argument"),
        (dict(nbytes=need - 1), M3G_ERR_SIZE, f"m3g_lo_init: state buffer too small ({need - 1} < {need})"),
        (dict(sizes=_sizes(n_atoms=0)), M3G_ERR_VALUE, "m3g_lo_init: bad sizes"),
        (dict(sizes=_sizes(max_species=5)), M3G_ERR_VALUE, "m3g_lo_init: max_species must be 1 .. 4"),
        (dict(sizes=_sizes(n_degrees=4)), M3G_ERR_VALUE, "m3g_lo_init: n_degrees must be 1 .. 3"),
        (dict(sizes=_sizes(n_degrees=0)), M3G_ERR_VALUE, "m3g_lo_init: n_degrees must be 1 .. 3"),
        (dict(sizes=_sizes(hist_bins=1025)), M3G_ERR_VALUE, "m3g_lo_init: hist_bins must be 1 .. 1024"),
        (dict(sizes=_sizes(series_cap=0)), M3G_ERR_VALUE, "m3g_lo_init: series_cap must be 1 .. 65536"),
        (dict(sizes=_sizes(series_cap=65537)), M3G_ERR_VALUE, "m3g_lo_init: series_cap must be 1 .. 65536"),
        (dict(params=_params(degrees=(4, 13, 0), solid_degree=4)), M3G_ERR_VALUE, "m3g_lo_init: every degree must be 1 .. 12"),
        (dict(params=_params(degrees=(0, 6, 0))), M3G_ERR_VALUE, "m3g_lo_init: every degree must be 1 .. 12"),
        (dict(params=_params(degrees=(6, 6, 0))), M3G_ERR_VALUE, "m3g_lo_init: the degrees must be distinct"),
        (dict(params=_params(solid_degree=8)), M3G_ERR_VALUE, "m3g_lo_init: solid_degree must be one of the degrees"),
        (dict(params=_params(solid_bonds=0)), M3G_ERR_VALUE, "m3g_lo_init: solid_bonds must be 1 .. 32"),
        (dict(params=_params(solid_bonds=33)), M3G_ERR_VALUE, "m3g_lo_init: solid_bonds must be 1 .. 32"),
        (dict(params=_params(solid_threshold=float("nan"))), M3G_ERR_VALUE, "m3g_lo_init: solid_threshold must be -1 .. 1"),
        (dict(params=_params(solid_threshold=1.5)), M3G_ERR_VALUE, "m3g_lo_init: solid_threshold must be -1 .. 1"),
        (dict(offsets=np.array([0, N - 1], np.int64)), M3G_ERR_VALUE, "m3g_lo_init: offsets must run from 0 to n_atoms"),
        (dict(r_cut=np.array([0.0])), M3G_ERR_VALUE, "m3g_lo_init: r_cut of structure 0 is not finite and > 0"),
        (dict(r_cut=np.array([np.inf])), M3G_ERR_VALUE, "m3g_lo_init: r_cut of structure 0 is not finite and > 0"),
        (dict(species=np.array([0, 2, 0], np.int32)), M3G_ERR_VALUE, "m3g_lo_init: species index of atom 1 is outside 0 .. max_species - 1"),
    ]
    for over, status, message in cases:
        assert _init(**over) == (status, message), over
    # the third degree is ignored with n_degrees = 2, and the limits themselves pass (up to the size check)
    assert _init(params=_params(degrees=(12, 1, 99), solid_degree=12, solid_bonds=32, solid_threshold=-1.0), nbytes=need - 1)[0] == M3G_ERR_SIZE
    _, lib = _lib()
    assert lib.m3g_lo_init(None, C.byref(_params()), None, None, None, DUMMY, BIG, None) == M3G_ERR_VALUE
    assert lib.m3g_last_error().decode() == "m3g_lo_init: null sizes or parameters"


def test_sample_read_and_frame_refusals_are_pinned():
    _, lib = _lib()
    sizes, params = _sizes(), _params()
    need = _state_bytes(sizes)
    z, p = C.byref(sizes), C.byref(params)
    err = lambda: lib.m3g_last_error().decode()
    assert lib.m3g_lo_state_bytes(z, None) == M3G_ERR_VALUE and err() == "m3g_lo_state_bytes: null argument"
    assert lib.m3g_lo_state_bytes(None, None) == M3G_ERR_VALUE and err() == "m3g_lo_state_bytes: null sizes or parameters"
    assert lib.m3g_lo_sample(z, p, None, BIG, DUMMY, DUMMY, None) == M3G_ERR_VALUE and err() == "m3g_lo_sample: null argument"
    assert lib.m3g_lo_sample(z, p, DUMMY, BIG, DUMMY, None, None) == M3G_ERR_VALUE and err() == "m3g_lo_sample: null argument"
    assert lib.m3g_lo_sample(z, None, DUMMY, BIG, DUMMY, DUMMY, None) == M3G_ERR_VALUE and err() == "m3g_lo_sample: null sizes or parameters"
    assert lib.m3g_lo_sample(z, C.byref(_params(solid_degree=5)), DUMMY, BIG, DUMMY, DUMMY, None) == M3G_ERR_VALUE
    assert err() == "m3g_lo_sample: solid_degree must be one of the degrees"
    assert lib.m3g_lo_sample(z, p, DUMMY, need - 1, DUMMY, DUMMY, None) == M3G_ERR_SIZE and err() == "m3g_lo_sample: state buffer too small"
    assert lib.m3g_lo_read(z, None, BIG, *[None] * 9, None) == M3G_ERR_VALUE and err() == "m3g_lo_read: null argument"
    assert lib.m3g_lo_read(z, DUMMY, need - 1, *[None] * 9, None) == M3G_ERR_SIZE and err() == "m3g_lo_read: state buffer too small"
    assert lib.m3g_lo_read(C.byref(_sizes(hist_bins=0)), DUMMY, BIG, *[None] * 9, None) == M3G_ERR_VALUE
    assert err() == "m3g_lo_read: hist_bins must be 1 .. 1024"
    assert lib.m3g_lo_frame(z, None, BIG, *[None] * 7, None) == M3G_ERR_VALUE and err() == "m3g_lo_frame: null argument"
    assert lib.m3g_lo_frame(z, DUMMY, need - 1, *[None] * 7, None) == M3G_ERR_SIZE and err() == "m3g_lo_frame: state buffer too small"


def test_state_bytes_grow_with_each_size():
    base = dict(n_atoms=1272, n_structs=7, max_species=3, n_degrees=2, hist_bins=20, series_cap=3)
    small = _state_bytes(_sizes(**base))
    assert small % 256 == 0
    for key, more in (("n_atoms", 1272 + 256), ("n_structs", 8), ("max_species", 4), ("n_degrees", 3), ("hist_bins", 200), ("series_cap", 300)):
        assert _state_bytes(_sizes(**{**base, key: more})) > small, key
    # the lists and the frame: 936 + 224 n_degrees bytes per atom
    assert _state_bytes(_sizes(**{**base, "n_atoms": 1272 + 2560})) - small >= 2560 * (936 + 224 * 2)


# ---- the driver's argument -----------------------------------------------------------------------------------------------------------
def test_observables_argument_of_run_with_local_order(monkeypatch):
    from torch_m3gnet import dynamics
    from torch_m3gnet.dynamics import MolecularDynamics, _split_observables, _take_local_order
    from torch_m3gnet.local_order import LocalOrderObservables
    from torch_m3gnet.scattering import ScatteringObservables
    from torch_m3gnet.trajectory import TrajectoryObservables

    traj, sq, lo = TrajectoryObservables(rdf_bins=10), ScatteringObservables(q_max=2.0), LocalOrderObservables(3.0)
    assert _split_observables(None) == (None, None)
    assert _take_local_order(None) == (None, None) and _take_local_order(lo) == (lo, None) and _take_local_order(traj) == (None, traj)
    assert _take_local_order([sq, lo, traj]) == (lo, [sq, traj]) and _take_local_order((lo,)) == (lo, []) and _take_local_order([sq]) == (None, [sq])
    assert _split_observables(_take_local_order([lo, sq, traj])[1]) == (traj, sq)

    class Reached(Exception):
        pass

    def stop(*args, **kwargs):   # the first thing run() does once the argument and the ensemble have been accepted
        raise Reached

    monkeypatch.setattr(dynamics, "integer", stop)
    lat, pos, z = np.eye(3) * 7.2, np.random.default_rng(0).uniform(0, 7.2, (32, 3)), np.full(32, 29)
    md = MolecularDynamics.__new__(MolecularDynamics)   # (run() looks at `observables` before it looks at anything else of the driver)
    for ensemble in ("nve", "nvt_langevin", "npt_mtk", "npt_mtk_cell"):
        md.ensemble = ensemble
        for obs in (lo, [lo], (lo,)):
            with pytest.raises(Reached):
                md.run([lat], [pos], [z], 2, observables=obs)
    md.ensemble = "nve"
    for obs in ([lo, traj], [sq, lo], [traj, lo, sq], traj, None):
        with pytest.raises(Reached):
            md.run([lat], [pos], [z], 2, observables=obs)
    with pytest.raises(TypeError, match="a second LocalOrderObservables"):
        md.run([lat], [pos], [z], 2, observables=[lo, traj, LocalOrderObservables(2.5)])
    with pytest.raises(TypeError, match="a second TrajectoryObservables"):
        md.run([lat], [pos], [z], 2, observables=[traj, lo, traj])
    with pytest.raises(TypeError, match="got int"):
        md.run([lat], [pos], [z], 2, observables=[lo, 3])
    for ensemble in ("npt_mtk", "npt_mtk_cell"):   # the refusal keeps applying to the other two kinds, beside local order too
        md.ensemble = ensemble
        for obs in ([lo, traj], [sq, lo], traj):
            with pytest.raises(ValueError, match=f"observables are not supported with {ensemble}"):
                md.run([lat], [pos], [z], 2, observables=obs)
