"""Thermo observables without a GPU: the restatement (tests/thermo_reference.py) against closed forms (a cosine stress series, rows of
a known covariance, the strain of a scaled and of a sheared cell); the shape of the test batch (tests/thermo_cases.py) and the margin
the GPU test allows the device, held to a second fp64 evaluation; the host post-processing on synthetic accumulators; the export
surface; every refusal of the C ABI that precedes its first HIP call (status and message pinned, as tests/test_entry_refusals_cpu.py
does); and the `observables` argument of MolecularDynamics.run."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import thermo_cases as tc
import thermo_reference as ref

ROOT = Path(__file__).resolve().parent.parent
DUMMY, BIG = C.c_void_p(256), 1 << 30
M3G_OK, M3G_ERR_VALUE, M3G_ERR_SIZE = 0, 1, 3
KB = 8.617333262e-5


def _lib():
    from torch_m3gnet import _lib as l

    return l, l.load_library()


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def test_cosine_stress_series_gives_the_known_lag_sums_and_running_integral():
    from torch_m3gnet.thermo import EV_FS_A3_TO_MPA_S, stress_correlations

    n, G, theta = 40, 8, 2.0 * np.pi / 16.0
    acc = ref.Accumulator([1.0], 0.0, np.eye(3) * 5.0, G, False, np.longdouble)
    for k in range(n):
        tensor = np.zeros(6)
        tensor[5] = np.cos(theta * k)
        acc.sample(-1.0, np.zeros(6), np.eye(3) * 5.0, kinetic=0.5, tensor=tensor)
    lag = np.arange(G)
    # sum_{k=l}^{n-1} cos(theta k) cos(theta (k - l)) = (n - l) cos(theta l) / 2 + sin((n - l) theta) cos((n - 1) theta) / (2 sin theta)
    want = 0.5 * (n - lag) * np.cos(theta * lag) + 0.5 * np.sin((n - lag) * theta) * np.cos((n - 1) * theta) / np.sin(theta)
    assert np.array_equal(acc.lag_count, n - lag)
    assert np.abs(acc.lag_uu[:, 5].astype(np.float64) - want).max() < 1e-12
    assert np.abs(acc.lag_now[:, 5].astype(np.float64) - [np.cos(theta * np.arange(l, n)).sum() for l in lag]).max() < 1e-12
    assert np.abs(acc.lag_old[:, 5].astype(np.float64) - [np.cos(theta * np.arange(0, n - l)).sum() for l in lag]).max() < 1e-12
    assert (acc.lag_uu[:, :5] == 0).all() and (acc.lag_uu[:, 6] == 0).all()
    # an ideal ACF <P_xy P_xy'> = cos(theta l) / 2 without means: shear ACF = 2 c_xy / 10, and the trapezoid rule integrates a cosine
    # to dt cot(theta / 2) sin(theta l) / 2
    count = np.full(G, 100)
    uu = np.zeros((G, 7))
    uu[:, 5] = 100 * 0.5 * np.cos(theta * lag)
    dt, vol, temp = 2.0, 125.0, 300.0
    out = stress_correlations(uu, np.zeros((G, 7)), np.zeros((G, 7)), count, vol, temp, dt, plateau_window=(0.5, 1.0))
    assert np.abs(out["shear_acf"] - np.cos(theta * lag) / 10.0).max() < 1e-15 and (out["bulk_acf"] == 0).all()
    eta = vol / (KB * temp) * EV_FS_A3_TO_MPA_S * 0.1 * dt * 0.5 / np.tan(0.5 * theta) * np.sin(theta * lag)
    assert np.abs(out["eta_shear"] - eta).max() < 1e-12 * np.abs(eta).max() and out["eta_shear"][0] == 0
    assert np.array_equal(out["time"], lag * dt) and np.isclose(out["viscosity_shear"], eta[lag * dt >= 0.5 * (G - 1) * dt].mean(), rtol=1e-12)
    assert EV_FS_A3_TO_MPA_S == pytest.approx(1.602176634e-4 * 1e3)


def test_rows_of_a_known_covariance_give_it_back():
    from torch_m3gnet.thermo import covariance

    rng = np.random.default_rng(5)
    B = rng.normal(size=(ref.ROW, ref.ROW))
    sigma, mu = B @ B.T, rng.normal(size=ref.ROW) * 10.0
    rows = rng.multivariate_normal(mu, sigma, size=4000)
    mean, co, n = ref.welford(rows)
    cov = covariance(co, n)
    two_pass = np.cov(rows.T, bias=True)
    assert np.abs(mean - rows.mean(axis=0)).max() < 1e-12 and np.abs(cov - two_pass).max() < 1e-11 * np.abs(two_pass).max()
    assert np.array_equal(cov, cov.T) and np.abs(cov - sigma).max() < 0.1 * np.abs(sigma).max()   # (4000 draws: a few per cent)
    # a constant offset does not reach the co-moments: the reason for Welford's form
    assert np.abs(covariance(ref.welford(rows + 1e6)[1], n) - two_pass).max() < 1e-6 * np.abs(two_pass).max()


def test_strain_of_a_scaled_and_of_a_sheared_cell():
    L0 = np.array([[4.0, 0.3, 0.0], [0.2, 5.0, 0.1], [-0.3, 0.4, 6.0]], dtype=np.longdouble)
    inv = ref.inverse(L0)
    assert np.abs((inv @ L0).astype(np.float64) - np.eye(3)).max() < 1e-15
    eps, _ = ref.strain(L0 * np.longdouble(1.01), inv)
    assert np.abs(eps[:3].astype(np.float64) - 0.5 * (1.01 ** 2 - 1)).max() < 1e-15 and np.abs(eps[3:].astype(np.float64)).max() < 1e-15
    gamma = 0.02
    F = np.eye(3)
    F[0, 1] = gamma   # x += gamma y
    eps, _ = ref.strain(L0 @ F.T.astype(np.longdouble), inv)   # rows are lattice vectors: L = L0 F^T, E = (F^T F - 1) / 2
    want = 0.5 * (F.T @ F - np.eye(3))
    assert np.abs(eps.astype(np.float64) - [want[i, j] for i, j in ref.VOIGT]).max() < 1e-15
    assert want[0, 1] == gamma / 2 and np.isclose(want[1, 1], gamma ** 2 / 2)
    # a rigid rotation of the cell strains nothing; a left-handed cell has a positive volume
    c, s = np.cos(0.3), np.sin(0.3)
    R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])
    assert np.abs(ref.strain(L0 @ R.T.astype(np.longdouble), inv)[0].astype(np.float64)).max() < 1e-15
    assert ref.volume(L0[[1, 0, 2]]) == ref.volume(L0) > 0


def test_one_atom_two_sources_and_the_skip_rule():
    acc = ref.Accumulator([10.0], 0.01, np.eye(3) * 4.0, 2, False, np.float64)
    v = np.array([[0.01, -0.02, 0.03]])
    x, u, _, _, bad = acc.form(np.float32(-2.0), np.full(6, 0.001, np.float32), np.eye(3) * 4.0, vel=v)
    K = 10.0 * np.outer(v[0], v[0]) / ref.KAPPA
    assert not bad and np.isclose(x[1], 0.5 * np.trace(K)) and x[2] == 64.0 and np.isclose(x[3], x[0] + x[1] + 0.01 * 64.0)
    assert np.allclose(u[:6], np.float32(0.001) + np.array([K[i, j] for i, j in ref.VOIGT]) / 64.0) and np.isclose(u[6], u[:3].mean())
    assert np.isclose(x[4], u[6]) and (x[5:] == 0).all()
    # mode (b) fed that ke and tensor forms the same row; without the tensor the scalar pressure of the integrators
    xb, ub, _, _, _ = acc.form(np.float32(-2.0), np.full(6, 0.001, np.float32), np.eye(3) * 4.0, kinetic=x[1], tensor=u[:6])
    assert np.array_equal(xb, x) and np.array_equal(ub, u)
    x0, u0, _, _, _ = acc.form(np.float32(-2.0), np.full(6, 0.001, np.float32), np.eye(3) * 4.0, kinetic=x[1])
    assert u0 is None and np.isclose(x0[4], x[4]) and np.array_equal(x0[:4], x[:4])
    # remove_com: one atom has no kinetic energy about its centre of mass (a difference of two equal terms: a few roundings of one)
    com = ref.Accumulator([10.0], 0.0, np.eye(3) * 4.0, 0, True, np.float64)
    assert abs(com.form(np.float32(-2.0), np.zeros(6, np.float32), np.eye(3) * 4.0, vel=v)[0][1]) <= 4 * np.finfo(np.float64).eps * x[1]
    with pytest.raises(ValueError):
        acc.form(np.float32(0), np.zeros(6), np.eye(3), vel=v, kinetic=1.0)
    with pytest.raises(ValueError):
        acc.form(np.float32(0), np.zeros(6), np.eye(3))
    # good, good, NaN, good: the NaN enters nothing and empties the ring
    for e in (-2.0, -2.1, np.nan, -2.2):
        acc.sample(np.float32(e), np.zeros(6, np.float32), np.eye(3) * 4.0, vel=v)
    assert (acc.n_samples, acc.n_skipped, acc.flags) == (3, 1, ref.NONFINITE) and acc.lag_count.tolist() == [3, 1] and len(acc.ring) == 1
    assert np.isclose(float(acc.mean[0]), np.mean(np.float32([-2.0, -2.1, -2.2]).astype(np.float64))) and np.isfinite(acc.comoments).all()
    assert np.isnan(acc.ring_entry(1)).all() and np.array_equal(acc.ring_entry(0), acc.tensors[-1])


def test_the_batch_and_its_reference():
    assert tc.long_double_is_wider()
    b = tc.batch()
    assert [int(b["offsets"][s + 1] - b["offsets"][s]) for s in range(4)] == tc.SIZES == [1, 2, 257, 600]
    assert np.linalg.det(b["cells"][1]) < 0 and len(b["frames"]) == tc.N_FRAMES == 11 > 2 * tc.N_LAGS
    assert all(not np.array_equal(b["frames"][k]["lattice"], b["frames"][k + 1]["lattice"]) for k in range(10))
    hi = tc.reference("longdouble")
    assert [a.n_samples for a in hi] == [11, 11, 10, 11] and [a.n_skipped for a in hi] == [0, 0, 1, 0] and [a.flags for a in hi] == [0, 0, 1, 0]
    assert [a.lag_count.tolist() for a in hi] == [[11, 10, 9, 8]] * 2 + [[10, 8, 6, 4]] + [[11, 10, 9, 8]]
    assert hi[2].skipped == [k == 5 for k in range(11)] and hi[1].rows[0][2] > 0
    one = tc.reference("longdouble", n_lags=1)
    assert [a.lag_count.tolist() for a in one] == [[11], [11], [10], [11]]
    assert all(np.array_equal(a.mean, c.mean) and np.array_equal(a.comoments, c.comoments) for a, c in zip(hi, tc.reference("longdouble", n_lags=0)))
    com = tc.reference("longdouble", remove_com=True)
    assert abs(float(com[0].rows[0][1])) <= 4 * np.finfo(np.float64).eps * float(hi[0].rows[0][1]) and float(com[3].rows[0][1]) < float(hi[3].rows[0][1])


def test_margin_covers_another_fp64_evaluation():
    """A second fp64 evaluation of the reference, every sum backwards, stays within a quarter of MARGIN of the long-double one in the
    units the device is held to (measured here: at most 1.6 units)."""
    for remove_com in (False, True):
        for name in tc.QUANTITIES:
            one = tc.unit(name, remove_com=remove_com)
            dev = tc.deviation(tc.reference("float64", reverse=True, remove_com=remove_com), name, remove_com=remove_com)
            assert one > 0 and tc.within(dev, one, tc.MARGIN / 4), (remove_com, name, dev, one)


# ---- the host post-processing on synthetic accumulators -------------------------------------------------------------------------------
def _comoments(cov, n):
    return (np.asarray(cov) * n)[np.triu_indices(ref.ROW)]


def test_fluctuation_formulas_on_synthetic_accumulators():
    from torch_m3gnet._driver import EV_A3_TO_GPA
    from torch_m3gnet.thermo import thermo_from_moments

    n_atoms, n, temp = 100, 50, 300.0
    ke = 1.5 * n_atoms * KB * temp
    mean = np.array([-350.0, ke, 1200.0, -340.0, 0.001, 0.01, 0.01, 0.01, 0.0, 0.0, 0.0])
    cov = np.zeros((ref.ROW, ref.ROW))
    cov[0, 0], cov[1, 1], cov[0, 1], cov[2, 2], cov[3, 3], cov[2, 3] = 0.04, 0.02, 0.005, 9.0, 0.09, 0.3
    cov[1, 0], cov[3, 2] = cov[0, 1], cov[2, 3]
    var_e = np.array([1e-5, 2e-5, 3e-5, 4e-6, 5e-6, 6e-6])   # of the tensor strain components
    cov[5:, 5:] = np.diag(var_e)
    co = _comoments(cov, n)
    out = thermo_from_moments(mean, co, n, n_atoms, "npt_mtk_cell")
    assert np.isclose(out["t"], temp) and out["p"] == 0.001 * EV_A3_TO_GPA and out["v"] == 1200.0 and np.array_equal(out["strain"], mean[5:])
    assert np.isclose(out["heat_capacity"], 0.09 / (KB * temp ** 2)) and np.isclose(out["heat_capacity_kb"], out["heat_capacity"] / (100 * KB))
    assert np.isclose(out["compressibility"], 9.0 / (KB * temp * 1200.0) / EV_A3_TO_GPA) and np.isclose(out["bulk_modulus"], 1.0 / out["compressibility"])
    assert np.isclose(out["thermal_expansion"], 0.3 / (KB * temp ** 2 * 1200.0))
    # a diagonal Cov(e), e the Voigt strain (2 eps for the shears): C_ii = kB T / (<V> Var(e_i))
    voigt_var = var_e * np.array([1, 1, 1, 4, 4, 4])
    assert np.allclose(np.diag(out["elastic_constants"]), KB * temp / (1200.0 * voigt_var) * EV_A3_TO_GPA, rtol=1e-12)
    assert np.abs(out["elastic_constants"] - np.diag(np.diag(out["elastic_constants"]))).max() < 1e-9
    ortho = thermo_from_moments(mean, co, n, n_atoms, "npt_mtk_cell", cell_mask="orthorhombic")["elastic_constants"]
    assert np.allclose(np.diag(ortho)[:3], np.diag(out["elastic_constants"])[:3]) and np.isnan(ortho[3:, :]).all() and np.isnan(ortho[:, 3:]).all()
    iso = thermo_from_moments(mean, co, n, n_atoms, "npt_mtk")
    assert iso["elastic_constants"] is None and np.isclose(iso["bulk_modulus"], out["bulk_modulus"])
    for ensemble in ("nvt_langevin", "nvt_nose_hoover"):
        nvt = thermo_from_moments(mean, co, n, n_atoms, ensemble)
        assert np.isclose(nvt["heat_capacity"], (0.04 + 0.02 + 2 * 0.005) / (KB * temp ** 2)) and nvt["compressibility"] is None
        assert nvt["thermal_expansion"] is None and nvt["bulk_modulus"] is None and nvt["elastic_constants"] is None
    # NVE: Var(ke) of a harmonic solid, (3 N kB^2 T^2 / 2)(1 - 3 N kB / (2 C_v)) with C_v = 3 N kB, gives C_v back
    g = 3.0 * n_atoms
    cov_nve = cov.copy()
    cov_nve[1, 1] = 0.5 * g * KB ** 2 * temp ** 2 * (1.0 - g * KB / (2.0 * g * KB))
    nve = thermo_from_moments(mean, _comoments(cov_nve, n), n, n_atoms, "nve")
    assert np.isclose(nve["heat_capacity"], g * KB) and np.isclose(nve["heat_capacity_kb"], 3.0)
    for ensemble in ("nvt_berendsen", "npt_berendsen", None):   # no ensemble's fluctuations: the means only
        ber = thermo_from_moments(mean, co, n, n_atoms, ensemble)
        assert all(ber[key] is None for key in ("heat_capacity", "heat_capacity_kb", "compressibility", "bulk_modulus", "thermal_expansion",
                                                "elastic_constants")) and np.isclose(ber["t"], temp)
    # remove_com: g = 3 n - 3
    assert np.isclose(thermo_from_moments(mean, co, n, n_atoms, "nve", remove_com=True)["t"], temp * 300.0 / 297.0)
    assert np.array_equal(out["covariance"], cov)


def test_daivis_evans_weights_and_mean_subtraction():
    from torch_m3gnet.thermo import running_integral, stress_correlations

    rng = np.random.default_rng(2)
    G, k = 6, 50
    c = rng.uniform(0.5, 1.0, (G, 7))
    now, old = rng.normal(size=(G, 7)), rng.normal(size=(G, 7))
    count = np.full(G, k)
    uu = (c + now * old) * k
    out = stress_correlations(uu, now * k, old * k, count, 1000.0, 300.0, 1.0, plateau_window=(0.0, 1.0))
    assert np.allclose(out["tensor_acf"], c, rtol=1e-12)
    assert np.allclose(out["shear_acf"], (c[:, :3].sum(1) + 2 * c[:, 3:6].sum(1) - 3 * c[:, 6]) / 10.0) and np.allclose(out["bulk_acf"], c[:, 6])
    assert np.allclose(running_integral([1.0, 1.0, 3.0], 2.0), [0.0, 2.0, 6.0])
    assert np.isclose(out["viscosity_bulk"], out["eta_bulk"].mean())
    short = stress_correlations(uu, now * k, old * k, np.array([k] * 5 + [0]), 1000.0, 300.0, 1.0)
    assert np.isnan(short["viscosity_shear"])   # a lag of the window has no sample yet


def test_observables_object_checks_its_arguments():
    from torch_m3gnet.thermo import ThermoObservables

    obs = ThermoObservables()
    assert (obs.n_lags, obs.sample_interval, obs.remove_com, obs.plateau_window, obs.reference_cells) == (0, 1, False, (0.5, 1.0), None)
    for bad in (dict(n_lags=-1), dict(n_lags=4097), dict(sample_interval=0), dict(remove_com=1), dict(plateau_window=(0.5, 0.5)),
                dict(plateau_window=(-0.1, 1.0)), dict(plateau_window=(0.2, 1.5))):
        with pytest.raises(ValueError):
            ThermoObservables(**bad)
    with pytest.raises(ValueError, match="reference_cells"):
        ThermoObservables(reference_cells=np.zeros((2, 3, 3))).begin([np.eye(3)], [np.arange(3)], [np.ones(3)], "cuda")
    with pytest.raises(ValueError, match="not supported with npt_mtk"):
        ThermoObservables(n_lags=2).begin([np.eye(3)], [np.arange(3)], [np.ones(3)], "cuda", ensemble="npt_mtk")


# ---- the export surface ------------------------------------------------------------------------------------------------------------
def test_header_prototypes_are_bound_and_exported_and_the_abi_version_stays():
    _l, lib = _lib()
    header = (ROOT / "include" / "m3gnet_hip.h").read_text()
    declared = set(re.findall(r"\b(m3g_thermo_[a-z_]+)\s*\(", header))
    assert declared == {"m3g_thermo_state_bytes", "m3g_thermo_init", "m3g_thermo_sample", "m3g_thermo_read", "m3g_thermo_frame"}
    for name in declared:
        assert re.search(rf"\bint {name}\(", header) and hasattr(lib, name) and name in _l.SYMBOLS, name
    assert "#define M3G_ABI_VERSION 11" in header and _l.ABI_VERSION == 11
    assert re.search(r"additive, same version: m3g_thermo_state_bytes / _init / _sample / _read / _frame", header)
    assert C.sizeof(_l.M3GThermoSizes) == 24 and C.sizeof(_l.M3GThermoParams) == 4
    for name, value in (("M3G_THERMO_ROW", _l.THERMO_ROW), ("M3G_THERMO_COMOMENTS", _l.THERMO_COMOMENTS), ("M3G_THERMO_TENSOR", _l.THERMO_TENSOR),
                        ("M3G_THERMO_MAX_LAGS", _l.THERMO_MAX_LAGS), ("M3G_THERMO_NONFINITE", _l.THERMO_NONFINITE)):
        assert re.search(rf"#define {name} {value}\b", header), name
    assert (_l.THERMO_ROW, _l.THERMO_COMOMENTS, _l.THERMO_TENSOR, _l.THERMO_NONFINITE) == (ref.ROW, ref.COMOMENTS, ref.TENSOR, ref.NONFINITE)
    assert len(ref.TRIU) == ref.COMOMENTS and all(at == i * 11 - i * (i - 1) // 2 + (j - i) for at, (i, j) in enumerate(ref.TRIU))


# ---- refusals: all of them answered on the host, before any HIP call -------------------------------------------------------------------
N, S = 3, 1


def _sizes(**kw):
    _l, _ = _lib()
    return _l.M3GThermoSizes(**{**dict(n_atoms=N, n_structs=S, n_lags=2), **kw})


def _params(remove_com=0):
    _l, _ = _lib()
    return _l.M3GThermoParams(remove_com)


def _state_bytes(sizes):
    _, lib = _lib()
    n = C.c_size_t()
    assert lib.m3g_thermo_state_bytes(C.byref(sizes), C.byref(n)) == M3G_OK
    return n.value


def _init(**over):
    _, lib = _lib()
    a = dict(sizes=_sizes(), params=_params(), offsets=np.array([0, N], np.int64), masses=np.array([1.0, 2.0, 3.0]), p_ext=np.array([0.0]),
             cells=np.eye(3).reshape(1, 3, 3).copy(), state=DUMMY, nbytes=BIG)
    a.update(over)
    ptr = lambda x: None if x is None else x.ctypes.data
    rc = lib.m3g_thermo_init(C.byref(a["sizes"]), C.byref(a["params"]), ptr(a["offsets"]), ptr(a["masses"]), ptr(a["p_ext"]), ptr(a["cells"]),
                             a["state"], a["nbytes"], None)
    return rc, lib.m3g_last_error().decode()


def test_init_refusals_are_pinned():
    need = _state_bytes(_sizes())
    singular = np.eye(3).reshape(1, 3, 3).copy()
    singular[0, 1] = 0.0
    infinite = np.eye(3).reshape(1, 3, 3).copy()
    infinite[0, 2, 2] = np.inf
    cases = [
        (dict(state=None), M3G_ERR_VALUE, "m3g_thermo_init: null argument"),
        (dict(masses=None), M3G_ERR_VALUE, "m3g_thermo_init: null argument"),
        (dict(p_ext=None), M3G_ERR_VALUE, "m3g_thermo_init: null argument"),
        (dict(cells=None), M3G_ERR_VALUE, "m3g_thermo_init: null argument"),
        (dict(nbytes=need - 1), M3G_ERR_SIZE, f"m3g_thermo_init: state buffer too small ({need - 1} < {need})"),
        (dict(sizes=_sizes(n_atoms=0)), M3G_ERR_VALUE, "m3g_thermo_init: bad sizes"),
        (dict(sizes=_sizes(n_structs=4)), M3G_ERR_VALUE, "m3g_thermo_init: bad sizes"),
        (dict(sizes=_sizes(n_lags=-1)), M3G_ERR_VALUE, "m3g_thermo_init: n_lags must be 0 .. 4096"),
        (dict(sizes=_sizes(n_lags=4097)), M3G_ERR_VALUE, "m3g_thermo_init: n_lags must be 0 .. 4096"),
        (dict(params=_params(2)), M3G_ERR_VALUE, "m3g_thermo_init: remove_com must be 0 or 1"),
        (dict(offsets=np.array([0, N - 1], np.int64)), M3G_ERR_VALUE, "m3g_thermo_init: offsets must run from 0 to n_atoms"),
        (dict(masses=np.array([1.0, 0.0, 3.0])), M3G_ERR_VALUE, "m3g_thermo_init: mass of atom 1 is not finite and > 0"),
        (dict(masses=np.array([1.0, 2.0, np.nan])), M3G_ERR_VALUE, "m3g_thermo_init: mass of atom 2 is not finite and > 0"),
        (dict(p_ext=np.array([np.inf])), M3G_ERR_VALUE, "m3g_thermo_init: p_ext of structure 0 is not finite"),
        (dict(cells=singular), M3G_ERR_VALUE, "m3g_thermo_init: singular cell of structure 0"),
        (dict(cells=infinite), M3G_ERR_VALUE, "m3g_thermo_init: lattice of structure 0 is not finite"),
    ]
    for over, status, message in cases:
        assert _init(**over) == (status, message), over
    assert _init(sizes=_sizes(n_lags=4096), nbytes=need - 1)[0] == M3G_ERR_SIZE and _init(sizes=_sizes(n_lags=0), params=_params(1), nbytes=0)[0] == M3G_ERR_SIZE
    _, lib = _lib()
    assert lib.m3g_thermo_init(None, C.byref(_params()), None, None, None, None, DUMMY, BIG, None) == M3G_ERR_VALUE
    assert lib.m3g_last_error().decode() == "m3g_thermo_init: null sizes or parameters"


def _sample(lib, sizes, params, state=DUMMY, nbytes=BIG, energies=DUMMY, stresses=DUMMY, lattice=DUMMY, vel=None, forces=None, kick=0.0,
            kinetic=None, kinetic_stride=0, tensor=None, tensor_stride=0):
    rc = lib.m3g_thermo_sample(sizes, params, state, nbytes, energies, stresses, lattice, vel, forces, kick, kinetic, kinetic_stride, tensor,
                               tensor_stride, None)
    return rc, lib.m3g_last_error().decode()


def test_sample_read_and_frame_refusals_are_pinned():
    _, lib = _lib()
    sizes, params, no_lags = _sizes(), _params(), _sizes(n_lags=0)
    need = _state_bytes(sizes)
    z, p, z0 = C.byref(sizes), C.byref(params), C.byref(no_lags)
    err = lambda: lib.m3g_last_error().decode()
    assert lib.m3g_thermo_state_bytes(z, None) == M3G_ERR_VALUE and err() == "m3g_thermo_state_bytes: null argument"
    assert lib.m3g_thermo_state_bytes(None, None) == M3G_ERR_VALUE and err() == "m3g_thermo_state_bytes: null sizes or parameters"
    assert lib.m3g_thermo_state_bytes(C.byref(_sizes(n_lags=5000)), None) == M3G_ERR_VALUE and err() == "m3g_thermo_state_bytes: n_lags must be 0 .. 4096"
    value = lambda message: (M3G_ERR_VALUE, "m3g_thermo_sample: " + message)
    assert _sample(lib, z, None, vel=DUMMY) == value("null sizes or parameters")
    assert _sample(lib, z, C.byref(_params(3)), vel=DUMMY) == value("remove_com must be 0 or 1")
    for missing in ("state", "energies", "stresses", "lattice"):
        assert _sample(lib, z, p, vel=DUMMY, **{missing: None}) == value("null argument"), missing
    # the two sources of the kinetic part: exactly one
    assert _sample(lib, z, p) == value("exactly one of vel and kinetic must be given")
    assert _sample(lib, z, p, vel=DUMMY, kinetic=DUMMY, kinetic_stride=1) == value("exactly one of vel and kinetic must be given")
    assert _sample(lib, z, p, vel=DUMMY, tensor=DUMMY, tensor_stride=6) == value("pressure_tensor goes with kinetic, not with vel")
    assert _sample(lib, z, p, vel=DUMMY, forces=DUMMY, kick=float("nan")) == value("kick must be finite")
    assert _sample(lib, z, p, kinetic=DUMMY, kinetic_stride=1, forces=DUMMY) == value("forces go with vel, not with kinetic")
    assert _sample(lib, z, p, kinetic=DUMMY, kinetic_stride=0, tensor=DUMMY, tensor_stride=6) == value("kinetic_stride must be >= 1")
    assert _sample(lib, z, p, kinetic=DUMMY, kinetic_stride=1, tensor=DUMMY, tensor_stride=5) == value("tensor_stride must be >= 6")
    # no tensor in mode (b): no stress correlations
    assert _sample(lib, z, p, kinetic=DUMMY, kinetic_stride=1) == value("n_lags > 0 needs the pressure tensor (vel, or pressure_tensor beside kinetic)")
    small = (M3G_ERR_SIZE, "m3g_thermo_sample: state buffer too small")
    assert _sample(lib, z0, p, kinetic=DUMMY, kinetic_stride=1, nbytes=0) == small   # (n_lags = 0: accepted up to the size check)
    assert _sample(lib, z, p, vel=DUMMY, nbytes=need - 1) == small and _sample(lib, z, p, kinetic=DUMMY, kinetic_stride=6, tensor=DUMMY, tensor_stride=12, nbytes=1) == small
    assert lib.m3g_thermo_read(z, None, BIG, *[None] * 9, None) == M3G_ERR_VALUE and err() == "m3g_thermo_read: null argument"
    assert lib.m3g_thermo_read(z, DUMMY, need - 1, *[None] * 9, None) == M3G_ERR_SIZE and err() == "m3g_thermo_read: state buffer too small"
    assert lib.m3g_thermo_read(None, DUMMY, BIG, *[None] * 9, None) == M3G_ERR_VALUE and err() == "m3g_thermo_read: null sizes or parameters"
    out = np.zeros(7)
    assert lib.m3g_thermo_frame(z, None, BIG, 0, None, None, None) == M3G_ERR_VALUE and err() == "m3g_thermo_frame: null argument"
    assert lib.m3g_thermo_frame(z, DUMMY, need - 1, 0, None, None, None) == M3G_ERR_SIZE and err() == "m3g_thermo_frame: state buffer too small"
    assert lib.m3g_thermo_frame(z, DUMMY, BIG, 2, None, out.ctypes.data, None) == M3G_ERR_VALUE and err() == "m3g_thermo_frame: no ring entry 2 samples back (n_lags = 2)"
    assert lib.m3g_thermo_frame(z, DUMMY, BIG, -1, None, out.ctypes.data, None) == M3G_ERR_VALUE and err() == "m3g_thermo_frame: no ring entry -1 samples back (n_lags = 2)"
    assert lib.m3g_thermo_frame(z0, DUMMY, BIG, 0, None, out.ctypes.data, None) == M3G_ERR_VALUE and err() == "m3g_thermo_frame: no ring entry 0 samples back (n_lags = 0)"


def test_state_bytes_grow_with_each_size():
    base = dict(n_atoms=860, n_structs=4, n_lags=4)
    small = _state_bytes(_sizes(**base))
    assert small % 256 == 0
    for key, more in (("n_atoms", 860 + 256), ("n_structs", 40), ("n_lags", 64)):
        assert _state_bytes(_sizes(**{**base, key: more})) > small, key
    # the masses: 8 bytes per atom; a ring and three lag sums of 7 doubles and a count per lag and structure
    assert _state_bytes(_sizes(**{**base, "n_atoms": 860 + 2560})) - small >= 2560 * 8
    assert _state_bytes(_sizes(**{**base, "n_lags": 4 + 1024})) - small >= 4 * 1024 * (4 * 7 + 1) * 8


# ---- the driver's argument -----------------------------------------------------------------------------------------------------------
def test_observables_argument_of_run_with_thermo(monkeypatch):
    from torch_m3gnet import dynamics
    from torch_m3gnet.dynamics import MolecularDynamics, _split_observables, _take_local_order, _take_thermo
    from torch_m3gnet.local_order import LocalOrderObservables
    from torch_m3gnet.scattering import ScatteringObservables
    from torch_m3gnet.thermo import ThermoObservables
    from torch_m3gnet.trajectory import TrajectoryObservables

    traj, sq, lo, th = TrajectoryObservables(rdf_bins=10), ScatteringObservables(q_max=2.0), LocalOrderObservables(3.0), ThermoObservables()
    lagged = ThermoObservables(n_lags=8)
    assert _take_thermo(None) == (None, None) and _take_thermo(th) == (th, None) and _take_thermo(traj) == (None, traj)
    assert _take_thermo([sq, th, lo, traj]) == (th, [sq, lo, traj]) and _take_thermo((th,)) == (th, []) and _take_thermo([lo]) == (None, [lo])
    assert _take_local_order(_take_thermo([lo, th, sq])[1]) == (lo, [sq])
    assert _split_observables(_take_local_order(_take_thermo([lo, sq, th, traj])[1])[1]) == (traj, sq)

    class Reached(Exception):
        pass

    def stop(*args, **kwargs):   # the first thing run() does once the argument and the ensemble have been accepted
        raise Reached

    monkeypatch.setattr(dynamics, "integer", stop)
    lat, pos, z = np.eye(3) * 7.2, np.random.default_rng(0).uniform(0, 7.2, (32, 3)), np.full(32, 29)
    md = MolecularDynamics.__new__(MolecularDynamics)   # (run() looks at `observables` before it looks at anything else of the driver)
    for ensemble in ("nve", "nvt_langevin", "nvt_nose_hoover", "nvt_berendsen", "npt_berendsen", "npt_mtk", "npt_mtk_cell"):
        md.ensemble = ensemble
        for obs in (th, [th], (th,), [th, lo], [lo, th]):
            with pytest.raises(Reached):
                md.run([lat], [pos], [z], 2, observables=obs)
    md.ensemble = "nve"
    for obs in ([th, traj], [sq, th], [traj, lo, th, sq], lagged, [lagged, traj], traj, lo, None):
        with pytest.raises(Reached):
            md.run([lat], [pos], [z], 2, observables=obs)
    with pytest.raises(TypeError, match="a second ThermoObservables"):
        md.run([lat], [pos], [z], 2, observables=[th, traj, ThermoObservables(n_lags=2)])
    with pytest.raises(TypeError, match="a second LocalOrderObservables"):   # the texts of the other kinds stay
        md.run([lat], [pos], [z], 2, observables=[th, lo, LocalOrderObservables(2.5)])
    with pytest.raises(TypeError, match="a second TrajectoryObservables"):
        md.run([lat], [pos], [z], 2, observables=[traj, th, traj])
    with pytest.raises(TypeError, match="got int"):
        md.run([lat], [pos], [z], 2, observables=[th, 3])
    md.ensemble = "npt_mtk_cell"   # its integrator states the tensor
    with pytest.raises(Reached):
        md.run([lat], [pos], [z], 2, observables=lagged)
    md.ensemble = "npt_mtk"
    with pytest.raises(ValueError, match=r"ThermoObservables\(n_lags > 0\) is not supported with npt_mtk: its integrator states no pressure tensor"):
        md.run([lat], [pos], [z], 2, observables=[lo, lagged])
    for ensemble in ("npt_mtk", "npt_mtk_cell"):   # the refusal keeps applying to the velocity samplers, beside thermo too
        md.ensemble = ensemble
        for obs in ([th, traj], [sq, th]):
            with pytest.raises(ValueError, match=f"observables are not supported with {ensemble}"):
                md.run([lat], [pos], [z], 2, observables=obs)
