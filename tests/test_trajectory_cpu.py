"""CPU checks of the trajectory observables: the C ABI (m3g_traj_*) refusing bad arguments before touching a device, the host
post-processing of torch_m3gnet.trajectory on analytic accumulators and against the numpy restatement
(tests/trajectory_reference.py), and the argument checks of TrajectoryObservables / MolecularDynamics.run."""
import ctypes as C

import numpy as np
import pytest

import trajectory_reference as tr

FCC_BASE = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])


def _fcc(a, n):
    grid = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1).reshape(-1, 1, 3)
    return (grid + FCC_BASE[None]).reshape(-1, 3) * a, np.eye(3) * n * a


# ---- C ABI: refused before any HIP call -----------------------------------------------------------------------------------------------
def _init(sizes=(3, 2, 2, 16, 4), r_max=2.0, remove_com=1, offsets=(0, 1, 3), species=(0, 1, 0), masses=(1.0, 2.0, 3.0),
          state_bytes=1 << 30, null=()):
    from torch_m3gnet import _lib

    lib = _lib.load_library()
    sz, pr = _lib.M3GTrajSizes(*sizes), _lib.M3GTrajParams(r_max, remove_com)
    off, sp, m = np.array(offsets, np.int64), np.array(species, np.int32), np.array(masses, np.float64)
    dummy = C.c_void_p(256)   # never dereferenced: the call returns at the checks
    args = dict(sizes=C.byref(sz), params=C.byref(pr), offsets=off.ctypes.data, species=sp.ctypes.data, masses=m.ctypes.data, state=dummy)
    for name in null:
        args[name] = None
    return lib.m3g_traj_init(args["sizes"], args["params"], args["offsets"], args["species"], args["masses"], args["state"], state_bytes, None)


@pytest.mark.parametrize("case,word", [(dict(null=("sizes",)), b"null"), (dict(null=("params",)), b"null"), (dict(null=("offsets",)), b"null"),
                                       (dict(null=("species",)), b"null"), (dict(null=("masses",)), b"null"), (dict(null=("state",)), b"null"),
                                       (dict(sizes=(3, 2, 0, 16, 4)), b"max_species"), (dict(sizes=(3, 2, 9, 16, 4)), b"max_species"),
                                       (dict(sizes=(3, 2, 2, 4097, 4)), b"rdf_bins"), (dict(sizes=(3, 2, 2, -1, 4)), b"rdf_bins"),
                                       (dict(sizes=(3, 2, 2, 16, 4097)), b"n_lags"), (dict(sizes=(3, 2, 2, 0, 0)), b"nothing"),
                                       (dict(sizes=(0, 1, 2, 16, 4)), b"sizes"), (dict(sizes=(3, 4, 2, 16, 4)), b"sizes"),
                                       (dict(r_max=0.0), b"r_max"), (dict(r_max=-1.0), b"r_max"), (dict(r_max=float("nan")), b"r_max"),
                                       (dict(r_max=float("inf")), b"r_max"), (dict(remove_com=2), b"remove_com"),
                                       (dict(species=(0, 2, 0)), b"species"), (dict(species=(0, -1, 0)), b"species"),
                                       (dict(offsets=(0, 3, 3)), b"offsets"), (dict(offsets=(1, 2, 3)), b"offsets"), (dict(offsets=(0, 2, 4)), b"offsets"),
                                       (dict(masses=(1.0, 0.0, 3.0)), b"mass"), (dict(masses=(1.0, float("nan"), 3.0)), b"mass")])
def test_c_abi_refuses_bad_trajectory_arguments(case, word):
    from torch_m3gnet import _lib

    assert _init(**case) == _lib.M3G_ERR_VALUE
    assert word in _lib.load_library().m3g_last_error()


def test_c_abi_trajectory_sizes_and_abi_version():
    from torch_m3gnet import _lib

    lib = _lib.load_library()
    info = _lib.M3GInfo()
    assert lib.m3g_get_info(C.byref(info)) == 0 and info.abi_version == 11   # additive exports only
    assert _init(state_bytes=1) == _lib.M3G_ERR_SIZE   # valid arguments: only the state buffer is too small
    size, small = C.c_size_t(), C.c_size_t()
    big = _lib.M3GTrajSizes(10000, 1, 2, 200, 512)
    assert lib.m3g_traj_state_bytes(C.byref(big), C.byref(size)) == _lib.M3G_OK and size.value > 512 * 10000 * 48   # the ring
    assert lib.m3g_traj_state_bytes(C.byref(_lib.M3GTrajSizes(10000, 1, 2, 200, 0)), C.byref(small)) == _lib.M3G_OK
    assert small.value < 10 ** 6
    assert lib.m3g_traj_state_bytes(C.byref(big), None) == _lib.M3G_ERR_VALUE
    assert lib.m3g_traj_state_bytes(None, C.byref(size)) == _lib.M3G_ERR_VALUE
    dummy, pr = C.c_void_p(256), _lib.M3GTrajParams(2.0, 1)
    sz = _lib.M3GTrajSizes(3, 2, 2, 16, 4)
    sample = lambda **kw: lib.m3g_traj_sample(C.byref(sz), C.byref(kw.get("pr", pr)), kw.get("state", dummy), kw.get("bytes", 1 << 30),
                                              kw.get("pos", dummy), kw.get("lat", dummy), kw.get("vel", dummy), kw.get("f", None),
                                              kw.get("kick", 0.0), None)
    for bad in (dict(state=None), dict(pos=None), dict(lat=None), dict(vel=None), dict(f=dummy, kick=float("nan")),
                dict(pr=_lib.M3GTrajParams(0.0, 1))):
        assert sample(**bad) == _lib.M3G_ERR_VALUE, bad
    assert sample(bytes=1) == _lib.M3G_ERR_SIZE
    assert lib.m3g_traj_read(C.byref(sz), None, 1 << 30, None, None, None, None, None, None, None, None) == _lib.M3G_ERR_VALUE
    assert lib.m3g_traj_read(C.byref(sz), dummy, 1, None, None, None, None, None, None, None, None) == _lib.M3G_ERR_SIZE
    assert lib.m3g_traj_frame(C.byref(sz), dummy, 1 << 30, 0, None, dummy, None) == _lib.M3G_ERR_VALUE
    assert lib.m3g_traj_frame(C.byref(sz), dummy, 1, 0, dummy, dummy, None) == _lib.M3G_ERR_SIZE
    a, b = C.c_size_t(), C.c_size_t()
    assert lib.m3g_dyn_state_view(1000, 3, C.byref(a), C.byref(b)) == _lib.M3G_OK and a.value % 256 == 0 and b.value >= a.value + 8000
    assert lib.m3g_dyn_state_view(1000, 3, None, C.byref(b)) == _lib.M3G_ERR_VALUE
    assert lib.m3g_dyn_state_view(0, 1, C.byref(a), C.byref(b)) == _lib.M3G_ERR_VALUE
    assert C.sizeof(_lib.M3GTrajSizes) == 32 and C.sizeof(_lib.M3GTrajParams) == 16


# ---- host post-processing on analytic accumulators ----------------------------------------------------------------------------------
def test_fcc_counts_give_twelve_neighbours_and_the_pair_count():
    from torch_m3gnet.trajectory import pair_index, perpendicular_widths, rdf_from_counts

    a0, bins = 3.6, 180
    pos, lat = _fcc(a0, 3)   # 108 atoms, two species in a checkerboard of the base sites: 27 of species 1
    species = np.tile([1, 0, 0, 0], 27)
    counts = np.bincount(species)
    r_max = 0.999 * perpendicular_widths(lat).min() / 2
    H, _ = tr.histogram(pos, lat, species, r_max, bins, 2)
    n = 3   # as if three identical samples had been accumulated
    out = rdf_from_counts(n * H, counts, n, n * abs(np.linalg.det(lat)), r_max)
    ref = tr.normalise_rdf(n * H, counts, n, n * abs(np.linalg.det(lat)), r_max, 2)
    for a in range(2):
        for b in range(2):
            assert np.allclose(out["g"][a][b], ref["g"][a, b], rtol=1e-13, atol=0)
            assert np.allclose(out["coordination"][a][b], ref["coordination"][a, b], rtol=1e-13, atol=0)
    assert np.allclose(out["g_total"], ref["g_total"], rtol=1e-13, atol=0)
    edges = out["r_edges"]
    first = np.searchsorted(edges, 0.5 * (a0 / np.sqrt(2) + a0)) - 1   # between the first (a / sqrt 2) and second (a) shell
    total_cn = [out["coordination"][a][0][first] + out["coordination"][a][1][first] for a in range(2)]
    assert total_cn == [12.0, 12.0]
    assert out["coordination"][1][1][first] == 0.0 and out["coordination"][1][0][first] == 12.0   # species 1 sits on a simple cubic sublattice
    assert out["coordination"][0][1][first] == 4.0
    assert out["g_total"][: np.searchsorted(edges, 2.5) - 1].max() == 0.0
    peak = out["r"][np.argmax(out["g_total"])]
    assert abs(peak - a0 / np.sqrt(2)) < r_max / bins
    # g integrates back to the pair counts: sum_k g_ab v_k n N_a N_b / <V> = ordered pairs
    shell = 4 * np.pi / 3 * (edges[1:] ** 3 - edges[:-1] ** 3)
    vol = abs(np.linalg.det(lat))
    for a in range(2):
        for b in range(2):
            ordered = (out["g"][a][b] * shell).sum() * counts[a] * counts[b] / vol
            want = H[pair_index(a, b, 2)].sum() * (2 if a == b else 1)
            assert abs(ordered - want) < 1e-9 * max(want, 1)
    all_pairs = (out["g_total"] * shell).sum() * 108 ** 2 / vol / 2
    assert abs(all_pairs - H.sum()) < 1e-9 * H.sum()
    assert pair_index(1, 0, 3) == 1 and pair_index(1, 1, 3) == 3 and pair_index(2, 2, 3) == 5 and pair_index(7, 7, 8) == 35
    assert all(pair_index(a, b, 8) == tr.pair_index(a, b, 8) for a in range(8) for b in range(8))


def test_linear_msd_returns_the_diffusion_coefficient():
    from torch_m3gnet.trajectory import correlations_from_sums

    G, dt, D = 64, 2.0, np.array([3.7e-4, 1.1e-2])
    counts = np.array([5, 11])
    lag_count = np.arange(100, 100 - G, -1)
    t = np.arange(G) * dt
    msd = 6 * D[:, None] * t[None, :]
    out = correlations_from_sums(msd * counts[:, None] * lag_count[None, :], np.ones((2, G)) * counts[:, None] * lag_count[None, :], lag_count,
                                 counts, dt)
    assert np.abs(out["diffusion_msd"] / D - 1).max() < 1e-12
    assert np.abs(out["diffusion_msd_cm2_s"] / (0.1 * D) - 1).max() < 1e-12
    assert np.array_equal(out["time"], t) and np.abs(out["msd"] - msd).max() < 1e-12 * msd.max()
    # an offset does not change the slope, and vacf = const integrates to const * T / 3
    off = correlations_from_sums((msd + 5.0) * counts[:, None] * lag_count[None, :], np.ones((2, G)) * counts[:, None] * lag_count[None, :],
                                 lag_count, counts, dt, fit_window=(0.5, 1.0))
    assert np.abs(off["diffusion_msd"] / D - 1).max() < 1e-12
    assert np.abs(off["diffusion_vacf"] - t[-1] / 3).max() < 1e-12
    m_ref, v_ref = tr.normalise_correlations(msd * counts[:, None] * lag_count[None, :], np.ones((2, G)) * counts[:, None] * lag_count[None, :],
                                             lag_count, counts)
    assert np.allclose(out["msd"], m_ref, rtol=1e-14, atol=0) and np.allclose(out["vacf"], v_ref, rtol=1e-14, atol=0)


def test_ballistic_frames_give_v_squared_t_squared():
    from torch_m3gnet.trajectory import correlations_from_sums

    rng = np.random.default_rng(3)
    n, G, dt = 7, 6, 0.5
    species = np.array([0, 1, 0, 0, 1, 1, 0])
    v = rng.normal(0, 0.02, (n, 3))
    r0 = rng.uniform(0, 5, (n, 3))
    ref = tr.Correlations(np.ones(n), species, 2, G, remove_com=False)
    for k in range(10):
        ref.sample(r0 + v * (k * dt), v)
    assert list(ref.lag_count) == [10, 9, 8, 7, 6, 5]
    counts = np.bincount(species)
    out = correlations_from_sums(ref.msd, ref.vacf, ref.lag_count, counts, dt)
    for a in range(2):
        v2 = (v[species == a] ** 2).sum(1).mean()
        assert np.abs(out["msd"][a] - v2 * out["time"] ** 2).max() < 1e-12 * v2 * out["time"][-1] ** 2
        assert np.abs(out["vacf"][a] - v2).max() < 1e-13 * v2
    assert out["msd"][0][0] == 0.0


def test_cosine_vacf_puts_the_vdos_peak_at_its_frequency():
    from torch_m3gnet.trajectory import correlations_from_sums

    G, dt = 256, 1.0
    t = np.arange(G) * dt
    for f0 in (0.0123, 0.031, 0.11):   # 1/fs: 12.3, 31 and 110 THz
        vacf = 4e-4 * np.cos(2 * np.pi * f0 * t)
        out = correlations_from_sums(np.zeros((1, G)), vacf[None] * 3 * 7, np.full(G, 7), [3], dt)
        f = out["vdos_frequency"]
        assert abs(f[1] - f[0] - 1e3 / (2 * G * dt)) < 1e-9 and f[0] == 0.0
        k = int(np.argmax(out["vdos"][0]))
        assert k == int(np.rint(f0 * 1e3 / (f[1] - f[0]))), (f0, k)   # the bin that contains f0
        assert abs(np.trapezoid(vacf, t) / 3 - out["diffusion_vacf"][0]) < 1e-15


# ---- argument checks ------------------------------------------------------------------------------------------------------------------
def test_trajectory_observables_argument_validation():
    from torch_m3gnet.trajectory import TrajectoryObservables

    for kw in (dict(rdf_bins=-1), dict(rdf_bins=1.5), dict(rdf_bins=4097), dict(n_lags=-1), dict(n_lags=4097), dict(rdf_bins=0, n_lags=0),
               dict(rdf_r_max=0.0), dict(rdf_r_max=float("nan")), dict(sample_interval=0), dict(sample_interval=True), dict(remove_com=1),
               dict(fit_window=(0.8, 0.2)), dict(fit_window=(-0.1, 0.5)), dict(fit_window=(0.2, 1.5))):
        with pytest.raises(ValueError):
            TrajectoryObservables(**kw)
    pos, lat = _fcc(3.6, 2)
    z = np.full(32, 29)
    m = np.full(32, 63.546)
    with pytest.raises(ValueError, match="perpendicular width"):   # 3.6 A is the half-width: refused before any device call
        TrajectoryObservables(rdf_r_max=3.7).begin([lat], [z], [m], "cuda")
    tri = np.array([[7.2, 0, 0], [3.6, 7.2, 0], [0, 0, 7.2]])   # sheared: the perpendicular width along a0 shrinks to 6.44 A
    with pytest.raises(ValueError, match="perpendicular width"):
        TrajectoryObservables(rdf_r_max=3.5).begin([lat, tri], [z, z], [m, m], "cuda")
    with pytest.raises(ValueError, match="species"):
        TrajectoryObservables().begin([lat], [np.arange(1, 33)], [m], "cuda")


def test_md_run_refuses_a_foreign_observables_object():
    from torch_m3gnet.dynamics import MolecularDynamics
    from torch_m3gnet.model.build import build_model

    md = MolecularDynamics(build_model(5.0, 4.0, 3, 3, 95, 16, 1), ensemble="nve")
    pos, lat = _fcc(3.6, 2)
    with pytest.raises(TypeError, match="TrajectoryObservables"):
        md.run([lat], [pos], [np.full(32, 29)], 2, observables=object())
