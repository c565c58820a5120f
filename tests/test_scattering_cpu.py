"""Scattering observables without a GPU: the restatement (tests/scattering_reference.py) on an exact lattice, under a change of the
frame called "now" and under a rigid translation; `q_vectors`; the host post-processing on synthetic sums; the export surface; every
refusal of the C ABI that precedes its first HIP call (status and message pinned, as tests/test_entry_refusals_cpu.py does); the
`observables` argument of MolecularDynamics.run; and the margin the GPU test allows the device, held to a second fp64 evaluation."""
import ctypes as C
import itertools
import re
from pathlib import Path

import numpy as np
import pytest

import scattering_cases as sc
import scattering_reference as ref

ROOT = Path(__file__).resolve().parent.parent
DUMMY, BIG = C.c_void_p(256), 1 << 30
M3G_OK, M3G_ERR_VALUE, M3G_ERR_SIZE = 0, 1, 3


def _lib():
    from torch_m3gnet import _lib as l

    return l, l.load_library()


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def _lattice_case(n=3, a=3.3, max_shift=40, seed=5):
    """n x n x n simple-cubic sites, every atom moved by a random integer number of (super)cell vectors."""
    rng = np.random.default_rng(seed)
    L = np.eye(3) * n * a
    sites = np.array(list(itertools.product(range(n), repeat=3)), dtype=np.float64) / n
    pos = (sites + rng.integers(-max_shift, max_shift + 1, sites.shape)) @ L
    hkl = np.array([h for h in itertools.product(range(-2 * n, 2 * n + 1), repeat=3) if any(h)], dtype=np.int32)
    return L, pos, hkl


def test_exact_lattice_gives_n_at_the_bragg_vectors_and_nothing_between():
    n = 3
    L, pos, hkl = _lattice_case(n)
    N = len(pos)
    rho, _, _ = ref.entries(pos, np.zeros_like(pos), L, np.zeros(N, int), np.ones(N), hkl, 1, False)
    bragg = (hkl % n == 0).all(axis=1)
    bound = ref.lattice_bound(N, hkl, 40)
    assert bragg.sum() == 5 ** 3 - 1 and bound.max() < 1e-9
    assert (np.abs(rho[bragg, 0] - N) <= bound[bragg]).all()
    assert (np.abs(rho[~bragg, 0]) <= bound[~bragg]).all()


def _walk(seed=2, n=12, frames=7):
    rng = np.random.default_rng(seed)
    L = np.array([[7.0, 0.2, 0.0], [0.5, 6.5, 0.1], [-0.3, 0.4, 7.5]])
    species, masses = np.arange(n) % 2, rng.uniform(1, 50, n)
    pos = [rng.uniform(0, 1, (n, 3)) @ L]
    for _ in range(frames - 1):
        pos.append(pos[-1] + rng.normal(0, 0.05, (n, 3)))
    vel = [rng.normal(0, 0.01, (n, 3)) for _ in range(frames)]
    hkl = np.array([[1, 0, 0], [0, -2, 1], [3, 1, -1], [1, 1, 1]])
    return L, species, masses, pos, vel, hkl


def test_lag_zero_does_not_depend_on_the_frame_called_now():
    """F(q, 0) over the frames k .. k + 2 of a ring of 3 is the same sum whether it is read when k + 2 is `now` (lags 0 of three
    samples) or rebuilt from the kept frames one at a time."""
    L, species, masses, pos, vel, hkl = _walk()
    for start in (0, 2, 4):
        acc = ref.Accumulator(species, masses, hkl, 2, 3, True)
        for k in range(start, start + 3):
            acc.sample(pos[k], vel[k], L)
        direct = np.zeros((len(hkl), 3))
        for rho, _, _ in acc.frames:
            for a in range(2):
                for b in range(a, 2):
                    direct[:, ref.pair_index(a, b, 2)] += (rho[:, a] * np.conj(rho[:, b])).real
        assert np.allclose(acc.f[:, :, 0], direct, rtol=1e-13, atol=1e-13)
        assert list(acc.lag_count) == [3, 2, 1]
    # and the ring forgets: five samples into a ring of three count each lag as often as three frames allow at every step
    acc = ref.Accumulator(species, masses, hkl, 2, 3, True)
    for k in range(5):
        acc.sample(pos[k], vel[k], L)
    assert list(acc.lag_count) == [5, 4, 3]


def test_rigid_translation_is_invisible_from_the_centre_of_mass_and_a_cosine_without():
    L, species, masses, pos, vel, hkl = _walk()
    step = np.array([0.31, -0.12, 0.07])
    frames = [pos[0] + k * step for k in range(5)]
    with_com = ref.Accumulator(species, masses, hkl, 2, 5, True)
    without = ref.Accumulator(species, masses, hkl, 2, 5, False)
    for p in frames:
        with_com.sample(p, vel[0], L)
        without.sample(p, vel[0], L)
    f = with_com.f / with_com.lag_count
    assert np.allclose(f, f[:, :, :1], rtol=1e-11, atol=1e-11)
    q = ref.cartesian_q(L, hkl)
    g = without.f / without.lag_count
    for lag in range(5):   # rho(t) = rho(0) exp(-i q . d t): Re[rho_a(t) rho_b*(t - l)] = Re[rho_a rho_b* exp(-i q . d l)], symmetrised: the cosine
        assert np.allclose(g[:, :, lag], g[:, :, 0] * np.cos(lag * q @ step)[:, None], rtol=1e-10, atol=1e-10)


def test_margin_covers_another_fp64_order():
    """The tolerance of tests/test_gpu_scattering.py, applied to a second fp64 evaluation of the reference (rows summed in the opposite
    order, fractional coordinates formed with the division last) in place of the device: it must pass with room to spare, and
    long double must be wider than fp64 or nothing here measures anything."""
    assert sc.long_double_is_wider(), "np.longdouble is no wider than fp64 on this host"
    for remove_com in (True, False):
        other = sc.reference(remove_com, "float64", True)
        for name in sc.QUANTITIES:
            unit, dev = sc.unit(remove_com, name), sc.deviation(other, name, remove_com)
            print(f"remove_com={remove_com} {name}: unit {unit:.3e}, other order / unit {dev / unit:.3f}")
            assert dev <= 0.25 * sc.MARGIN * unit


# ---- q_vectors -----------------------------------------------------------------------------------------------------------------------
def test_q_vectors_enumerates_half_the_sphere_once():
    from torch_m3gnet.scattering import cartesian_q, q_vectors

    a, q_max = 5.0, 4.1
    h = q_vectors(np.eye(3) * a, q_max)
    assert h.dtype == np.int32 and h.shape[1] == 3 and not (h == 0).all(axis=1).any()
    rows = {tuple(r) for r in h.tolist()}
    assert len(rows) == len(h) and not any((-x, -y, -z) in rows for x, y, z in rows)
    assert (np.linalg.norm(cartesian_q(np.eye(3) * a, h), axis=1) <= q_max).all()
    brute = sum(1 for t in itertools.product(range(-6, 7), repeat=3) if any(t) and 2 * np.pi / a * np.sqrt(sum(x * x for x in t)) <= q_max)
    assert brute % 2 == 0 and len(h) == brute // 2
    tri = np.array([[9.9, 0.0, 0.0], [2.0, 10.1, 0.0], [1.5, -1.2, 10.3]])
    thin = q_vectors(tri, 2.5, max_per_shell=4, seed=7)
    assert np.array_equal(thin, q_vectors(tri, 2.5, max_per_shell=4, seed=7))
    assert not np.array_equal(thin, q_vectors(tri, 2.5, max_per_shell=4, seed=8))
    full = q_vectors(tri, 2.5)
    assert len(thin) < len(full) and {tuple(r) for r in thin.tolist()} <= {tuple(r) for r in full.tolist()}
    from torch_m3gnet.scattering import default_shell_width, shell_index

    shells = shell_index(np.linalg.norm(cartesian_q(tri, thin), axis=1), default_shell_width(tri))
    assert np.bincount(shells).max() == 4
    assert (np.linalg.norm(cartesian_q(tri, full), axis=1) <= 2.5).all()


# ---- host post-processing ----------------------------------------------------------------------------------------------------------
def _synthetic(Q=6, G=16, n_sp=2, M=3, seed=3):
    rng = np.random.default_rng(seed)
    P = M * (M + 1) // 2
    sums = [rng.normal(0, 1, (Q, P, G)) for _ in range(3)]
    lag_count = np.arange(40, 40 - G, -1)
    counts = np.array([5, 3])[:n_sp]
    q_mod = np.array([1.0, 1.05, 1.9, 2.0, 2.1, 3.3])[:Q]
    return sums, lag_count, counts, q_mod


def test_post_processing_normalises_weights_and_averages_shells():
    from torch_m3gnet.scattering import scattering_from_sums
    from torch_m3gnet.trajectory import pair_index

    (f, cl, ct), lag_count, counts, q_mod = _synthetic()
    out = scattering_from_sums(f, cl, ct, lag_count, counts, q_mod, 2.0, 0.5, None, 3)
    N = counts.sum()
    for key, sums in (("f", f), ("c_l", cl), ("c_t", ct)):
        for a in range(2):
            for b in range(2):
                assert np.array_equal(out[key][a][b], sums[:, pair_index(a, b, 3)] / (lag_count * N))
        total = out[key][0][0] + out[key][1][1] + 2 * out[key][0][1]
        assert np.allclose(out[key + "_total"], total, rtol=1e-13, atol=1e-15)   # (four terms of ~1e-2 that may cancel)
    assert np.array_equal(out["s"], out["f_total"][:, 0]) and np.array_equal(out["time"], 2.0 * np.arange(16))
    # equal scattering lengths change nothing: sum_ab b^2 F_ab / (b^2 sum_a c_a)
    same = scattering_from_sums(f, cl, ct, lag_count, counts, q_mod, 2.0, 0.5, [2.5, 2.5], 3)
    assert np.allclose(same["f_total"], out["f_total"], rtol=1e-13, atol=1e-15)
    other = scattering_from_sums(f, cl, ct, lag_count, counts, q_mod, 2.0, 0.5, [1.0, -0.5], 3)
    want = (out["f"][0][0] - 0.5 * 2 * out["f"][0][1] + 0.25 * out["f"][1][1]) / (5 / 8 + 0.25 * 3 / 8)
    assert np.allclose(other["f_total"], want, rtol=1e-13, atol=1e-15)
    # shells against a loop: bins [1.0, 1.5) {0, 1}, [1.5, 2.0) {2}, [2.0, 2.5) {3, 4}, [3.0, 3.5) {5}
    members = [[0, 1], [2], [3, 4], [5]]
    assert list(out["shell_count"]) == [2, 1, 2, 1]
    for k, rows in enumerate(members):
        assert np.isclose(out["q_shell"][k], q_mod[rows].mean())
        for key in ("f", "c_l", "c_t"):
            loop = sum(out[key + "_total"][r] for r in rows) / len(rows)
            assert np.allclose(out[key + "_shell"][k], loop, rtol=1e-14, atol=1e-16)
    assert np.array_equal(out["s_shell"], out["f_shell"][:, 0])


def test_a_cosine_in_time_peaks_at_its_frequency_bin():
    """F(q,t) = cos(2 pi f_k t) with f_k on the grid of the transform: s_qw peaks in bin k, and a current correlation of the same
    shape puts `dispersion_l` there; the transform is the VDOS's own (trajectory.hann_cosine_transform)."""
    from torch_m3gnet.scattering import scattering_from_sums
    from torch_m3gnet.trajectory import correlations_from_sums, hann_cosine_transform

    G, dt, k = 64, 2.0, 9
    freq = np.arange(G) / (2.0 * G * dt)
    signal = np.cos(2 * np.pi * freq[k] * np.arange(G) * dt)
    lag_count = np.full(G, 10)
    sums = np.zeros((2, 1, G))
    sums[0, 0], sums[1, 0] = signal * 10 * 4, np.cos(2 * np.pi * freq[20] * np.arange(G) * dt) * 10 * 4
    out = scattering_from_sums(sums, sums, sums, lag_count, [4], [1.0, 2.0], dt, 0.5, None, 1)
    assert np.allclose(out["frequency"], freq * 1e3)
    assert list(np.argmax(out["s_qw"], axis=1)) == [k, 20] and list(np.argmax(out["c_t_qw"], axis=1)) == [k, 20]
    assert np.allclose(out["dispersion_l"], freq[[k, 20]] * 1e3)
    # the shared function is the one behind the VDOS, to the bit
    vacf = (signal * 10 * 4)[None, :] + 50.0
    vd = correlations_from_sums(np.zeros((1, G)), vacf, lag_count, [4], dt)
    c = vacf[0] / (4 * 10)
    assert np.array_equal(vd["vdos"][0], hann_cosine_transform(c / c[0], dt)[1])


# ---- the export surface ------------------------------------------------------------------------------------------------------------
def test_header_prototypes_are_bound_and_exported_and_the_abi_version_stays():
    _l, lib = _lib()
    header = (ROOT / "include" / "m3gnet_hip.h").read_text()
    declared = set(re.findall(r"\b(m3g_sq_[a-z_]+)\s*\(", header))
    assert declared == {"m3g_sq_state_bytes", "m3g_sq_init", "m3g_sq_sample", "m3g_sq_read", "m3g_sq_frame"}
    for name in declared:
        assert re.search(rf"\bint {name}\(", header) and hasattr(lib, name) and name in _l.SYMBOLS, name
    assert "#define M3G_ABI_VERSION 11" in header and _l.ABI_VERSION == 11
    assert C.sizeof(_l.M3GSqSizes) == 32 and C.sizeof(_l.M3GSqParams) == 8
    for name, value in (("M3G_SQ_MAX_INDEX", _l.SQ_MAX_INDEX), ("M3G_SQ_MAX_Q", _l.SQ_MAX_Q), ("M3G_SQ_MAX_SPECIES", _l.SQ_MAX_SPECIES),
                        ("M3G_SQ_MAX_LAGS", _l.SQ_MAX_LAGS), ("M3G_SQ_CELL", _l.SQ_CELL)):
        assert re.search(rf"#define {name} {value}\b", header), name


# ---- refusals: all of them answered on the host, before any HIP call -------------------------------------------------------------------
N, S, Q = 3, 1, 2


def _args(**over):
    """Valid host arrays of the smallest case (three atoms, one structure, two q-vectors); `over` replaces entries."""
    _l, lib = _lib()
    a = dict(sizes=_l.M3GSqSizes(N, S, Q, 2, 4), params=_l.M3GSqParams(1, 0), offsets=np.array([0, N], np.int64),
             species=np.array([0, 1, 0], np.int32), masses=np.array([63.5, 12.0, 63.5]), q_offsets=np.array([0, Q], np.int64),
             hkl=np.array([[1, 0, 0], [0, -2, 5]], np.int32), state=DUMMY, nbytes=BIG)
    a.update(over)
    return lib, a


def _init(**over):
    lib, a = _args(**over)
    ptr = lambda x: None if x is None else x.ctypes.data
    rc = lib.m3g_sq_init(C.byref(a["sizes"]), C.byref(a["params"]), ptr(a["offsets"]), ptr(a["species"]), ptr(a["masses"]), ptr(a["q_offsets"]),
                         ptr(a["hkl"]), a["state"], a["nbytes"], None)
    return rc, lib.m3g_last_error().decode()


def _state_bytes(sizes):
    _l, lib = _lib()
    n = C.c_size_t()
    assert lib.m3g_sq_state_bytes(C.byref(sizes), C.byref(n)) == M3G_OK
    return n.value


def test_init_refusals_are_pinned():
    _l, _ = _lib()
    sizes = lambda **kw: _l.M3GSqSizes(**{**dict(n_atoms=N, n_structs=S, n_q=Q, max_species=2, n_lags=4), **kw})
    need = _state_bytes(sizes())
    cases = [
        (dict(state=None), M3G_ERR_VALUE, "m3g_sq_init: null argument"),
        (dict(hkl=None), M3G_ERR_VALUE, "m3g_sq_init: null argument"),
        (dict(q_offsets=None), M3G_ERR_VALUE, "m3g_sq_init: null argument"),
        (dict(nbytes=need - 1), M3G_ERR_SIZE, f"m3g_sq_init: state buffer too small ({need - 1} < {need})"),
        (dict(hkl=np.array([[1, 0, 0], [0, 0, 0]], np.int32)), M3G_ERR_VALUE, "m3g_sq_init: q-vector 1 is h = 0"),
        (dict(hkl=np.array([[1, 0, 0], [0, -129, 0]], np.int32)), M3G_ERR_VALUE, "m3g_sq_init: q-vector 1 has an index beyond +-128"),
        (dict(sizes=sizes(max_species=5)), M3G_ERR_VALUE, "m3g_sq_init: max_species must be 1 .. 4"),
        (dict(sizes=sizes(n_lags=0)), M3G_ERR_VALUE, "m3g_sq_init: n_lags must be 1 .. 4096"),
        (dict(sizes=sizes(n_q=0)), M3G_ERR_VALUE, "m3g_sq_init: n_q must be 1 .. 4096 n_structs"),
        (dict(q_offsets=np.array([0, Q - 1], np.int64)), M3G_ERR_VALUE, "m3g_sq_init: q offsets must run from 0 to n_q"),
        (dict(q_offsets=np.array([1, Q], np.int64)), M3G_ERR_VALUE, "m3g_sq_init: q offsets must run from 0 to n_q"),
        (dict(species=np.array([0, 2, 0], np.int32)), M3G_ERR_VALUE, "m3g_sq_init: species index of atom 1 is outside 0 .. max_species - 1"),
        (dict(masses=np.array([63.5, 0.0, 63.5])), M3G_ERR_VALUE, "m3g_sq_init: mass of atom 1 is not finite and > 0"),
        (dict(offsets=np.array([0, N - 1], np.int64)), M3G_ERR_VALUE, "m3g_sq_init: offsets must run from 0 to n_atoms"),
        (dict(params=_l.M3GSqParams(2, 0)), M3G_ERR_VALUE, "m3g_sq_init: remove_com must be 0 or 1"),
    ]
    for over, status, message in cases:
        assert _init(**over) == (status, message), over
    assert _init(hkl=np.array([[128, 0, 0], [0, -128, 0]], np.int32), nbytes=need - 1)[0] == M3G_ERR_SIZE   # (the largest index passes)


def test_q_offsets_of_a_batch_are_checked_per_structure():
    _l, lib = _lib()
    over = dict(sizes=_l.M3GSqSizes(N, 2, 4097, 2, 4), offsets=np.array([0, 1, N], np.int64), hkl=np.ones((4097, 3), np.int32))
    assert _init(q_offsets=np.array([0, 4097, 4097], np.int64), **over) == (M3G_ERR_VALUE, "m3g_sq_init: structure 0 has more than 4096 q-vectors")
    assert _init(q_offsets=np.array([0, 4000, 3000, 4097], np.int64), offsets=np.array([0, 1, 2, N], np.int64), hkl=over["hkl"],
                 sizes=_l.M3GSqSizes(N, 3, 4097, 2, 4)) == (M3G_ERR_VALUE, "m3g_sq_init: q offsets must not decrease")
    need = _state_bytes(over["sizes"])
    assert _init(q_offsets=np.array([0, 0, 4097], np.int64), nbytes=need - 1, **over)[0] == M3G_ERR_VALUE   # (4097 in the second)
    assert _init(q_offsets=np.array([0, 1, 4097], np.int64), nbytes=need - 1, **over)[0] == M3G_ERR_SIZE    # an empty first one is legal


def test_sample_read_and_frame_refusals_are_pinned():
    _l, lib = _lib()
    sizes, params = _l.M3GSqSizes(N, S, Q, 2, 4), _l.M3GSqParams(1, 0)
    need = _state_bytes(sizes)
    z, p = C.byref(sizes), C.byref(params)
    err = lambda: lib.m3g_last_error().decode()
    assert lib.m3g_sq_state_bytes(z, None) == M3G_ERR_VALUE and err() == "m3g_sq_state_bytes: null argument"
    assert lib.m3g_sq_state_bytes(None, None) == M3G_ERR_VALUE and err() == "m3g_sq_state_bytes: null sizes or parameters"
    assert lib.m3g_sq_sample(z, p, None, BIG, DUMMY, DUMMY, DUMMY, None, 0.0, None) == M3G_ERR_VALUE and err() == "m3g_sq_sample: null argument"
    assert lib.m3g_sq_sample(z, p, DUMMY, BIG, DUMMY, None, DUMMY, None, 0.0, None) == M3G_ERR_VALUE and err() == "m3g_sq_sample: null argument"
    assert lib.m3g_sq_sample(z, p, DUMMY, need - 1, DUMMY, DUMMY, DUMMY, None, 0.0, None) == M3G_ERR_SIZE
    assert err() == "m3g_sq_sample: state buffer too small"
    assert lib.m3g_sq_sample(z, p, DUMMY, BIG, DUMMY, DUMMY, DUMMY, DUMMY, float("nan"), None) == M3G_ERR_VALUE
    assert err() == "m3g_sq_sample: kick must be finite"
    assert lib.m3g_sq_read(z, None, BIG, *[None] * 6, None) == M3G_ERR_VALUE and err() == "m3g_sq_read: null argument"
    assert lib.m3g_sq_read(z, DUMMY, need - 1, *[None] * 6, None) == M3G_ERR_SIZE and err() == "m3g_sq_read: state buffer too small"
    assert lib.m3g_sq_frame(z, None, BIG, 0, None, None, None, None) == M3G_ERR_VALUE and err() == "m3g_sq_frame: null argument"
    assert lib.m3g_sq_frame(z, DUMMY, need - 1, 0, None, None, None, None) == M3G_ERR_SIZE and err() == "m3g_sq_frame: state buffer too small"


def test_state_size_follows_from_the_sizes_alone():
    _l, _ = _lib()
    small, more_q, more_lags = (_state_bytes(_l.M3GSqSizes(863, 5, q, 3, g)) for q, g in ((326, 4), (327, 4), (326, 5)))
    assert small % 256 == 0 and more_q > small and more_lags - small >= 326 * 3 * 80


# ---- the driver's argument -----------------------------------------------------------------------------------------------------------
def test_observables_argument_of_run():
    from torch_m3gnet.dynamics import MolecularDynamics, _split_observables
    from torch_m3gnet.scattering import ScatteringObservables
    from torch_m3gnet.trajectory import TrajectoryObservables

    traj, sq = TrajectoryObservables(rdf_bins=10), ScatteringObservables(q_max=2.0)
    assert _split_observables(None) == (None, None) and _split_observables(traj) == (traj, None) and _split_observables(sq) == (None, sq)
    assert _split_observables([sq, traj]) == (traj, sq) and _split_observables((traj,)) == (traj, None) and _split_observables([]) == (None, None)

    lat, pos, z = np.eye(3) * 7.2, np.random.default_rng(0).uniform(0, 7.2, (32, 3)), np.full(32, 29)
    md = MolecularDynamics.__new__(MolecularDynamics)   # (run() looks at `observables` before it looks at anything else of the driver)
    md.ensemble = "nve"
    with pytest.raises(TypeError, match="TrajectoryObservables"):
        md.run([lat], [pos], [z], 2, observables=object())
    with pytest.raises(TypeError, match="a second ScatteringObservables"):
        md.run([lat], [pos], [z], 2, observables=[sq, ScatteringObservables(q_max=1.0)])
    with pytest.raises(TypeError, match="a second TrajectoryObservables"):
        md.run([lat], [pos], [z], 2, observables=[traj, sq, traj])
    with pytest.raises(TypeError, match="got int"):
        md.run([lat], [pos], [z], 2, observables=[traj, 3])
    for ensemble in ("npt_mtk", "npt_mtk_cell"):
        md.ensemble = ensemble
        for obs in (sq, [traj, sq], traj):
            with pytest.raises(ValueError, match=f"observables are not supported with {ensemble}"):
                md.run([lat], [pos], [z], 2, observables=obs)


def test_scattering_observables_checks_its_arguments():
    from torch_m3gnet.scattering import ScatteringObservables

    for bad in (dict(), dict(q_max=2.0, hkl=[[1, 0, 0]]), dict(q_max=-1.0), dict(q_max=2.0, n_lags=0), dict(q_max=2.0, n_lags=4097),
                dict(q_max=2.0, sample_interval=0), dict(q_max=2.0, remove_com=1), dict(q_max=2.0, max_per_shell=0)):
        with pytest.raises(ValueError):
            ScatteringObservables(**bad)
    for hkl in ([[1, 0, 0], [0, 129, 0]], [[1.5, 0, 0]], [1, 0, 0, 1]):   # refused on the host, before any device is touched
        with pytest.raises(ValueError):
            ScatteringObservables(hkl=hkl).begin([np.eye(3) * 5.0], [np.full(4, 29)], [np.full(4, 63.5)], "cuda")
    with pytest.raises(ValueError, match="at most 4"):
        ScatteringObservables(q_max=2.0).begin([np.eye(3) * 5.0], [np.arange(5) + 1], [np.ones(5)], "cuda")
    with pytest.raises(ValueError, match="no q-vector"):
        ScatteringObservables(q_max=0.1).begin([np.eye(3) * 5.0], [np.full(4, 29)], [np.full(4, 63.5)], "cuda")
