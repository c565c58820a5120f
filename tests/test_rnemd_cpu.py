"""CPU checks of reverse non-equilibrium MD: the C ABI family m3g_rnemd_* is declared, bound and exported and refuses bad arguments
before touching a device, ReverseNEMD validates its arguments, the restatement (tests/rnemd_reference.py, the yardstick of the GPU
tests) conserves momentum and kinetic energy, and the host post-processing recovers a known conductivity and viscosity."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import rnemd_reference as rr

ROOT = Path(__file__).resolve().parent.parent
FAMILY = {"m3g_rnemd_state_bytes", "m3g_rnemd_init", "m3g_rnemd_exchange", "m3g_rnemd_read"}


def _lib():
    from torch_m3gnet import _lib

    return _lib, _lib.load_library()


def _params(_l, **kw):
    return _l.M3GRnemdParams(**dict(dict(kind=0, axis=2, flow_axis=0, n_slabs=8, n_swaps=1, reserved=0), **kw))


def test_header_prototypes_are_bound_and_exported_and_the_abi_version_stays():
    _l, lib = _lib()
    header = (ROOT / "include" / "m3gnet_hip.h").read_text()
    declared = set(re.findall(r"\b(m3g_rnemd_[a-z_]+)\s*\(", header))
    assert declared == FAMILY
    for name in declared:
        assert re.search(rf"\bint {name}\(", header) and hasattr(lib, name) and name in _l.SYMBOLS, name
    assert int(re.search(r"#define M3G_ABI_VERSION (\S+)", header).group(1)) == _l.ABI_VERSION == 11
    info = _l.M3GInfo()
    assert lib.m3g_get_info(C.byref(info)) == 0 and info.abi_version == 11
    value = lambda name: int(re.search(rf"#define {name} (\S+)", header).group(1))
    assert (value("M3G_RNEMD_HEAT"), value("M3G_RNEMD_MOMENTUM")) == (_l.RNEMD_HEAT, _l.RNEMD_MOMENTUM) == (rr.HEAT, rr.MOMENTUM)
    assert (value("M3G_RNEMD_MAX_SWAPS"), value("M3G_RNEMD_MAX_SLABS")) == (_l.RNEMD_MAX_SWAPS, _l.RNEMD_MAX_SLABS) == (8, 64)
    assert C.sizeof(_l.M3GRnemdParams) == 24
    assert [name for name, _ in _l.M3GRnemdParams._fields_] == ["kind", "axis", "flow_axis", "n_slabs", "n_swaps", "reserved"]
    assert re.search(r"typedef struct \{ int32_t kind, axis, flow_axis, n_slabs, n_swaps, reserved; \} m3g_rnemd_params;", header)
    assert (_l.DYN_STARTED, _l.DYN_ERROR) == (rr.STARTED, rr.ERROR)


def test_c_abi_state_bytes_grow_with_atoms_structures_and_slabs():
    _l, lib = _lib()
    sizes = {}
    for N, S, nb in [(2, 1, 2), (10000, 1, 2), (10000, 100, 2), (20000, 100, 2), (20000, 100, 64)]:
        n = C.c_size_t()
        assert lib.m3g_rnemd_state_bytes(N, S, nb, C.byref(n)) == _l.M3G_OK
        sizes[N, S, nb] = n.value
    assert sizes[2, 1, 2] < sizes[10000, 1, 2] < sizes[10000, 100, 2] < sizes[20000, 100, 2] < sizes[20000, 100, 64]
    n = C.c_size_t()
    for N, S, nb in [(0, 1, 8), (4, 0, 8), (3, 4, 8), (-1, 1, 8), (4, 1, 0), (4, 1, 1), (4, 1, 7), (4, 1, 66), (4, 1, -2)]:
        assert lib.m3g_rnemd_state_bytes(N, S, nb, C.byref(n)) == _l.M3G_ERR_VALUE, (N, S, nb)
    assert lib.m3g_rnemd_state_bytes(4, 1, 8, None) == _l.M3G_ERR_VALUE


def _init(lib, p, N=6, S=2, offsets=(0, 3, 6), lattices="default", active=None, state=C.c_void_p(256), nbytes=1 << 30):
    offs = None if offsets is None else np.array(offsets, dtype=np.int64)
    lat = np.stack([np.eye(3) * 5.0] * max(S, 1)) if isinstance(lattices, str) else lattices
    return lib.m3g_rnemd_init(None if p is None else C.byref(p), N, S, None if offs is None else offs.ctypes.data,
                              None if lat is None else lat.ctypes.data, None if active is None else active.ctypes.data, state, nbytes, None)


BAD_PARAMS = [dict(kind=2), dict(kind=-1), dict(axis=3), dict(axis=-1), dict(flow_axis=3), dict(flow_axis=-1),
              dict(kind=1, axis=1, flow_axis=1), dict(n_slabs=7), dict(n_slabs=0), dict(n_slabs=1), dict(n_slabs=66), dict(n_slabs=-2),
              dict(n_swaps=0), dict(n_swaps=9), dict(n_swaps=-1)]


@pytest.mark.parametrize("bad", BAD_PARAMS)
def test_c_abi_refuses_bad_parameters_in_every_call(bad):
    _l, lib = _lib()
    d, big = C.c_void_p(256), 1 << 30
    p = _params(_l, **bad)
    assert _init(lib, p) == _l.M3G_ERR_VALUE
    assert b"m3g_rnemd_init" in lib.m3g_last_error()
    assert lib.m3g_rnemd_exchange(C.byref(p), 6, 2, d, big, d, big, d, 1, 1, None) == _l.M3G_ERR_VALUE
    assert lib.m3g_rnemd_read(C.byref(p), 6, 2, d, big, *[None] * 7, None) == _l.M3G_ERR_VALUE


@pytest.mark.parametrize("offsets", [[0, 3, 2, 6], [0, 2, 2, 6], [1, 3, 5, 6], [0, 2, 4, 5], [0, 2, 4, 7]])
def test_c_abi_refuses_bad_offsets(offsets):
    _l, lib = _lib()
    assert _init(lib, _params(_l), N=6, S=3, offsets=offsets) == _l.M3G_ERR_VALUE
    assert b"m3g_rnemd_init: offsets" in lib.m3g_last_error()


def test_c_abi_refuses_bad_lattices():
    _l, lib = _lib()
    good = np.eye(3) * 5.0
    for bad in (np.zeros((3, 3)), np.array([[1.0, 0, 0], [2.0, 0, 0], [0, 0, 1.0]]), good * np.nan, good + np.diag([np.inf, 0, 0])):
        assert _init(lib, _params(_l), lattices=np.stack([good, bad])) == _l.M3G_ERR_VALUE
        assert b"structure 1" in lib.m3g_last_error()


def test_c_abi_refuses_null_pointers_and_short_buffers():
    _l, lib = _lib()
    d, big = C.c_void_p(256), 1 << 30
    p = _params(_l)
    assert _init(lib, None) == _l.M3G_ERR_VALUE
    assert _init(lib, p, offsets=None) == _l.M3G_ERR_VALUE
    assert _init(lib, p, lattices=None) == _l.M3G_ERR_VALUE
    assert _init(lib, p, state=None) == _l.M3G_ERR_VALUE
    assert _init(lib, p, N=1) == _l.M3G_ERR_VALUE   # fewer atoms than structures
    need, dyn = C.c_size_t(), C.c_size_t()
    assert lib.m3g_rnemd_state_bytes(6, 2, 8, C.byref(need)) == _l.M3G_OK and lib.m3g_dyn_state_bytes(6, 2, C.byref(dyn)) == _l.M3G_OK
    assert _init(lib, p, nbytes=need.value - 1) == _l.M3G_ERR_SIZE
    ex = lib.m3g_rnemd_exchange
    assert ex(None, 6, 2, d, big, d, big, d, 1, 1, None) == _l.M3G_ERR_VALUE
    assert ex(C.byref(p), 6, 2, None, big, d, big, d, 1, 1, None) == _l.M3G_ERR_VALUE
    assert ex(C.byref(p), 6, 2, d, big, None, big, d, 1, 1, None) == _l.M3G_ERR_VALUE
    assert ex(C.byref(p), 6, 2, d, big, d, big, None, 1, 1, None) == _l.M3G_ERR_VALUE
    assert ex(C.byref(p), 1, 2, d, big, d, big, d, 1, 1, None) == _l.M3G_ERR_VALUE
    assert ex(C.byref(p), 6, 2, d, need.value - 1, d, big, d, 1, 1, None) == _l.M3G_ERR_SIZE
    assert ex(C.byref(p), 6, 2, d, big, d, dyn.value - 1, d, 1, 1, None) == _l.M3G_ERR_SIZE
    assert b"dynamics state" in lib.m3g_last_error()
    none = [None] * 7
    assert lib.m3g_rnemd_read(None, 6, 2, d, big, *none, None) == _l.M3G_ERR_VALUE
    assert lib.m3g_rnemd_read(C.byref(p), 6, 2, None, big, *none, None) == _l.M3G_ERR_VALUE
    assert lib.m3g_rnemd_read(C.byref(p), 1, 2, d, big, *none, None) == _l.M3G_ERR_VALUE
    assert lib.m3g_rnemd_read(C.byref(p), 6, 2, d, need.value - 1, *none, None) == _l.M3G_ERR_SIZE


def test_reverse_nemd_argument_validation():
    from torch_m3gnet.model.build import build_model
    from torch_m3gnet.transport import ReverseNEMD, rnemd_params

    model = build_model(5.0, 4.0, 3, 3, 95, 16, 1)
    md = ReverseNEMD(model)
    assert (md.kind, md.params.axis, md.params.n_slabs, md.params.n_swaps, md.swap_interval, md.sample_interval) == ("heat", 2, 20, 1, 100, 10)
    assert ReverseNEMD(model, kind="momentum").params.flow_axis == 0 and ReverseNEMD(model, kind="momentum", axis=0).params.flow_axis == 1
    for kw in (dict(kind="mass"), dict(kind=0), dict(axis=3), dict(axis=-1), dict(axis=1.0), dict(n_slabs=4), dict(n_slabs=7), dict(n_slabs=66),
               dict(n_slabs=True), dict(n_swaps=0), dict(n_swaps=9), dict(n_swaps=1.5), dict(swap_interval=0), dict(sample_interval=0),
               dict(swap_interval=2.5), dict(flow_axis=3), dict(kind="momentum", flow_axis=2), dict(kind="momentum", axis=0, flow_axis=0),
               dict(temperature=0.0), dict(temperature=float("nan")), dict(timestep=0.0), dict(friction=-0.1), dict(skin=0.0)):
        with pytest.raises(ValueError):
            ReverseNEMD(model, **kw)
    with pytest.raises(TypeError):
        ReverseNEMD(model.model)
    assert rnemd_params("heat", 2, 2, 8).n_slabs == 2   # the kernels take two slabs; the driver needs six for a slope
    # counted in run() before anything touches the device
    lat, pos, z = np.eye(3) * 5.0, np.zeros((2, 3)) + [[0.0], [2.5]], np.array([29, 29])
    for kw in (dict(steps=-1), dict(steps=2.5), dict(steps=5, equilibration=-1), dict(steps=5, discard=6), dict(steps=5, discard=-1),
               dict(steps=5, loginterval=0), dict(steps=5, blocks=0)):
        with pytest.raises(ValueError):
            md.run([lat], [pos], [z], **kw)
    with pytest.raises(ValueError):
        md.run([lat], [pos], [z[:1]], 5)


@pytest.mark.parametrize("kind", [rr.HEAT, rr.MOMENTUM])
@pytest.mark.parametrize("mixed", [False, True])
def test_restatement_conserves_momentum_and_kinetic_energy(kind, mixed):
    """Equal masses: a permutation of rows (or of one component), so both sums change by the rounding of another summation order only;
    mixed masses: by the rounding of the reflection about the pair's centre of mass as well.  300 rows, 20 exchanges of 8 pairs."""
    rng = np.random.default_rng(5)
    n = 300
    lat = np.array([[7.0, 0.3, 0.1], [0.2, 8.0, -0.4], [0.5, 0.1, 30.0]])
    m = rng.choice([26.98, 63.546, 196.97], n) if mixed else np.full(n, 63.546)
    pos = rng.uniform(-2, 3, (n, 3)) @ lat
    v = rng.normal(0, 1e-2, (n, 3))
    ref = rr.RnemdReference(lat, m, kind, 2, 6, 8, flow_axis=0)
    bound = 4 * n * 2.0 ** -52   # relative to the sum of magnitudes: two summation orders of n terms, a few roundings per exchanged row
    for call in range(20):
        before = v.copy()
        moved = ref.transferred
        ref.exchange(pos, v)
        touched = [r for r in ref.last_pairs.reshape(-1) if r >= 0]
        assert len(touched) == len(set(touched)) == 16   # fresh velocities at every call: every pair finds slab 0 ahead
        untouched = np.setdiff1d(np.arange(n), touched)
        assert np.array_equal(v[untouched], before[untouched]) and not np.array_equal(v[touched], before[touched])
        assert np.abs((m[:, None] * (v - before)).sum(0)).max() <= bound * np.abs(m[:, None] * before).sum()
        assert abs((m * rr.speed2(v)).sum() - (m * rr.speed2(before)).sum()) <= bound * (m * rr.speed2(before)).sum()
        assert ref.transferred > moved
        if not mixed and kind == rr.HEAT:
            assert sorted(map(tuple, v)) == sorted(map(tuple, before))   # the multiset of velocity rows
        v[:] = rng.normal(0, 1e-2, (n, 3))
    assert ref.n_calls == ref.n_samples == 20 and ref.n_exchanged == 160
    assert ref.count.sum() == 20 * n and np.array_equal(ref.count, 20 * np.bincount(rr.slabs_of(pos, ref.g, 6), minlength=6))
    if mixed:
        return
    # equal masses, no fresh velocities: the exchange runs dry -- slab 0 ends no hotter (faster) than the middle slab, nothing more moves
    for _ in range(40):
        ref.exchange(pos, v, sample=False)
    slab, key = rr.slabs_of(pos, ref.g, 6), ref.keys(v)
    assert (ref.last_pairs == -1).all() and key[slab == 0].max() <= key[slab == 3].min()


def test_the_gpu_cases_hold_the_edges_they_are_built_for():
    """The inputs of tests/test_gpu_rnemd.py in the restatement: the one-row chunk's candidate leads, ties go to the lower row, a masked
    row is passed over, a short slab 0 and an empty middle slab, rows on slab planes, and a structure whose slab 0 is not ahead."""
    import rnemd_cases as rc

    for case in rc.CASES:
        parts = rc.parts_of(case)
        refs = rc.references(case, parts)
        vel = [p[3].copy() for p in parts]
        for call in range(3):
            for ref, p, v in zip(refs, parts, vel):
                ref.exchange(p[1], v)
            if call == 0:
                first = np.stack([ref.last_pairs.copy() for ref in refs])
        rc.check_construction(case, refs, first, 3)
        keys = refs[1].keys(parts[1][3])
        assert keys[10] == keys[20] == keys[30] and keys[40] == keys[50] and keys[256] > keys[10] > keys[40]
    for kind in ("heat", "momentum"):
        case = (kind, 2, 8, False, False)
        parts = rc.parts_of(case, cold_c=True)
        ref = rc.references(case, parts)[2]
        v = parts[2][3].copy()
        ref.exchange(parts[2][1], v)
        assert ref.n_exchanged == 0 and np.array_equal(v, parts[2][3]) and ref.count.tolist() == [32, 32]


def test_slab_assignment_wraps_and_clamps():
    g = rr.inverse_column(np.diag([4.0, 4.0, 16.0]), 2)
    assert g.tolist() == [0.0, 0.0, 0.0625]
    z = np.array([0.0, 2.0, 1.999999, 16.0, -1e-17 * 16.0, -2.0, 15.999, 34.0, -30.0])
    pos = np.stack([np.zeros_like(z), np.zeros_like(z), z], axis=1)
    assert rr.slabs_of(pos, g, 8).tolist() == [0, 1, 0, 0, 7, 7, 7, 1, 1]   # f = -1e-17 wraps to exactly 1.0: the last slab


@pytest.mark.parametrize("kind", ["heat", "momentum"])
def test_post_processing_recovers_a_known_coefficient(kind):
    """Synthetic accumulators with a profile linear between the exchange slabs (slope +G on one side, -G on the other) in a tilted
    cell, and the amount that a coefficient of 7.5 W/(m K) (2e-4 Pa s) transfers through both halves at that slope."""
    from torch_m3gnet import transport as tr

    n, axis, flow = 8, 2, 0
    lat = np.array([[6.0, 0.0, 0.0], [1.0, 5.0, 0.0], [1.5, -2.0, 40.0]])
    centres, area = tr.slab_geometry(lat, axis, n)
    assert area == pytest.approx(30.0) and np.allclose(centres, (np.arange(n) + 0.5) * 5.0)
    G = 0.8 if kind == "heat" else 3e-5       # K/A, or 1/fs
    base = 40.0 if kind == "heat" else -2e-4
    dist = np.minimum(np.arange(n), n - np.arange(n)) * 5.0   # distance to slab 0 through the nearer side
    prof = base + G * dist
    count = np.array([9, 10, 11, 10, 9, 12, 10, 8])
    mass = 63.546
    sums = np.zeros((n, 5))
    sums[:, 0] = mass * count
    if kind == "heat":
        sums[:, 4] = prof * 3.0 * tr.KB * tr.KAPPA * count
        want, unit, name = 7.5, tr.EV_PER_FS_A_K_IN_W_PER_M_K, "thermal_conductivity"
    else:
        sums[:, 1 + flow] = prof * sums[:, 0]
        sums[:, 4] = 1.0
        want, unit, name = 2e-4, tr.AMU_PER_A_FS_IN_PA_S, "viscosity"
    time = 5000.0
    moved = want / unit * G * 2.0 * area * time
    out = tr.transport_coefficients(kind, lat, axis, flow, count, sums, moved, time)
    assert out[name] == pytest.approx(want, rel=1e-10)
    assert out["gradient_sides"] == pytest.approx([G, -G], rel=1e-10) and out["gradient"] == pytest.approx(G, rel=1e-10)
    assert out["flux"] == pytest.approx(moved / (2 * area * time), rel=1e-14)
    got = out["temperature_profile"] if kind == "heat" else out["velocity_profile"][:, flow]
    assert np.allclose(got, prof, rtol=1e-12, atol=0) and np.array_equal(out["counts"], count)
    empty = count.copy()
    empty[2] = 0
    assert np.isnan(tr.transport_coefficients(kind, lat, axis, flow, empty, sums * (empty > 0)[:, None], moved, time)[name])
    assert tr.EV_PER_FS_A_K_IN_W_PER_M_K == 1.602176634e6 and tr.AMU_PER_A_FS_IN_PA_S == 1.66053906660e-2
