"""CPU checks of the batched finite-displacement phonons: the numpy restatement (tests/phonon_reference.py, the yardstick of the GPU
tests) under the truncated-LJ yardstick of tests/test_relax_cpu.py -- primitive fcc against the analytic lattice sum, the conventional
cell against the folded primitive bands, the force constants against the pair Hessian, the acoustic modes at Gamma -- the thermal
properties and DOS (restatement and torch_m3gnet.phonons) against closed forms, and the C ABI / Phonons refusing bad arguments before
touching a device."""
import ctypes as C

import numpy as np
import pytest
import torch

import phonon_reference as pr
from test_relax_cpu import EPS, RC, SIGMA, analytic_a0, lj

DELTA = 1e-3
MASS = 63.546
FCC_PRIM = 0.5 * np.array([[0.0, 1.0, 1.0], [1.0, 0.0, 1.0], [1.0, 1.0, 0.0]])
FCC_BASE = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])
# primitive fcc, fractional coordinates of the primitive reciprocal lattice
GAMMA, X, W, L, K = (0, 0, 0), (0, 0.5, 0.5), (0.25, 0.75, 0.5), (0.5, 0.5, 0.5), (0.375, 0.375, 0.75)


def lj_forces(lattice, rows, n_atoms):
    return np.concatenate([lj(rows[i:i + n_atoms], lattice)[1] for i in range(0, len(rows), n_atoms)])


def lj_phonons(lattice, pos, n, asr=True):
    """(Phi, sums, image table) of the truncated LJ crystal by central differences of fp64 forces."""
    ls, _ = pr.supercell(lattice, pos, n)
    rows = pr.displaced(lattice, pos, n, DELTA)
    ns = len(pos) * int(np.prod(n))
    phi, sums = pr.force_constants(lj_forces(ls, rows, ns), len(pos), DELTA, asr)
    return phi, sums, pr.image_table(lattice, pos, n)


def pair_hessian(R):
    r = np.linalg.norm(R)
    sr6 = (SIGMA / r) ** 6
    d1 = 4 * EPS * (-12 * sr6 * sr6 + 6 * sr6) / r
    d2 = 4 * EPS * (156 * sr6 * sr6 - 42 * sr6) / (r * r)
    e = R / r
    return d2 * np.outer(e, e) + (d1 / r) * (np.eye(3) - np.outer(e, e))


def analytic_frequencies(lattice, q):
    """Primitive fcc: D(q) = (1/m) sum_R K(R) (1 - cos 2 pi q.n_R) over the lattice points R = n_R L inside RC."""
    ns = np.stack(np.meshgrid(*[np.arange(-4, 5)] * 3, indexing="ij"), -1).reshape(-1, 3)
    d = np.zeros((3, 3))
    for nr in ns:
        R = nr @ lattice
        r = np.linalg.norm(R)
        if 1e-9 < r < RC:
            d += pair_hessian(R) * (1 - np.cos(2 * np.pi * np.dot(q, nr)))
    return pr.frequencies(d / MASS)


def path(points, npts=7):
    t = np.linspace(0, 1, npts)[:, None]
    return np.concatenate([np.asarray(a) + t * (np.asarray(b) - np.asarray(a)) for a, b in zip(points[:-1], points[1:])])


@pytest.fixture(scope="module")
def primitive():
    a0 = analytic_a0()
    lat = a0 * FCC_PRIM
    return a0, lat, lj_phonons(lat, np.zeros((1, 3)), (6, 6, 6))


def test_supercell_layout():
    lat = np.array([[3.0, 0.1, 0.0], [0.0, 4.0, 0.2], [0.3, 0.0, 5.0]])
    pos = np.array([[0.1, 0.2, 0.3], [1.0, 1.5, 2.0]])
    ls, sp = pr.supercell(lat, pos, (2, 3, 4))
    assert np.allclose(ls, np.diag([2.0, 3.0, 4.0]) @ lat) and sp.shape == (48, 3)
    l = (1 * 3 + 2) * 4 + 3
    assert np.allclose(sp[l * 2 + 1], pos[1] + np.array([1, 2, 3]) @ lat)
    assert np.array_equal(sp[:2], pos)
    rows = pr.displaced(lat, pos, (2, 3, 4), 0.01)
    assert rows.shape == ((1 + 12) * 48, 3)
    d = rows.reshape(13, 48, 3) - sp[None]
    assert np.abs(d[0]).max() == 0.0
    for u in range(2):
        for a in range(3):
            for k, sign in enumerate((1, -1)):
                c = d[1 + 6 * u + 2 * a + k]
                assert abs(c[u, a] - sign * 0.01) < 1e-12 and np.count_nonzero(c) == 1


def test_force_constants_equal_the_pair_hessian(primitive):
    a0, lat, (phi, sums, table) = primitive
    ls, sp = pr.supercell(lat, np.zeros((1, 3)), (6, 6, 6))
    expect = np.zeros_like(phi)
    for j in range(1, len(sp)):
        img = table[0, j]
        R = img[0] @ lat
        if np.linalg.norm(R) < RC:
            assert len(img) == 1   # width > 2 RC: one shortest image per pair inside RC
            expect[0, j] = -pair_hessian(R)
    expect[0, 0] = -expect[0, 1:].sum(axis=0)
    scale = np.abs(expect).max()
    # every pair entry to 1e-6; the self term (minus the sum of the twelve nearest-neighbour blocks, whose O(delta^2) errors add up
    # coherently) to 1e-5
    assert np.abs(phi[0, 1:] - expect[0, 1:]).max() < 1e-6 * scale
    assert np.abs(phi[0, 0] - expect[0, 0]).max() < 1e-5 * scale
    assert np.abs(sums).max() < 1e-6 * np.abs(expect).max()   # fp64 forces: the rule holds already


def test_primitive_fcc_matches_the_analytic_lattice_sum(primitive):
    a0, lat, (phi, _, table) = primitive
    qs = path([GAMMA, X, W, L, GAMMA, K])
    for q in qs:
        f = pr.frequencies(pr.dynamical_matrix(phi, table, [MASS], q))
        ref = analytic_frequencies(lat, q)
        assert np.abs(f - ref).max() <= 1e-5 * max(np.abs(ref).max(), 0.1), (q, f, ref)   # (Gamma: both ~1e-7 THz)


def test_gamma_has_three_zero_acoustic_modes_with_asr(primitive):
    _, lat, (phi, _, table) = primitive
    f = pr.frequencies(pr.dynamical_matrix(phi, table, [MASS], GAMMA))
    assert np.abs(f).max() < 1e-6
    x = pr.frequencies(pr.dynamical_matrix(phi, table, [MASS], X))
    assert x.min() > 1.0 and abs(x[0] - x[1]) < 1e-6 * x[2]   # TA doubly degenerate at X


def test_conventional_cell_gives_the_folded_primitive_bands(primitive):
    a0, lat_p, (phi_p, _, table_p) = primitive
    conv = np.eye(3) * a0
    phi, sums, table = lj_phonons(conv, FCC_BASE * a0, (3, 3, 3))
    rng = np.random.default_rng(0)
    for qc in [np.zeros(3), np.array([0.5, 0, 0]), np.array([0.5, 0.5, 0.5]), np.array([0.25, 0.5, 0])] + list(rng.uniform(-0.5, 0.5, (4, 3))):
        f = pr.frequencies(pr.dynamical_matrix(phi, table, [MASS] * 4, qc))
        union = []
        for g in np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]):
            q_cart = (qc + g) @ np.linalg.inv(conv).T   # no 2 pi
            union.extend(pr.frequencies(pr.dynamical_matrix(phi_p, table_p, [MASS], lat_p @ q_cart)))
        union = np.sort(union)
        assert np.abs(f - union).max() <= 1e-5 * np.abs(union).max(), (qc, f, union)


# ---- thermal properties and DOS ---------------------------------------------------------------------------------------------------
FREQS = np.array([[0.0, 0.5, 2.0, 3.5, 7.0, 11.0], [-0.3, 1.0, 1.0, 4.0, 6.5, 9.0]])   # THz, two q-points of a 2-atom cell
WEIGHTS = np.array([0.25, 0.75])


def closed_forms(T):
    """Per mode: F = kT ln(2 sinh(x/2)), E = (h nu / 2) coth(x/2), Cv = k (x/2)^2 / sinh^2(x/2), S = (E - F) / T."""
    out = {k: 0.0 for k in ("free_energy", "entropy", "heat_capacity", "energy")}
    for w, row in zip(WEIGHTS, FREQS):
        for f in row[row >= 1e-3]:
            e = f * pr.H_EV_THZ
            x = e / (pr.KB * T)
            F = pr.KB * T * np.log(2 * np.sinh(x / 2))
            E = 0.5 * e / np.tanh(x / 2)
            out["free_energy"] += w * F
            out["energy"] += w * E
            out["heat_capacity"] += w * pr.KB * (x / 2) ** 2 / np.sinh(x / 2) ** 2
            out["entropy"] += w * (E - F) / T
    return out


def test_thermal_properties_match_closed_forms():
    from torch_m3gnet.phonons import KB_EV, harmonic_thermal

    T = np.array([10.0, 77.0, 300.0, 1000.0])
    ref = pr.thermal(FREQS, WEIGHTS, T)
    got = harmonic_thermal(torch.tensor(FREQS), torch.tensor(WEIGHTS), torch.tensor(T))
    assert got["n_excluded"] == 2   # the zero and the imaginary mode
    for i, t in enumerate(T):
        c = closed_forms(t)
        for k in c:
            assert abs(ref[k][i] - c[k]) <= 1e-10 * max(abs(c[k]), 1e-8), (k, t)
            assert abs(float(got[k][i]) - c[k]) <= 1e-10 * max(abs(c[k]), 1e-8), (k, t)
    # high T: each included mode contributes k_B (3 n k_B per cell when every mode is included)
    hot = harmonic_thermal(torch.tensor(FREQS[:, 2:]), torch.tensor(WEIGHTS), torch.tensor([1e5]))
    assert abs(float(hot["heat_capacity"][0]) / (4 * KB_EV) - 1) < 1e-6
    # T = 0: zero-point energy, no entropy or heat capacity
    zero = harmonic_thermal(torch.tensor(FREQS), torch.tensor(WEIGHTS), torch.tensor([0.0]))
    zpe = sum(w * 0.5 * pr.H_EV_THZ * row[row >= 1e-3].sum() for w, row in zip(WEIGHTS, FREQS))
    assert abs(float(zero["free_energy"][0]) - zpe) < 1e-15 and abs(float(zero["energy"][0]) - zpe) < 1e-15
    assert float(zero["entropy"][0]) == 0.0 and float(zero["heat_capacity"][0]) == 0.0


def test_dos_integrates_to_the_mode_count():
    from torch_m3gnet.phonons import gaussian_dos

    grid = np.linspace(-2, 14, 4001)
    ref = pr.dos(FREQS, WEIGHTS, grid, 0.2)
    got = gaussian_dos(torch.tensor(FREQS), torch.tensor(WEIGHTS), torch.tensor(grid), 0.2).numpy()
    assert np.abs(got - ref).max() < 1e-12 * ref.max()
    assert abs(np.trapezoid(ref, grid) - 6.0) < 1e-6


def test_constants_and_mesh():
    from torch_m3gnet.phonons import THZ_PER_SQRT_EV_A2_AMU, monkhorst_pack

    assert abs(THZ_PER_SQRT_EV_A2_AMU - 15.633304) < 1e-6
    g = monkhorst_pack(4)
    assert g.shape == (64, 3) and (g >= -0.5).all() and (g < 0.5).all() and (np.abs(g).sum(1) == 0).sum() == 1
    mp = monkhorst_pack((2, 2, 2), gamma_centered=False)
    assert np.allclose(np.sort(np.unique(mp)), [-0.25, 0.25])


# ---- argument checks (no device needed: refused before any HIP call) ----------------------------------------------------------------
def _init(offsets=(0, 1, 3), supercells=((2, 2, 2), (1, 1, 2)), lattices=None, positions=None, masses=(1.0, 2.0, 3.0), delta=0.01,
          sizes=None, state_bytes=1 << 30):
    from torch_m3gnet import _lib

    lib = _lib.load_library()
    off = np.array(offsets, dtype=np.int64)
    sc = np.array(supercells, dtype=np.int32).reshape(-1, 3)
    lat = np.ascontiguousarray(np.array(lattices, dtype=np.float64) if lattices is not None else np.stack([np.eye(3) * 4.0] * len(sc)))
    pos = np.ascontiguousarray(np.array(positions, dtype=np.float64) if positions is not None else np.arange(3 * off[-1], dtype=np.float64).reshape(-1, 3) * 0.1)
    m = np.array(masses, dtype=np.float64)
    if sizes is None:
        nu = np.diff(off)
        cells = np.clip(sc, 1, None).prod(1)
        sizes = (len(nu), int(off[-1]), int((nu * cells).sum()), int((nu * nu * cells).sum()))
    sz = _lib.M3GPhSizes(*sizes)
    dummy = C.c_void_p(256)   # never dereferenced: the call returns at the checks
    return lib.m3g_ph_init(C.byref(sz), off.ctypes.data, sc.ctypes.data, lat.ctypes.data, pos.ctypes.data, m.ctypes.data, delta, dummy,
                           state_bytes, None)


TIE = dict(offsets=(0, 2), supercells=((1, 1, 1),), lattices=[np.diag([1e-7, 1e-7, 2e3])], positions=[[0, 0, 0], [0, 0, 1e3]],
           masses=(1.0, 1.0))   # 50 images of the pair (0, 1) tie: twice a 5 x 5 grid of 1e-7 A


@pytest.mark.parametrize("case,word", [(dict(offsets=(0, 2, 1, 3), supercells=((1, 1, 1),) * 3, sizes=(3, 3, 3, 3)), b"offsets"), (dict(offsets=(1, 2, 3)), b"offsets"),
                                       (dict(supercells=((0, 2, 2), (1, 1, 2))), b"supercell"),
                                       (dict(supercells=((2, 2, 2), (1, -1, 2))), b"supercell"),
                                       (dict(delta=0.0), b"delta"), (dict(delta=-0.01), b"delta"), (dict(delta=float("nan")), b"delta"),
                                       (dict(delta=float("inf")), b"delta"),
                                       (dict(masses=(1.0, 0.0, 3.0)), b"mass"), (dict(masses=(1.0, 2.0, float("nan"))), b"mass"),
                                       (dict(masses=(-1.0, 2.0, 3.0)), b"mass"),
                                       (dict(lattices=[np.eye(3) * 4, np.zeros((3, 3))]), b"singular"),
                                       (dict(lattices=[np.eye(3) * 4, [[1, 0, 0], [2, 0, 0], [0, 0, 1]]]), b"singular"),
                                       (dict(lattices=[np.eye(3) * 4, np.eye(3) * np.nan]), b"not finite"),
                                       (dict(positions=np.full((3, 3), np.inf)), b"not finite"),
                                       (dict(sizes=(2, 3, 20, 40)), b"sizes do not match"),
                                       (TIE, b"image table capacity")])
def test_c_abi_refuses_bad_phonon_arguments(case, word):
    from torch_m3gnet import _lib

    assert _init(**case) == _lib.M3G_ERR_VALUE
    assert word in _lib.load_library().m3g_last_error()


def test_c_abi_phonon_sizes():
    from torch_m3gnet import _lib

    lib = _lib.load_library()
    # valid arguments: the call gets past the checks (the image table included) and fails only on the too small state buffer
    assert _init(state_bytes=1) == _lib.M3G_ERR_SIZE
    assert _init(**dict(TIE, lattices=[np.diag([3.0, 3.0, 2e3])]), state_bytes=1) == _lib.M3G_ERR_SIZE
    size = C.c_size_t()
    assert lib.m3g_ph_state_bytes(C.byref(_lib.M3GPhSizes(1, 4, 108, 432)), C.byref(size)) == _lib.M3G_OK and size.value > 432 * 27 * 24
    for bad in ((0, 1, 1, 1), (2, 1, 1, 1), (1, 4, 3, 8), (1, 4, 8, 7)):
        assert lib.m3g_ph_state_bytes(C.byref(_lib.M3GPhSizes(*bad)), C.byref(size)) == _lib.M3G_ERR_VALUE
    dummy = C.c_void_p(256)
    sz = _lib.M3GPhSizes(1, 4, 108, 432)
    assert lib.m3g_ph_displace(C.byref(sz), dummy, 1 << 30, None, None) == _lib.M3G_ERR_VALUE
    assert lib.m3g_ph_displace(C.byref(sz), dummy, 1, dummy, None) == _lib.M3G_ERR_SIZE
    assert lib.m3g_ph_force_constants(C.byref(sz), dummy, 1 << 30, dummy, 2, dummy, dummy, dummy, None) == _lib.M3G_ERR_VALUE
    assert lib.m3g_ph_force_constants(C.byref(sz), dummy, 1 << 30, dummy, 1, dummy, None, dummy, None) == _lib.M3G_ERR_VALUE
    for n_q, max_nu in ((-1, 4), (3, 0), (3, 5)):
        assert lib.m3g_ph_dynmat(C.byref(sz), dummy, 1 << 30, dummy, n_q, dummy, dummy, max_nu, dummy, None) == _lib.M3G_ERR_VALUE
    assert lib.m3g_ph_dynmat(C.byref(sz), dummy, 1 << 30, dummy, 0, None, None, 4, None, None) == _lib.M3G_OK   # nothing to do


def test_sub_batches_against_a_brute_force_restatement():
    """The engine sub-batches of one structure's copies (Phonons.run, the strain drivers): in order, no overlap, at most max_atoms
    atoms each but never less than one copy -- the split decides the engine's batch composition, so it is pinned."""
    from torch_m3gnet._driver import sub_batches

    cases = ((25, 32, 200), (25, 32, 31), (25, 32, 32), (25, 32, 800), (25, 32, 10**6), (1, 4, 3), (13, 8, 24), (7, 5, 11))
    for n_copies, n, max_atoms in cases:
        want, first = [], 0
        while first < n_copies:
            count = 1
            while (count + 1) * n <= max_atoms and first + count < n_copies:
                count += 1
            want.append((first, count))
            first += count
        got = list(sub_batches(n_copies, n, max_atoms))
        assert got == want, (n_copies, n, max_atoms)
        assert [f for f, _ in got] == np.cumsum([0] + [c for _, c in got])[:-1].tolist() and sum(c for _, c in got) == n_copies
    assert [c for _, c in sub_batches(25, 32, 200)] == [6, 6, 6, 6, 1]
    assert [c for _, c in sub_batches(25, 32, 31)] == [1] * 25


def test_phonons_argument_validation():
    from torch_m3gnet.model.build import build_model
    from torch_m3gnet.phonons import Phonons

    model = build_model(5.0, 4.0, 3, 3, 95, 16, 1)
    with pytest.raises(TypeError):
        Phonons(model.model)
    with pytest.raises(TypeError, match="Phonons"):   # names the driver that was constructed
        Phonons(model.model)
    for kw in (dict(delta=0.0), dict(delta=-0.01), dict(delta=float("nan")), dict(asr=2), dict(max_atoms=0), dict(max_atoms=1.5),
               dict(max_qpoints=0), dict(cutoff_frequency=-1.0), dict(skin=0.0)):
        with pytest.raises(ValueError):
            Phonons(model, **kw)
    ph = Phonons(model)
    lat = np.eye(3) * 3.6
    pos = FCC_BASE * 3.6
    z = np.full(4, 29)
    ph._check([lat], [pos], [z], (2, 2, 2), None)   # valid
    for args in (([lat], [pos], [z], (0, 2, 2), None),              # supercell dim < 1
                 ([lat], [pos], [z], (2, 2), None),                 # bad supercell shape
                 ([lat], [pos], [z], (2.0, 2.0, 2.0), None),        # not integers
                 ([lat], [pos], [z], [(2, 2, 2), (2, 2, 2)], None),  # one supercell too many
                 ([lat], [pos], [z], (2, 2, 2), [np.ones(3)]),      # masses of the wrong length
                 ([lat], [pos], [z], (2, 2, 2), [np.array([1.0, 1.0, 0.0, 1.0])]),
                 ([lat], [pos], [z], (2, 2, 2), [np.array([1.0, 1.0, np.nan, 1.0])]),
                 ([lat], [pos], [np.full(4, 0)], (2, 2, 2), None),  # no default mass for Z = 0
                 ([np.zeros((3, 3))], [pos], [z], (2, 2, 2), None),  # singular cell
                 ([lat], [pos * np.nan], [z], (2, 2, 2), None),
                 ([lat], [pos[:3]], [z], (2, 2, 2), None),
                 ([], [], [], (2, 2, 2), None)):
        with pytest.raises(ValueError):
            ph.run(*args)
