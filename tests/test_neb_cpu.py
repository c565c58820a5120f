"""CPU checks of the batched climbing-image NEB: the numpy restatement (tests/neb_reference.py, the yardstick of the GPU tests) -- the
four tangent branches and the climbing choice by hand, a CI-NEB on the Mueller-Brown surface that lands on the saddle scipy finds, a
vacancy hop under the truncated-LJ yardstick of tests/test_relax_cpu.py that comes out mirror-symmetric -- `interpolate`, and the C
ABI / NEB refusing bad arguments before touching a device."""
import ctypes as C

import numpy as np
import pytest
from scipy.optimize import minimize, root

import fire_reference as fr
import neb_reference as nr
from test_relax_cpu import analytic_a0, fcc, lj
from torch_m3gnet.neb import interpolate

# ---- Mueller-Brown surface in x, y (energy x 0.01 eV, length x 2 A) with a harmonic z term -------------------------------------
MB_A = np.array([-200.0, -100.0, -170.0, 15.0])
MB_a = np.array([-1.0, -1.0, -6.5, 0.7])
MB_b = np.array([0.0, 0.0, 11.0, 0.6])
MB_c = np.array([-10.0, -10.0, -6.5, 0.7])
MB_X0 = np.array([1.0, 0.0, -0.5, -1.0])
MB_Y0 = np.array([0.0, 0.5, 1.5, 1.0])
MB_E, MB_L, MB_KZ = 0.01, 2.0, 1.0


def mueller_brown(p):
    """Energy (eV) and force [3] of one atom at p (A)."""
    x, y, z = p[0] / MB_L, p[1] / MB_L, p[2]
    dx, dy = x - MB_X0, y - MB_Y0
    t = MB_A * np.exp(MB_a * dx * dx + MB_b * dx * dy + MB_c * dy * dy)
    gx = MB_E * (t * (2 * MB_a * dx + MB_b * dy)).sum() / MB_L
    gy = MB_E * (t * (MB_b * dx + 2 * MB_c * dy)).sum() / MB_L
    return MB_E * t.sum() + 0.5 * MB_KZ * z * z, np.array([-gx, -gy, -MB_KZ * z])


def mb_image(pos):
    e, f = mueller_brown(np.asarray(pos).reshape(3))
    return e, f[None]


def _mb_grad(p):
    return -mueller_brown(p)[1]


def _mb_hess(p, h=1e-6):
    return np.array([(_mb_grad(p + d) - _mb_grad(p - d)) / (2 * h) for d in np.eye(3) * h])


def mb_minima():
    """The minima near (0.62, 0.03) and (-0.05, 0.47) (Mueller-Brown units), refined."""
    return [minimize(lambda p: mueller_brown(p)[0], np.array([x * MB_L, y * MB_L, 0.0]), jac=_mb_grad, method="BFGS",
                     options=dict(gtol=1e-12)).x for x, y in ((0.62, 0.03), (-0.05, 0.47))]


def mb_band(n_images=9):
    """A straight band between the two minima, the interior images pushed off the plane z = 0 (the z force is exercised)."""
    a, b = mb_minima()
    imgs = interpolate(np.eye(3) * 100.0, a[None], b[None], n_images, mic=False)
    return [p + np.array([[0.0, 0.0, 0.01 * np.sin(j)]]) if 0 < j < n_images - 1 else p for j, p in enumerate(imgs)]


def mb_saddle(start):
    s = root(_mb_grad, np.asarray(start).reshape(3), jac=_mb_hess, tol=1e-12).x
    assert np.linalg.norm(_mb_grad(s)) < 1e-10
    return s


# ---- tangent, projection, climbing choice ------------------------------------------------------------------------------------
TP = np.array([[1.0, 0.0, 0.0], [0.0, 2.0, 0.0]])
TM = np.array([[0.0, 0.5, 0.0], [0.0, 0.0, 3.0]])


@pytest.mark.parametrize("v,expect", [((0.0, 1.0, 2.0), (1, 0)),       # rising: tau+
                                      ((2.0, 1.0, 0.0), (0, 1)),       # falling: tau-
                                      ((0.0, 2.0, 1.0), (2, 1)),       # maximum, V_i+1 > V_i-1: dVmax tau+ + dVmin tau-
                                      ((1.0, 2.0, 0.0), (1, 2)),       # maximum, V_i+1 < V_i-1: dVmin tau+ + dVmax tau-
                                      ((1.0, 0.0, 2.0), (2, 1)),       # minimum, V_i+1 > V_i-1
                                      ((2.0, 0.0, 1.0), (1, 2)),       # minimum, V_i+1 < V_i-1
                                      ((0.0, 1.0, 1.0), (1, 0)),       # tie with the next image (not strictly rising)
                                      ((1.0, 1.0, 0.0), (0, 1)),       # tie with the previous image
                                      ((1.0, 1.0, 1.0), (0, 0))])      # all equal: tau = 0
def test_tangent_branches(v, expect):
    t = nr.tangent(v[0], v[1], v[2], TP, TM)
    assert np.array_equal(t, expect[0] * TP + expect[1] * TM)


def test_climbing_choice_takes_the_lowest_index_on_ties():
    assert nr.climbing_index([1.0, 3.0, 3.0, 2.0]) == 1
    assert nr.climbing_index([np.nan, 1.0, 1.0]) == 1
    assert nr.climbing_index([-5.0]) == 0
    assert nr.climbing_index([np.nan, np.nan]) == -1


def test_projection_ordinary_climbing_and_degenerate_images():
    rng = np.random.default_rng(0)
    imgs = [rng.normal(0, 1, (4, 3)) for _ in range(5)]
    forces = [rng.normal(0, 1, (4, 3)) for _ in range(3)]
    e = [0.0, 0.5, 2.0, 1.0, 0.2]
    k = 0.3
    nf, rows = nr.neb_forces(imgs, e, forces, k, climb=True)
    assert list(rows[:, 4]) == [0.0, 1.0, 0.0]
    for i in (1, 2, 3):
        t = nr.tangent(e[i - 1], e[i], e[i + 1], imgs[i + 1] - imgs[i], imgs[i] - imgs[i - 1])
        t /= np.linalg.norm(t)
        f = forces[i - 1]
        perp = f - np.vdot(f, t) * t
        assert np.allclose(nf[i - 1] - np.vdot(nf[i - 1], t) * t, perp, atol=1e-13)   # the perpendicular force is kept
        par = np.vdot(nf[i - 1], t)
        if i == 2:   # climbing: the parallel component is inverted, no spring
            assert abs(par + np.vdot(f, t)) < 1e-13 and rows[1, 3] == 0.0
        else:        # ordinary: the parallel component is the spring
            spring = k * (np.linalg.norm(imgs[i + 1] - imgs[i]) - np.linalg.norm(imgs[i] - imgs[i - 1]))
            assert abs(par - spring) < 1e-13 and rows[i - 1, 3] == spring
    # without climb the highest image is an ordinary one
    _, rows = nr.neb_forces(imgs, e, forces, k, climb=False)
    assert not rows[:, 4].any()
    # all three energies equal -> |tau| = 0 -> NaN rows; a non-finite force -> NaN rows of that image only
    nf, _ = nr.neb_forces(imgs, [0.0, 1.0, 1.0, 1.0, 0.0], forces, k, climb=False)
    assert np.isnan(nf[1]).all() and np.isfinite(nf[[0, 2]]).all()
    bad = [f.copy() for f in forces]
    bad[2][1, 0] = np.inf
    nf, _ = nr.neb_forces(imgs, e, bad, k, climb=True)
    assert np.isnan(nf[2]).all() and np.isfinite(nf[:2]).all()


def test_interpolate_takes_the_minimum_image():
    lat = np.array([[4.0, 0.0, 0.0], [1.0, 5.0, 0.0], [0.0, 0.5, 6.0]])
    p0 = np.array([[0.2, 0.3, 0.1], [1.0, 1.0, 1.0]])
    p1 = p0 + np.array([[0.3, -0.2, 0.1], [-0.1, 0.2, 0.4]]) + np.array([[1, 0, 0], [0, -1, 2]]) @ lat
    imgs = interpolate(lat, p0, p1, 5)
    assert len(imgs) == 5 and np.array_equal(imgs[0], p0)
    assert np.allclose(imgs[-1] - p0, [[0.3, -0.2, 0.1], [-0.1, 0.2, 0.4]], atol=1e-12)
    assert np.allclose(imgs[2], 0.5 * (imgs[0] + imgs[-1]), atol=1e-12)
    assert np.allclose(interpolate(lat, p0, p1, 3, mic=False)[-1], p1)
    with pytest.raises(ValueError):
        interpolate(lat, p0, p1, 2)


# ---- the band loop ----------------------------------------------------------------------------------------------------------
def test_restatement_ci_neb_finds_the_mueller_brown_saddle():
    band = nr.run_band(mb_band(), mb_image, k=0.1, climb=True, fmax=1e-4, steps=2000)
    assert band.fire.converged and 0 < band.fire.n_steps < 2000
    ci = band.climbing_image
    assert 0 < ci < 8 and ci == 1 + int(np.argmax(band.energies[1:-1]))
    s = mb_saddle(band.images[ci])
    assert np.sort(np.linalg.eigvalsh(_mb_hess(s)))[0] < 0 < np.sort(np.linalg.eigvalsh(_mb_hess(s)))[1]   # a first-order saddle
    assert np.linalg.norm(band.images[ci][0] - s) < 1e-3, (band.images[ci], s)
    assert abs(band.energies[ci] - mueller_brown(s)[0]) < 1e-5
    assert abs(s[0] / MB_L - 0.212) < 2e-3 and abs(s[1] / MB_L - 0.293) < 2e-3   # the saddle between these two minima
    # without climbing the highest image lies below the saddle
    plain = nr.run_band(mb_band(), mb_image, k=0.1, climb=False, fmax=1e-3, steps=2000)
    assert plain.fire.converged and plain.energies.max() < mueller_brown(s)[0]


def _vacancy_hop():
    """2x2x2 fcc at the LJ lattice constant without site 0; atom 0 (on site 1) hops into the vacancy.  Returns the lattice, the
    relaxed endpoints and the mirror through the hop's midplane."""
    a0 = analytic_a0()
    sites, lat = fcc(a0)
    init = sites[1:].copy()
    final = init.copy()
    final[0] = sites[0]
    ends = [fr.relax(p, lat, lj, relax_cell=False, fmax=1e-5, steps=3000)[0] for p in (init, final)]
    assert all(e.converged for e in ends)
    n = (sites[1] - sites[0]) / np.linalg.norm(sites[1] - sites[0])
    mid = 0.5 * (sites[0] + sites[1])

    def mirror(p):
        return p - 2.0 * ((p - mid) @ n)[:, None] * n[None]

    return lat, ends[0].pos, ends[1].pos, mirror


def _same_up_to_permutation(p, q, lat):
    d = p[:, None, :] - q[None, :, :]
    frac = np.linalg.solve(lat.T, d.reshape(-1, 3).T).T
    d = ((frac - np.round(frac)) @ lat).reshape(d.shape)
    return np.linalg.norm(d, axis=-1).min(axis=1).max()


def test_restatement_vacancy_hop_is_symmetric_with_the_saddle_in_the_middle():
    lat, p0, p1, mirror = _vacancy_hop()
    assert _same_up_to_permutation(mirror(p0), p1, lat) < 1e-6   # the relaxed endpoints are mirror images

    def ef(pos):
        e, f, _ = lj(pos, lat)
        return e, f

    band = nr.run_band(interpolate(lat, p0, p1, 7), ef, k=0.1, climb=True, fmax=0.01, steps=1000)
    assert band.fire.converged and band.fire.n_steps < 1000
    assert band.climbing_image == 3
    e = band.energies
    assert np.abs(e - e[::-1]).max() < 1e-6, e - e[::-1]
    mid = band.images[3]
    assert _same_up_to_permutation(mirror(mid), mid, lat) < 1e-4
    assert e[3] - e[0] > 0.0 and e.argmax() == 3


# ---- argument checks (no device needed: refused before any HIP call) ------------------------------------------------------------
def _init(image_offsets=(0, 2, 4), band_images=(0, 2), k=(0.1,), climb=(1,), energies=(0.0, 0.0), state_bytes=1 << 20):
    from torch_m3gnet import _lib

    lib = _lib.load_library()
    io = np.array(image_offsets, dtype=np.int64)
    bi = np.array(band_images, dtype=np.int32)
    kk = np.array(k, dtype=np.float64)
    cl = np.array(climb, dtype=np.int32)
    en = np.array(energies, dtype=np.float64)
    dummy = C.c_void_p(256)   # never dereferenced: the call returns at the checks
    return lib.m3g_neb_init(int(io[-1]), len(io) - 1, len(bi) - 1, io.ctypes.data, bi.ctypes.data, kk.ctypes.data, cl.ctypes.data, dummy,
                            en.ctypes.data, dummy, state_bytes, None)


@pytest.mark.parametrize("case,word", [(dict(image_offsets=(0, 3, 2, 4), band_images=(0, 3)), b"offsets"),
                                       (dict(image_offsets=(1, 2, 4)), b"offsets"),
                                       (dict(band_images=(0, 1)), b"band image offsets"),
                                       (dict(band_images=(1, 2)), b"band image offsets"),
                                       (dict(band_images=(0, 0, 2), k=(0.1, 0.1), climb=(1, 1), energies=(0,) * 4), b"no interior image"),
                                       (dict(band_images=(0, 3, 2), k=(0.1, 0.1), climb=(1, 1), energies=(0,) * 4), b"band image offsets"),
                                       (dict(image_offsets=(0, 2, 5)), b"different atom counts"),
                                       (dict(k=(0.0,)), b"spring constant"), (dict(k=(-0.1,)), b"spring constant"),
                                       (dict(k=(float("nan"),)), b"spring constant"), (dict(k=(float("inf"),)), b"spring constant"),
                                       (dict(climb=(2,)), b"climb"), (dict(climb=(-1,)), b"climb"),
                                       (dict(energies=(0.0, float("nan"))), b"endpoint energies")])
def test_c_abi_refuses_bad_neb_arguments(case, word):
    from torch_m3gnet import _lib

    assert _init(**case) == _lib.M3G_ERR_VALUE
    assert word in _lib.load_library().m3g_last_error()


def test_c_abi_neb_sizes():
    from torch_m3gnet import _lib

    lib = _lib.load_library()
    # valid arguments: the call gets past the checks and fails only on the deliberately too small state buffer
    assert _init(image_offsets=(0, 2, 4, 7, 10), band_images=(0, 2, 4), k=(0.1, 2.0), climb=(0, 1), energies=(0.0,) * 4, state_bytes=1) == _lib.M3G_ERR_SIZE
    size = C.c_size_t()
    assert lib.m3g_neb_state_bytes(10000, 5, 1, C.byref(size)) == _lib.M3G_OK and size.value > 10000 * 3 * 8 * 2
    for n, i, b in ((2, 3, 1), (4, 2, 3), (0, 1, 1), (4, 0, 0), (4, 2, 0)):
        assert lib.m3g_neb_state_bytes(n, i, b, C.byref(size)) == _lib.M3G_ERR_VALUE
    dummy = C.c_void_p(256)
    assert lib.m3g_neb_forces(2, 3, 1, dummy, 1 << 20, dummy, dummy, dummy, dummy, None, None) == _lib.M3G_ERR_VALUE
    assert lib.m3g_neb_forces(4, 2, 1, dummy, 1 << 20, dummy, dummy, None, dummy, None, None) == _lib.M3G_ERR_VALUE


def test_neb_argument_validation():
    from torch_m3gnet.model.build import build_model
    from torch_m3gnet.neb import NEB

    model = build_model(5.0, 4.0, 3, 3, 95, 16, 1)
    with pytest.raises(TypeError):
        NEB(model.model)
    with pytest.raises(TypeError, match="NEB"):   # names the driver that was constructed
        NEB(model.model)
    for kw in (dict(k=0.0), dict(k=-1.0), dict(k=float("nan")), dict(climb=2), dict(skin=0.0)):
        with pytest.raises(ValueError):
            NEB(model, **kw)
    neb = NEB(model)
    pos, lat = fcc(3.6)
    z = np.full(len(pos), 29)
    imgs = interpolate(lat, pos, pos + 0.1, 5)
    for kw in (dict(fmax=0.0), dict(fmax=float("inf")), dict(steps=-1), dict(steps=1.5), dict(endpoint_fmax=-1.0)):
        with pytest.raises(ValueError):
            neb.run([(lat, z, imgs)], **kw)
    for band in ((lat, z, imgs[:2]),                                   # M < 3
                 (lat, z, imgs[:2] + [imgs[2][:5]] + imgs[3:]),         # unequal atom counts
                 (lat, z[:5], imgs),                                    # species do not match the images
                 (np.zeros((3, 3)), z, imgs),                           # singular cell
                 (lat[:2], z, imgs),                                    # bad cell shape
                 (lat, z, imgs[:2] + [imgs[2] * np.nan] + imgs[3:]),    # non-finite positions
                 (lat, z)):
        with pytest.raises(ValueError):
            neb.run([band])
    with pytest.raises(ValueError):
        neb.run([])
