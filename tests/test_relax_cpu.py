"""CPU checks of batched FIRE relaxation: the numpy restatement (tests/fire_reference.py, the yardstick of the GPU tests) relaxes a
truncated Lennard-Jones fcc cell with its cell to the analytic lattice constant, and the C ABI / Relaxer refuse bad arguments before
touching a device."""
import ctypes as C
import itertools

import numpy as np
import pytest

import fire_reference as fr

EPS, SIGMA, RC = 0.4, 2.3, 5.3   # eV, A, A (RC lies between the 4th and 5th fcc shells near the minimum)
FCC_BASE = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])
SHIFTS = np.array(list(itertools.product((-1, 0, 1), repeat=3)), dtype=np.float64)


def fcc(a, n=2):
    grid = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1).reshape(-1, 1, 3)
    return (grid + FCC_BASE[None]).reshape(-1, 3) * a, np.eye(3) * n * a


def lj(pos, lattice):
    """Energy, forces and virial W = -dE/d eps of the truncated (unshifted) LJ potential over explicit image shifts."""
    widths = abs(np.linalg.det(lattice)) / np.linalg.norm(np.cross(lattice[[1, 2, 0]], lattice[[2, 0, 1]]), axis=1)
    assert widths.min() > RC   # one image in each direction suffices
    frac = np.linalg.solve(lattice.T, pos.T).T
    pos = (frac - np.floor(frac)) @ lattice   # wrapped (forces and virial do not change)
    rij = pos[None, :, None, :] + (SHIFTS @ lattice)[None, None, :, :] - pos[:, None, None, :]   # [i, j, shift, 3]
    r = np.linalg.norm(rij, axis=-1)
    mask = (r > 1e-9) & (r < RC)
    rs = np.where(mask, r, 1.0)
    sr6 = (SIGMA / rs) ** 6
    phi = np.where(mask, 4 * EPS * (sr6 * sr6 - sr6), 0.0)
    dphi = np.where(mask, 4 * EPS * (-12 * sr6 * sr6 + 6 * sr6) / rs, 0.0)   # d phi / d r
    unit = rij / rs[..., None]
    e = 0.5 * phi.sum()
    f = (dphi[..., None] * unit).sum(axis=(1, 2))
    w = -0.5 * np.einsum("ijs,ijsa,ijsb->ab", dphi * rs, unit, unit)
    return e, f, w


def analytic_a0():
    """Minimum of the truncated LJ lattice sum: a^6 = 2 sigma^6 S12 / S6 over the shells inside RC (a fixed point)."""
    pts = (np.stack(np.meshgrid(*[np.arange(-4, 5)] * 3, indexing="ij"), -1).reshape(-1, 1, 3) + FCC_BASE[None]).reshape(-1, 3)
    d = np.linalg.norm(pts, axis=1)
    d = d[d > 1e-9]
    a = 1.5422 * SIGMA
    for _ in range(20):
        inside = d * a < RC
        a = SIGMA * (2 * (d[inside] ** -12.0).sum() / (d[inside] ** -6.0).sum()) ** (1 / 6)
    return a


def test_lj_yardstick_forces_and_virial_are_derivatives():
    rng = np.random.default_rng(1)
    pos, lat = fcc(3.5)
    pos = pos + rng.normal(0, 0.05, pos.shape)
    lat = lat + rng.normal(0, 0.02, (3, 3))
    e, f, w = lj(pos, lat)
    h = 1e-5
    for i, k in [(0, 0), (5, 1), (17, 2)]:
        dp = np.zeros_like(pos)
        dp[i, k] = h
        fd = -(lj(pos + dp, lat)[0] - lj(pos - dp, lat)[0]) / (2 * h)
        assert abs(fd - f[i, k]) < 1e-6 * max(1.0, abs(f[i, k]))
    for a, b in [(0, 0), (1, 2), (2, 0)]:
        eps = np.zeros((3, 3))
        eps[a, b] += 0.5 * h
        eps[b, a] += 0.5 * h
        dfm = np.eye(3) + eps
        fd = -(lj(pos @ dfm, lat @ dfm)[0] - lj(pos @ (np.eye(3) - eps), lat @ (np.eye(3) - eps))[0]) / (2 * h)
        assert abs(fd - w[a, b]) < 1e-5 * max(1.0, np.abs(w).max())


def test_restatement_relaxes_lj_cell_to_analytic_lattice_constant():
    a0 = analytic_a0()
    pos, lat = fcc(3.45)
    pos = pos + np.random.default_rng(0).normal(0, 0.05, pos.shape)
    ref, (e, f, w) = fr.relax(pos, lat, lj, relax_cell=True, fmax=1e-3, steps=2000)
    assert ref.converged and 0 < ref.n_steps < 2000
    L = ref.lattice
    assert np.abs(L - np.diag(np.diag(L))).max() < 1e-3   # stays cubic
    a = np.diag(L) / 2
    assert np.abs(a - a0).max() < 1e-3, (a, a0)
    # energy per atom at the analytic minimum (perfect crystal)
    e0 = lj(*fcc(a0))[0]
    assert abs(e - e0) / len(pos) < 1e-5


def test_restatement_fixed_cell_keeps_cell_and_converges():
    pos0, lat = fcc(3.55)
    pos = pos0 + np.random.default_rng(2).normal(0, 0.05, pos0.shape)
    ref, (e, f, w) = fr.relax(pos, lat, lj, relax_cell=False, fmax=1e-3, steps=1000)
    assert ref.converged
    assert np.array_equal(ref.lattice, lat)
    assert (f ** 2).sum(1).max() < 1e-6
    # FIRE conserves sum v when sum f = 0: the crystal ends at the perfect sites shifted by the initial centre-of-mass offset
    shift = (pos - pos0).mean(0)
    assert np.abs(ref.pos - (pos0 + shift)).max() < 1e-3


def test_restatement_branches():
    """The first step takes no branch; P <= 0 resets v, a and dt; P > 0 for more than Nmin steps grows dt; maxstep clips |dr|."""
    ref = fr.FireReference(np.zeros((2, 3)), np.eye(3) * 5, relax_cell=False, fmax=1e-6)
    g = np.array([[1.0, 0, 0], [0, 1.0, 0]])
    ref.step(g)
    assert ref.dt == 0.1 and ref.n == 0 and np.allclose(ref.v, 0.1 * g)
    for _ in range(7):
        ref.step(g)
    assert ref.n == 7 and ref.dt == pytest.approx(0.1 * 1.1) and ref.a == pytest.approx(0.1 * 0.99)   # grown once: at n = 6 > Nmin
    ref.step(-g)
    assert ref.n == 0 and ref.a == 0.1 and ref.dt == pytest.approx(0.5 * 0.1 * 1.1)
    x = ref.X.copy()
    ref.step(-1e4 * g)
    assert np.linalg.norm(ref.X - x) == pytest.approx(0.2)


# ---- argument checks (no device needed: refused before any HIP call) ------------------------------------------------------------
def _params(**kw):
    from torch_m3gnet import _lib
    from torch_m3gnet.relax import FIRE_DEFAULTS

    p = dict(FIRE_DEFAULTS, fmax=0.1, relax_cell=1)
    p.update(kw)
    return _lib.M3GFireParams(**p)


@pytest.mark.parametrize("bad", [dict(fmax=0.0), dict(fmax=-0.1), dict(fmax=float("nan")), dict(dt=0.0), dict(maxstep=-1.0),
                                 dict(fa=1.5), dict(nmin=-1), dict(relax_cell=2)])
def test_c_abi_refuses_invalid_fire_parameters(bad):
    from torch_m3gnet import _lib

    lib = _lib.load_library()
    offs = np.array([0, 2], dtype=np.int64)
    dummy = C.c_void_p(256)   # never dereferenced: the call returns at the parameter check
    assert lib.m3g_fire_init(C.byref(_params(**bad)), 2, 1, offs.ctypes.data, dummy, dummy, dummy, 1 << 20, None) == _lib.M3G_ERR_VALUE
    assert lib.m3g_fire_step(C.byref(_params(**bad)), 2, 1, dummy, 1 << 20, dummy, dummy, dummy, dummy, dummy, 0, None, None) == _lib.M3G_ERR_VALUE


@pytest.mark.parametrize("offsets", [[0, 3, 2, 4], [0, 2, 2, 4], [1, 2, 3, 4], [0, 1, 2, 3]])
def test_c_abi_refuses_bad_offsets(offsets):
    from torch_m3gnet import _lib

    lib = _lib.load_library()
    offs = np.array(offsets, dtype=np.int64)
    dummy = C.c_void_p(256)
    assert lib.m3g_fire_init(C.byref(_params()), 4, 3, offs.ctypes.data, dummy, dummy, dummy, 1 << 20, None) == _lib.M3G_ERR_VALUE
    assert b"offsets" in lib.m3g_last_error()


def test_c_abi_refuses_cell_relaxation_without_stresses():
    from torch_m3gnet import _lib

    lib = _lib.load_library()
    dummy = C.c_void_p(256)
    assert lib.m3g_fire_step(C.byref(_params(relax_cell=1)), 4, 1, dummy, 1 << 20, dummy, None, dummy, dummy, dummy, 0, None, None) == _lib.M3G_ERR_VALUE
    assert b"stresses" in lib.m3g_last_error()
    size = C.c_size_t()
    assert lib.m3g_fire_state_bytes(10000, 3, C.byref(size)) == _lib.M3G_OK and size.value > 10000 * 2 * 24
    assert lib.m3g_fire_state_bytes(2, 3, C.byref(size)) == _lib.M3G_ERR_VALUE


def test_relaxer_argument_validation():
    from torch_m3gnet.model.build import build_model
    from torch_m3gnet.relax import Relaxer

    model = build_model(5.0, 4.0, 3, 3, 95, 16, 1)
    with pytest.raises(TypeError):
        Relaxer(model.model)
    with pytest.raises(ValueError):
        Relaxer(model, skin=0.0)
    r = Relaxer(model)
    pos, lat = fcc(3.6)
    z = np.full(len(pos), 29)
    for kw in (dict(fmax=0.0), dict(fmax=-1.0), dict(fmax=float("inf")), dict(steps=-1), dict(steps=1.5)):
        with pytest.raises(ValueError):
            r.relax([lat], [pos], [z], **kw)
    with pytest.raises(ValueError):
        r.relax([lat, lat], [pos], [z])
    with pytest.raises(ValueError):
        r.relax([lat], [pos[:5]], [z])
    with pytest.raises(ValueError):
        r.relax([np.zeros((3, 3))], [pos], [z])
    with pytest.raises(ValueError):
        r.relax([lat[:2]], [pos], [z])
