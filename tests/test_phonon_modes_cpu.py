"""CPU checks of the phonon eigenvectors and group velocities: the C ABI of m3g_eigh_batched, m3g_ph_dynmat_gradient and
m3g_ph_group_velocities and the host functions refusing bad arguments before touching a device, and the numpy restatement
(tests/phonon_modes_reference.py, the yardstick of the GPU tests) against closed forms under the truncated-LJ fcc crystal of
tests/test_relax_cpu.py -- the gradient against the analytic lattice sum, velocities against central differences, the [100] sound
velocities against sqrt(C / rho), Gamma, the conventional cell against the folded primitive bands, the projected-DOS weights.

The force constants here are the analytic pair Hessians themselves (-K(R) inside RC, the self term from the sum rule), not finite
differences: the closed forms then hold to rounding."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import phonon_modes_reference as pm
import phonon_reference as pr
from test_phonons_cpu import FCC_BASE, FCC_PRIM, MASS, pair_hessian
from test_relax_cpu import RC, analytic_a0

ROOT = Path(__file__).resolve().parent.parent
C11, C44 = 3.139, 1.750   # eV/A^3: the lattice-sum constants of the clamped crystal


def exact_phonons(lattice, pos, n):
    """(Phi [n_u, N_s, 3, 3], image table) of the truncated LJ crystal from the analytic pair Hessian."""
    table = pr.image_table(lattice, pos, n)
    n_u, ns = len(pos), len(pos) * int(np.prod(n))
    phi = np.zeros((n_u, ns, 3, 3))
    for u in range(n_u):
        for j in range(ns):
            R = table[u, j][0] @ lattice
            if 1e-9 < np.linalg.norm(R) < RC:
                assert len(table[u, j]) == 1   # the supercell is wider than 2 RC: one image per pair inside RC
                phi[u, j] = -pair_hessian(R)
        phi[u, u] = -phi[u].sum(axis=0)
    return phi, table


@pytest.fixture(scope="module")
def crystal():
    a0 = analytic_a0()
    prim = a0 * FCC_PRIM
    conv = a0 * np.eye(3)
    return a0, (prim, np.zeros((1, 3)), [MASS]) + exact_phonons(prim, np.zeros((1, 3)), (6, 6, 6)), \
        (conv, FCC_BASE * a0, [MASS] * 4) + exact_phonons(conv, FCC_BASE * a0, (3, 3, 3))


def modes_at(cell, q_cart, direction=(1, 2, 3), tol=1e-4, cutoff=1e-3):
    lat, _, m, phi, table = cell
    q = pm.fractional_q(lat, q_cart)
    return pm.group_velocities(pr.dynamical_matrix(phi, table, m, q), pm.dynamical_matrix_gradient(phi, table, m, q, lat), direction, tol,
                               cutoff)


def test_gradient_equals_the_analytic_lattice_sum(crystal):
    _, (lat, _, m, phi, table), _ = crystal
    ns = np.stack(np.meshgrid(*[np.arange(-4, 5)] * 3, indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng(0)
    qs = [np.zeros(3), np.array([0, 0.5, 0.5]), np.array([0.25, 0.75, 0.5]), np.array([0.5, 0.5, 0.5])] + list(rng.uniform(-1, 1, (6, 3)))
    got, ref = [], []
    for q in qs:
        g = np.zeros((3, 3, 3))
        for nr in ns:
            R = nr @ lat
            if 1e-9 < np.linalg.norm(R) < RC:
                g += pair_hessian(R)[None] * (2 * np.pi * R * np.sin(2 * np.pi * np.dot(q, nr)))[:, None, None]
        ref.append(g / MASS)
        got.append(pm.dynamical_matrix_gradient(phi, table, m, q, lat))
    err = np.abs(np.array(got) - np.array(ref)).max() / np.abs(np.array(ref)).max()
    print(f"gradient against the analytic lattice sum: {err:.2e} of the largest entry")
    assert err <= 1e-10


H = 1e-4   # 1/A
# Central differences of the restatement's own frequencies at h = 1e-4 1/A: the O(h^2) term is h^2 f''' / 6, and it is what is seen --
# the deviation goes as h^2 (6.8e-6, 1.7e-6, 4.3e-7, 6.8e-8 of the largest velocity at h = 2e-4, 1e-4, 5e-5, 2e-5 in the primitive
# cell), rounding (eps f / h ~ 2e-11 THz A) is far below.  Measured at h = 1e-4 over the q-points below: 1.7e-6 in the primitive,
# 5.2e-6 in the conventional cell (bands that lie closer bend more); asserted at 10 x.
FD_BOUND = 5.2e-5


def test_velocities_equal_central_differences_at_generic_q(crystal):
    _, prim, conv = crystal
    rng = np.random.default_rng(1)
    worst = 0.0
    for cell in (prim, conv):
        lat, _, m, phi, table = cell
        for qc in rng.uniform(-0.12, 0.12, (4, 3)) + np.array([0.05, 0.02, -0.03]):
            f, v, sets, _ = modes_at(cell, qc)
            assert all(c - b == 1 for b, c in sets), (qc, f)   # generic: no degenerate set
            for a in range(3):
                e = np.zeros(3)
                e[a] = H
                fp = pr.frequencies(pr.dynamical_matrix(phi, table, m, pm.fractional_q(lat, qc + e)))
                fm = pr.frequencies(pr.dynamical_matrix(phi, table, m, pm.fractional_q(lat, qc - e)))
                worst = max(worst, np.abs(v[:, a] - (fp - fm) / (2 * H)).max() / np.abs(v).max())
    print(f"velocities against central differences (h = {H} 1/A): {worst:.2e} of the largest velocity")
    assert worst <= FD_BOUND


# At q = 0.01 1/A the dispersion lowers d f / d q below the sound velocity by terms of order (pi q a0)^2 ~ 1e-2 times a coefficient
# below one, and the lattice-sum constants carry four digits (3e-4).  Measured: longitudinal 7.7e-4, transverse 1.73e-3 below
# sqrt(C / rho); asserted at 3 x the larger.
SOUND_BOUND = 3 * 1.73e-3


def test_sound_velocities_along_100(crystal):
    a0, prim, conv = crystal
    rho = 4 * MASS / a0 ** 3
    vl, vt = (2 * np.pi * pm.THZ * np.sqrt(c / rho) for c in (C11, C44))
    for cell in (prim, conv):
        f, v, sets, w = modes_at(cell, np.array([0.01, 0.0, 0.0]))
        assert sets[0] == (0, 2) and sets[1] == (2, 3), (f, sets)   # the two transverse modes are one degenerate set
        dl, dt = v[2, 0] / vl - 1, v[:2, 0] / vt - 1
        print(f"[100] sound velocities: v_L {v[2, 0]:.4f} ({dl:+.2e} of sqrt(C11 / rho)), v_T {v[0, 0]:.4f} {v[1, 0]:.4f} ({dt[0]:+.2e})")
        assert abs(dl) <= SOUND_BOUND and np.abs(dt).max() <= SOUND_BOUND
        assert np.abs(v[:3, 1:]).max() <= 1e-9 * vl                    # along x by symmetry
        assert abs(v[0, 0] - v[1, 0]) <= 1e-9 * vt                     # the set's W has two equal eigenvalues along (1, 2, 3)


def test_every_velocity_is_zero_at_gamma(crystal):
    _, prim, conv = crystal
    for cell in (prim, conv):
        f, v, _, _ = modes_at(cell, np.zeros(3))
        assert np.abs(f[:3]).max() < 1e-3
        assert (v[:3] == 0.0).all()                                    # the cutoff rule: exactly 0
        assert np.abs(v).max() <= 1e-9 * 2 * np.pi * pm.THZ            # and the optical modes of the folded cell are stationary


def test_conventional_cell_gives_the_primitive_set_traces(crystal):
    """The conventional cell's bands are the primitive ones at the four folded points: where they cross (zone faces, Gamma) the
    eigenvectors are not unique, the sum of v over each degenerate set is."""
    a0, prim, conv = crystal
    rng = np.random.default_rng(2)
    worst, scale = 0.0, 0.0   # (every velocity is zero at some of the points: one scale for the whole set)
    for q_frac in [np.array([0.5, 0, 0]), np.array([0.5, 0.5, 0.5]), np.array([0.25, 0.5, 0]), np.array([0.5, 0.5, 0]),
                   np.array([0.3, 0.0, 0.0])] + list(rng.uniform(-0.5, 0.5, (3, 3))):
        f, v, sets, _ = modes_at(conv, q_frac / a0)
        fp, vp = [], []
        for g in np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]):
            a, b, _, _ = modes_at(prim, (q_frac + g) / a0)
            fp.extend(a)
            vp.extend(b)
        order = np.argsort(fp, kind="stable")
        fp, vp = np.array(fp)[order], np.array(vp)[order]
        assert np.abs(f - fp).max() <= 1e-8 * np.abs(fp).max()
        assert max(c - b for b, c in sets) > 1 or np.abs(q_frac).min() > 0
        worst, scale = max(worst, np.abs(pm.set_traces(v, sets) - pm.set_traces(vp, sets)).max()), max(scale, np.abs(vp).max())
    print(f"conventional against primitive per-set velocity traces: {worst / scale:.2e} of the largest velocity")
    assert worst <= 1e-8 * scale   # rounding (1e-16) times the condition THZ^2 / (2 f) |dD| / |v| of the quotient, ~1e3 at most, with room


def test_projected_dos_weights_sum_to_one(crystal):
    from torch_m3gnet.phonons import gaussian_dos, projected_gaussian_dos

    _, _, (lat, _, m, phi, table) = crystal
    qs = np.random.default_rng(3).uniform(-0.5, 0.5, (5, 3))
    f, p = [], []
    for q in qs:
        lam, e = np.linalg.eigh(pr.dynamical_matrix(phi, table, m, q))
        w = pm.projection_weights(e, 4)
        assert w.shape == (4, 12) and np.abs(w.sum(axis=0) - 1).max() <= 1e-13
        f.append(np.sign(lam) * np.sqrt(np.abs(lam)) * pm.THZ)
        p.append(w)
    grid, wq = torch.linspace(-1, 12, 131, dtype=torch.float64), torch.full((5,), 0.2, dtype=torch.float64)
    part = projected_gaussian_dos(torch.tensor(np.array(f)), torch.tensor(np.array(p)), wq, grid, 0.2)
    total = gaussian_dos(torch.tensor(np.array(f)), wq, grid, 0.2)
    assert part.shape == (4, 131) and float((part.sum(0) - total).abs().max()) <= 1e-12 * float(total.max())


# ---- the C ABI and the host functions: refused before any HIP call ---------------------------------------------------------------------
def test_header_constants_equal_the_bindings():
    from torch_m3gnet import _lib
    from torch_m3gnet.phonons import THZ_PER_SQRT_EV_A2_AMU

    header = (ROOT / "include" / "m3gnet_hip.h").read_text()
    value = lambda name: re.search(rf"#define {name} (\S+)", header).group(1)
    assert int(value("M3G_EIGH_MAX_N")) == _lib.EIGH_MAX_N >= 48 and int(value("M3G_EIGH_MAX_SWEEPS")) == _lib.EIGH_MAX_SWEEPS == 30
    assert int(value("M3G_EIGH_SWEEPS_MASK"), 16) == _lib.EIGH_SWEEPS_MASK and int(value("M3G_EIGH_NONFINITE"), 16) == _lib.EIGH_NONFINITE
    assert int(value("M3G_EIGH_NOT_CONVERGED"), 16) == _lib.EIGH_NOT_CONVERGED
    assert int(value("M3G_PH_GV_MAX_N")) == _lib.PH_GV_MAX_N and int(value("M3G_PH_GV_MAX_SET")) == _lib.PH_GV_MAX_SET
    assert float(value("M3G_PH_THZ")) == _lib.PH_THZ == THZ_PER_SQRT_EV_A2_AMU == pm.THZ
    assert int(value("M3G_ABI_VERSION")) == _lib.ABI_VERSION == 11


def test_c_abi_refuses_bad_eigh_arguments():
    from torch_m3gnet import _lib

    lib = _lib.load_library()
    d = C.c_void_p(256)   # never dereferenced: the calls return at the checks
    for m, n, a, want, w, v, info in ((-1, 4, d, 1, d, d, d), (3, 0, d, 1, d, d, d), (3, -2, d, 1, d, d, d), (3, _lib.EIGH_MAX_N + 1, d, 1, d, d, d),
                                      (3, 4, None, 1, d, d, d), (3, 4, d, 1, None, d, d), (3, 4, d, 1, d, None, d), (3, 4, d, 1, d, d, None),
                                      (3, 4, d, 2, d, d, d), (0, 4, None, 0, d, None, d)):
        assert lib.m3g_eigh_batched(m, n, a, want, w, v, info, None) == _lib.M3G_ERR_VALUE, (m, n, want)
    assert b"M3G_EIGH_MAX_N" in lib.m3g_last_error() or b"null" in lib.m3g_last_error()
    assert lib.m3g_eigh_batched(0, 4, d, 1, d, d, d, None) == _lib.M3G_OK          # nothing to do
    assert lib.m3g_eigh_batched(0, _lib.EIGH_MAX_N, d, 0, d, None, d, None) == _lib.M3G_OK   # no eigenvectors asked for: none needed


def test_c_abi_refuses_bad_gradient_and_velocity_arguments():
    from torch_m3gnet import _lib

    lib = _lib.load_library()
    d = C.c_void_p(256)
    sz = _lib.M3GPhSizes(1, 4, 108, 432)
    for n_q, max_nu in ((-1, 4), (3, 0), (3, 5)):
        assert lib.m3g_ph_dynmat_gradient(C.byref(sz), d, 1 << 30, d, n_q, d, d, max_nu, d, None) == _lib.M3G_ERR_VALUE
    assert lib.m3g_ph_dynmat_gradient(C.byref(sz), None, 1 << 30, d, 3, d, d, 4, d, None) == _lib.M3G_ERR_VALUE
    assert lib.m3g_ph_dynmat_gradient(C.byref(sz), d, 1 << 30, d, 3, d, d, 4, None, None) == _lib.M3G_ERR_VALUE
    assert lib.m3g_ph_dynmat_gradient(C.byref(sz), d, 1, d, 3, d, d, 4, d, None) == _lib.M3G_ERR_SIZE
    # the q-count limit holds for the tripled grid: 2^26 workgroups fit the plain launch, not this one
    assert lib.m3g_ph_dynmat_gradient(C.byref(sz), d, 1 << 30, d, 1 << 25, d, d, 4, d, None) == _lib.M3G_ERR_VALUE
    assert b"too many q-points" in lib.m3g_last_error()
    assert lib.m3g_ph_dynmat_gradient(C.byref(sz), d, 1 << 30, d, 0, None, None, 4, None, None) == _lib.M3G_OK

    unit = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    call = lambda n_q=3, n=12, w=d, e=d, g=d, tol=1e-4, cut=1e-3, direction=unit, v=d: lib.m3g_ph_group_velocities(
        n_q, n, w, e, g, tol, cut, None if direction is None else np.ascontiguousarray(direction, dtype=np.float64).ctypes.data, v, None)
    for kw in (dict(n_q=-1), dict(n=0), dict(n=-3), dict(n=_lib.PH_GV_MAX_N + 1), dict(w=None), dict(e=None), dict(g=None), dict(v=None),
               dict(direction=None), dict(direction=[1.0, 2.0, 3.0]), dict(direction=[0.0, 0.0, 0.0]), dict(direction=[np.nan, 0.0, 1.0]),
               dict(direction=[np.inf, 0.0, 0.0]), dict(direction=unit * (1 + 1e-9)), dict(tol=-1.0), dict(tol=np.nan), dict(cut=-1e-3),
               dict(cut=np.inf)):
        assert call(**kw) == _lib.M3G_ERR_VALUE, kw
    assert call(n_q=0) == _lib.M3G_OK and call(n_q=0, w=None, e=None, g=None, v=None, n=_lib.PH_GV_MAX_N) == _lib.M3G_OK


def test_host_functions_refuse_bad_arguments():
    from torch_m3gnet import _lib
    from torch_m3gnet.linalg import EIGH_MAX_N, eigh_batched
    from torch_m3gnet.model.build import build_model
    from torch_m3gnet.phonons import Phonons, ph_group_velocities, unit_direction

    assert EIGH_MAX_N == _lib.EIGH_MAX_N
    a = torch.zeros(2, 4, 4, dtype=torch.complex128)
    for bad in (a[0, 0], torch.zeros(2, 4, 3, dtype=torch.complex128), a.to(torch.complex64), a.real.float(), np.zeros((4, 4)),
                torch.zeros(2, 0, 0, dtype=torch.complex128), a):   # (the last: not on a GPU)
        with pytest.raises(ValueError):
            eigh_batched(bad)
    with pytest.raises(ValueError, match=f"EIGH_MAX_N = {EIGH_MAX_N}"):
        eigh_batched(torch.zeros(1, EIGH_MAX_N + 1, EIGH_MAX_N + 1, dtype=torch.complex128))
    with pytest.raises(ValueError, match="eigenvectors"):
        eigh_batched(a, eigenvectors=1)

    model = build_model(5.0, 4.0, 3, 3, 95, 16, 1)
    for name in ("Jacobi", "eigh", None, 1):
        with pytest.raises(ValueError, match="eigensolver"):
            Phonons(model, eigensolver=name)
    assert Phonons(model).eigensolver == "embedding" and Phonons(model, eigensolver="jacobi").eigensolver == "jacobi"

    assert np.allclose(unit_direction((1, 2, 3)), np.array([1, 2, 3]) / np.sqrt(14))
    w, e, g = torch.zeros(2, 3, dtype=torch.float64), torch.zeros(2, 3, 3, dtype=torch.complex128), torch.zeros(2, 3, 3, 3, dtype=torch.complex128)
    for direction in ((0, 0, 0), (1, 2), (1, float("nan"), 0), (float("inf"), 0, 0)):
        with pytest.raises(ValueError, match="direction"):
            ph_group_velocities(w, e, g, direction)
    for tol in (-1e-4, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="degeneracy_tolerance"):
            ph_group_velocities(w, e, g, (1, 0, 0), tol)
    with pytest.raises(ValueError, match="cutoff_frequency"):
        ph_group_velocities(w, e, g, (1, 0, 0), 1e-4, -1.0)
    with pytest.raises(ValueError, match="GPU"):
        ph_group_velocities(w, e, g, (1, 0, 0))
