"""CPU checks of batched L-BFGS relaxation: the numpy restatement (tests/lbfgs_reference.py, the yardstick of the GPU tests) equals
the dense BFGS inverse-Hessian product, wraps its ring, rejects a zero-curvature pair, clips per row, relaxes the truncated
Lennard-Jones fcc cell of test_relax_cpu.py in fewer steps than FIRE, and the C ABI / Relaxer refuse bad arguments before touching a
device."""
import ctypes as C

import numpy as np
import pytest

import fire_reference as fr
import lbfgs_reference as lr
from test_relax_cpu import analytic_a0, fcc, lj


def _quadratic(n=5, seed=3):
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(3 * n, 3 * n))
    hess = a @ a.T / (3 * n) + 2.0 * np.eye(3 * n)   # symmetric positive definite, eigenvalues of order 1 .. 10
    x0 = rng.normal(size=(n, 3))
    return hess, x0, (lambda x: -(hess @ (x - x0).reshape(-1)).reshape(n, 3))


@pytest.mark.parametrize("steps", [1, 2, 4, 8])
def test_direction_equals_dense_bfgs_inverse_hessian_product(steps):
    """k <= memory pairs: H from H0 I by H <- (I - rho s y^T) H (I - rho y s^T) + rho s s^T, oldest pair first; p = -H grad."""
    hess, x0, force = _quadratic()
    ref = lr.LbfgsReference(x0 + 0.3 * np.random.default_rng(4).normal(size=x0.shape), np.eye(3) * 50, relax_cell=False, fmax=1e-12,
                            maxstep=0.05)   # (clipped steps: the pairs are no Newton steps, so H stays far from the true inverse)
    for _ in range(steps + 1):
        ref.step(force(ref.pos))
    assert ref.n_pairs == steps
    n = ref.X.size
    H = np.eye(n) / ref.p["alpha"]
    for s, y, rho in zip(ref.s, ref.y, ref.rho):
        s, y = s.reshape(-1), y.reshape(-1)
        assert rho == 1.0 / np.dot(y, s)
        V = np.eye(n) - rho * np.outer(y, s)
        H = V.T @ H @ V + rho * np.outer(s, s)
    grad = -force(ref.pos)
    dense = -(H @ grad.reshape(-1)).reshape(-1, 3)
    p = ref.direction(grad)
    assert np.abs(p - dense).max() <= 1e-12 * np.abs(dense).max()


def test_ring_wraps_at_memory():
    hess, x0, force = _quadratic()
    ref = lr.LbfgsReference(x0 + 0.5, np.eye(3) * 50, relax_cell=False, fmax=1e-12, memory=3, maxstep=0.01)
    kept, xs = [], []
    for k in range(5):
        ref.step(force(ref.pos))
        xs.append(ref.X.copy())
        if k == 3:
            kept = [s.copy() for s in ref.s]
            assert ref.n_pairs == 3 and ref.wrapped == 0
    assert ref.n_pairs == 3 and ref.wrapped == 1   # the fourth pair evicted the first
    assert np.array_equal(ref.s[0], kept[1]) and np.array_equal(ref.s[1], kept[2]) and np.array_equal(ref.s[2], xs[3] - xs[2])


def test_zero_curvature_pair_is_not_stored():
    """The same forces twice: y = 0, y.s = 0 -- ASE would divide by zero; here no pair is stored and the step stays finite."""
    f = np.array([[0.3, -0.1, 0.2], [-0.3, 0.1, -0.2]])
    ref = lr.LbfgsReference(np.zeros((2, 3)), np.eye(3) * 9, relax_cell=False, fmax=1e-6)
    ref.step(f)
    ref.step(f)
    assert ref.n_pairs == 0 and ref.rejected == 1 and ref.n_steps == 2 and not ref.flags & lr.ERROR
    assert np.isfinite(ref.pos).all()
    assert np.allclose(ref.pos, 2 * f / 70.0, rtol=1e-15)   # two steepest-descent steps of H0 = 1 / alpha


def test_clip_is_per_row():
    """One huge force on one atom: that row moves by exactly maxstep, the others keep their ratio to it (ASE's determine_step)."""
    f = np.zeros((4, 3))
    f[2] = [3e4, -4e4, 0.0]
    f[0] = [1.0, 0.0, 0.0]
    ref = lr.LbfgsReference(np.zeros((4, 3)), np.eye(3) * 9, relax_cell=False, fmax=1e-6)
    ref.step(f)
    moved = np.linalg.norm(ref.pos, axis=1)
    assert ref.clipped == 1 and moved[2] == pytest.approx(0.2, rel=1e-15)
    assert moved[0] == pytest.approx(0.2 / 5e4, rel=1e-14) and moved[1] == moved[3] == 0.0


def test_restatement_relaxes_lj_cell_to_analytic_lattice_constant_in_fewer_steps_than_fire():
    a0 = analytic_a0()
    pos, lat = fcc(3.45)
    pos = pos + np.random.default_rng(0).normal(0, 0.05, pos.shape)
    ref, (e, f, w) = lr.relax(pos, lat, lj, relax_cell=True, fmax=1e-3, steps=2000)
    assert ref.converged and 0 < ref.n_steps < 2000
    L = ref.lattice
    assert np.abs(L - np.diag(np.diag(L))).max() < 1e-3   # stays cubic
    a = np.diag(L) / 2
    assert np.abs(a - a0).max() < 1e-3, (a, a0)
    e0 = lj(*fcc(a0))[0]
    assert abs(e - e0) / len(pos) < 1e-5
    fire, _ = fr.relax(pos, lat, lj, relax_cell=True, fmax=1e-3, steps=2000)
    print(f"variable cell: L-BFGS {ref.n_steps} steps, FIRE {fire.n_steps} steps")
    assert fire.converged and ref.n_steps < fire.n_steps


def test_restatement_fixed_cell_keeps_cell_and_converges_in_fewer_steps_than_fire():
    pos0, lat = fcc(3.55)
    pos = pos0 + np.random.default_rng(2).normal(0, 0.05, pos0.shape)
    ref, (e, f, w) = lr.relax(pos, lat, lj, relax_cell=False, fmax=1e-3, steps=1000)
    assert ref.converged
    assert np.array_equal(ref.lattice, lat)
    assert (f ** 2).sum(1).max() < 1e-6
    # every s and y sums to zero over the atoms when the forces do: the crystal ends at the perfect sites shifted by the initial offset
    shift = (pos - pos0).mean(0)
    assert np.abs(ref.pos - (pos0 + shift)).max() < 1e-3
    fire, _ = fr.relax(pos, lat, lj, relax_cell=False, fmax=1e-3, steps=1000)
    print(f"fixed cell: L-BFGS {ref.n_steps} steps, FIRE {fire.n_steps} steps")
    assert fire.converged and ref.n_steps < fire.n_steps


# ---- argument checks (no device needed: refused before any HIP call) ------------------------------------------------------------
def _params(**kw):
    from torch_m3gnet import _lib
    from torch_m3gnet.relax import LBFGS_DEFAULTS

    p = dict(LBFGS_DEFAULTS, fmax=0.1, relax_cell=1)
    p.update(kw)
    return _lib.M3GLbfgsParams(**p)


@pytest.mark.parametrize("bad", [dict(memory=0), dict(memory=-3), dict(maxstep=0.0), dict(maxstep=float("inf")), dict(damping=-1.0),
                                 dict(damping=float("nan")), dict(alpha=0.0), dict(alpha=float("nan")), dict(fmax=0.0), dict(fmax=-0.1),
                                 dict(fmax=float("nan")), dict(relax_cell=2), dict(relax_cell=-1)])
def test_c_abi_refuses_invalid_lbfgs_parameters(bad):
    from torch_m3gnet import _lib

    lib = _lib.load_library()
    offs = np.array([0, 2], dtype=np.int64)
    dummy = C.c_void_p(256)   # never dereferenced: the call returns at the parameter check
    assert lib.m3g_lbfgs_init(C.byref(_params(**bad)), 2, 1, offs.ctypes.data, dummy, dummy, dummy, 1 << 30, None) == _lib.M3G_ERR_VALUE
    assert lib.m3g_lbfgs_step(C.byref(_params(**bad)), 2, 1, dummy, 1 << 30, dummy, dummy, dummy, dummy, dummy, 0, None, None) == _lib.M3G_ERR_VALUE


@pytest.mark.parametrize("offsets", [[0, 3, 2, 4], [0, 2, 2, 4], [1, 2, 3, 4], [0, 1, 2, 3]])
def test_c_abi_refuses_bad_offsets(offsets):
    from torch_m3gnet import _lib

    lib = _lib.load_library()
    offs = np.array(offsets, dtype=np.int64)
    dummy = C.c_void_p(256)
    assert lib.m3g_lbfgs_init(C.byref(_params()), 4, 3, offs.ctypes.data, dummy, dummy, dummy, 1 << 30, None) == _lib.M3G_ERR_VALUE
    assert b"offsets" in lib.m3g_last_error()


def test_c_abi_refuses_cell_relaxation_without_stresses_or_lattice_and_short_buffers():
    from torch_m3gnet import _lib

    lib = _lib.load_library()
    dummy = C.c_void_p(256)
    offs = np.array([0, 4], dtype=np.int64)
    assert lib.m3g_lbfgs_step(C.byref(_params()), 4, 1, dummy, 1 << 30, dummy, None, dummy, dummy, dummy, 0, None, None) == _lib.M3G_ERR_VALUE
    assert b"stresses" in lib.m3g_last_error()
    assert lib.m3g_lbfgs_step(C.byref(_params()), 4, 1, dummy, 1 << 30, dummy, dummy, dummy, None, dummy, 0, None, None) == _lib.M3G_ERR_VALUE
    assert lib.m3g_lbfgs_init(C.byref(_params()), 4, 1, offs.ctypes.data, dummy, None, dummy, 1 << 30, None) == _lib.M3G_ERR_VALUE
    size, small = C.c_size_t(), C.c_size_t()
    assert lib.m3g_lbfgs_state_bytes(10000, 3, 100, C.byref(size)) == _lib.M3G_OK
    rows = 10000 + 3 * 3
    assert 101 * 2 * 24 * rows < size.value < 1.2 * 101 * 2 * 24 * rows   # dominated by the rings of s and y
    assert lib.m3g_lbfgs_state_bytes(10000, 3, 5, C.byref(small)) == _lib.M3G_OK and small.value < size.value / 10
    assert lib.m3g_lbfgs_state_bytes(2, 3, 100, C.byref(size)) == _lib.M3G_ERR_VALUE
    assert lib.m3g_lbfgs_state_bytes(4, 1, 0, C.byref(size)) == _lib.M3G_ERR_VALUE
    # a short state buffer: M3G_ERR_SIZE from init, step and read, before any HIP call
    assert lib.m3g_lbfgs_state_bytes(4, 1, 100, C.byref(size)) == _lib.M3G_OK
    short = size.value - 1
    p = _params(relax_cell=0)
    assert lib.m3g_lbfgs_init(C.byref(p), 4, 1, offs.ctypes.data, dummy, None, dummy, short, None) == _lib.M3G_ERR_SIZE
    assert lib.m3g_lbfgs_step(C.byref(p), 4, 1, dummy, short, dummy, None, dummy, None, None, 0, None, None) == _lib.M3G_ERR_SIZE
    assert lib.m3g_lbfgs_read(4, 1, 100, dummy, short, None, None, None, None, None) == _lib.M3G_ERR_SIZE


def test_relaxer_optimizer_argument_validation():
    from torch_m3gnet.model.build import build_model
    from torch_m3gnet.relax import Relaxer

    model = build_model(5.0, 4.0, 3, 3, 95, 16, 1)
    assert Relaxer(model).optimizer == "fire"   # the default stays FIRE
    assert Relaxer(model, optimizer="lbfgs", memory=7).optimizer_params == {"memory": 7}
    with pytest.raises(ValueError):
        Relaxer(model, optimizer="bfgs")
    with pytest.raises(TypeError):
        Relaxer(model, optimizer="lbfgs", dtmax=1.0)   # a FIRE parameter
    with pytest.raises(TypeError):
        Relaxer(model, optimizer="fire", memory=5)
    with pytest.raises(TypeError):
        Relaxer(model.model, optimizer="lbfgs")
