"""CPU checks of batched molecular dynamics: the numpy restatement (tests/md_reference.py, the yardstick of the GPU tests) -- its
Philox against numpy's generator, NVE on the truncated-LJ yardstick of tests/test_relax_cpu.py (second-order energy error, time
reversal), the Berendsen scaling law and clamps, Langevin (BAOAB) equipartition on harmonic oscillators, NPT Berendsen to the analytic
lattice constant -- the default mass table, and the C ABI / MolecularDynamics refusing bad arguments before touching a device."""
import ctypes as C

import numpy as np
import pytest

import md_reference as mr
from test_relax_cpu import analytic_a0, fcc, lj

CU = 63.546


def _mb(masses, temperature, seed):
    from torch_m3gnet.dynamics import maxwell_boltzmann

    return maxwell_boltzmann(masses, temperature, seed)


# ---- Philox4x64-10 ---------------------------------------------------------------------------------------------------------------
def test_philox_known_answer_and_numpy_generator():
    w = mr.philox4x64_10(np.array([1, 0, 0, 0], np.uint64), np.array([0, 0], np.uint64))
    assert [int(x) for x in w] == [0x02F4BA6408E4D89B, 0x3DD62B0B9CA8C5B2, 0x1C8667A55D902E79, 0x907D7A052FD5B4DC]
    rng = np.random.default_rng(11)
    ctrs = rng.integers(1, 2 ** 63, (20, 4), dtype=np.uint64)
    keys = rng.integers(0, 2 ** 63, (20, 2), dtype=np.uint64) * np.uint64(2) + np.uint64(1)   # odd keys, top bit set
    got = mr.philox4x64_10(ctrs, keys)
    for c, k, g in zip(ctrs, keys, got):
        # numpy increments its 256-bit counter before each block: the block of counter c is the first of Philox(counter=c - 1)
        prev = c.copy()
        prev[0] -= np.uint64(1)
        ref = np.random.Philox(counter=prev, key=k).random_raw(4)
        assert np.array_equal(ref, g)


def test_gaussians_are_standard_normal_and_depend_on_counter_and_key():
    xi = mr.gaussians(123, 0, 100_000)
    assert abs(xi.mean()) < 0.01 and abs(xi.std() - 1.0) < 0.01
    assert np.array_equal(mr.gaussians(123, 0, 10), xi[:10])   # an atom's noise does not depend on how many atoms follow
    assert not np.array_equal(mr.gaussians(123, 1, 10), xi[:10]) and not np.array_equal(mr.gaussians(124, 0, 10), xi[:10])


# ---- NVE on the LJ yardstick -----------------------------------------------------------------------------------------------------
def _nve(pos, lat, vel, dt, n_steps):
    ref = mr.DynReference(pos, lat, np.full(len(pos), CU), vel, "nve", dt=dt)
    energies = []
    for k in range(n_steps + 1):
        e, f, _ = lj(ref.pos, lat)
        ref.step(f, finish_only=(k == n_steps))
        energies.append(e + ref.obs[0])
    return ref, np.array(energies)


def test_restatement_nve_energy_error_is_second_order():
    pos, lat = fcc(3.55)
    pos = pos + np.random.default_rng(3).normal(0, 0.02, pos.shape)
    vel = _mb(np.full(len(pos), CU), 100.0, 3)
    _, e2 = _nve(pos, lat, vel, 2.0, 100)
    _, e1 = _nve(pos, lat, vel, 1.0, 200)
    d2, d1 = np.abs(e2 - e2[0]).max(), np.abs(e1 - e1[0]).max()
    assert 0 < d1 < 1e-3 and 2.5 < d2 / d1 < 6.0, (d1, d2)


def test_restatement_nve_is_time_reversible():
    pos0, lat = fcc(3.55)
    pos0 = pos0 + np.random.default_rng(4).normal(0, 0.02, pos0.shape)
    vel = _mb(np.full(len(pos0), CU), 100.0, 4)
    fwd, _ = _nve(pos0, lat, vel, 2.0, 60)
    assert np.abs(fwd.pos - pos0).max() > 0.05
    back, _ = _nve(fwd.pos, lat, -fwd.v, 2.0, 60)
    assert np.abs(back.pos - pos0).max() < 1e-9
    assert np.abs(back.v + vel).max() < 1e-9


# ---- Berendsen ---------------------------------------------------------------------------------------------------------------------
def test_restatement_berendsen_scaling_and_clamps():
    n = 50
    m = np.random.default_rng(5).uniform(1.0, 100.0, n)
    zero = np.zeros((n, 3))
    for t0, taut, lam_expect in ((300.0, 10.0, None), (3000.0, 10.0, 1.1), (0.0, 2.0, 0.9)):
        ref = mr.DynReference(np.zeros((n, 3)), np.eye(3) * 10, m, _mb(m, 200.0, 6), "nvt_berendsen", temperature=t0, dt=1.0, taut=taut)
        temps, lams = [], []
        for _ in range(6):
            ref.step(zero)
            temps.append(ref.obs[1])
            lams.append(ref.lam)
        for k in range(5):
            assert temps[k + 1] == pytest.approx(lams[k] ** 2 * temps[k], rel=1e-12)
        if lam_expect is None:
            assert 1.0 < lams[0] < 1.1 and temps[0] == pytest.approx(200.0, rel=1e-12)
        else:
            assert lams[0] == lam_expect
    ref = mr.DynReference(np.zeros((n, 3)), np.eye(3) * 10, m, zero, "nvt_berendsen", temperature=300.0)
    ref.step(zero)
    assert ref.obs[1] == 0.0 and ref.lam == 1.1 and not ref.v.any()


# ---- Langevin (BAOAB) ------------------------------------------------------------------------------------------------------------
def test_restatement_langevin_equipartition_on_harmonic_oscillators():
    n, m, dt, omega, t0 = 4000, 10.0, 1.0, 0.1, 300.0   # omega dt = 0.1
    k_spring = m * omega ** 2 / mr.KAPPA                # eV/A^2
    ref = mr.DynReference(np.zeros((n, 3)), np.eye(3) * 100, np.full(n, m), np.zeros((n, 3)), "nvt_langevin", temperature=t0, seed=7,
                          dt=dt, friction=0.05)
    ke, kx2 = [], []
    for step in range(2000):
        x = ref.pos
        if step >= 500:
            kx2.append(k_spring * (x * x).mean())
        ref.step(-k_spring * x)
        if step >= 500:
            ke.append(ref.obs[0])
    kt = mr.KB * t0
    assert np.mean(ke) == pytest.approx(1.5 * n * kt, rel=0.02)
    assert np.mean(kx2) == pytest.approx(kt, rel=0.02)


# ---- NPT Berendsen -------------------------------------------------------------------------------------------------------------------
def test_restatement_npt_berendsen_reaches_analytic_lattice_constant():
    a0 = analytic_a0()
    pos, lat = fcc(3.45)
    m = np.full(len(pos), CU)
    ref = mr.DynReference(pos, lat, m, _mb(m, 1.0, 8), "npt_berendsen", temperature=1.0, dt=2.0, taut=20.0, pressure=0.0, taup=200.0,
                          compressibility=0.5)
    for _ in range(1000):
        _, f, w = lj(ref.pos, ref.lattice)
        vol = abs(np.linalg.det(ref.lattice))
        ref.step(f, np.array([w[0, 0], w[1, 1], w[2, 2], w[1, 2], w[2, 0], w[0, 1]]) / vol)
    L = ref.lattice
    assert np.abs(L - np.diag(np.diag(L))).max() < 1e-9
    assert np.abs(np.diag(L) / 2 - a0).max() < 1e-3, (np.diag(L) / 2, a0)
    assert ref.obs[1] < 5.0


# ---- mass table ----------------------------------------------------------------------------------------------------------------------
def test_default_mass_table():
    from torch_m3gnet.data.atomic_masses import ATOMIC_MASSES, masses_of

    assert len(ATOMIC_MASSES) == 95 and (ATOMIC_MASSES > 0).all()
    spot = {1: 1.008, 6: 12.011, 8: 15.999, 13: 26.982, 22: 47.867, 29: 63.546, 42: 95.95}
    assert np.array_equal(masses_of(list(spot)), np.array(list(spot.values())))
    assert masses_of([43, 94, 95]).tolist() == [97.0, 244.0, 243.0]
    for bad in ([0], [96], [1.5]):
        with pytest.raises(ValueError):
            masses_of(bad)


def test_maxwell_boltzmann_zero_momentum_and_exact_temperature():
    m = np.random.default_rng(9).uniform(1.0, 200.0, 64)
    v = _mb(m, 450.0, 1)
    assert np.abs((m[:, None] * v).sum(0)).max() < 1e-12
    t = (m * (v * v).sum(1)).sum() / mr.KAPPA / (3 * len(m) * mr.KB)
    assert t == pytest.approx(450.0, rel=1e-12)
    assert np.array_equal(v, _mb(m, 450.0, 1)) and not np.array_equal(v, _mb(m, 450.0, 2))
    assert not _mb(m, 0.0, 1).any() and not _mb(m[:1], 300.0, 1).any()


# ---- argument checks (no device needed: refused before any HIP call) ------------------------------------------------------------
def _params(**kw):
    from torch_m3gnet import _lib

    p = dict(ensemble=_lib.DYN_NPT_BERENDSEN, fix_com=1, dt=1.0, taut=100.0, friction=0.01, pressure=0.0, taup=1000.0, compressibility=1.0)
    p.update(kw)
    return _lib.M3GDynParams(**p)


def _init(params, offsets=(0, 2), masses=(1.0, 1.0), temps=(300.0,)):
    from torch_m3gnet import _lib

    lib = _lib.load_library()
    offs = np.array(offsets, dtype=np.int64)
    m = np.array(masses, dtype=np.float64)
    t = np.array(temps, dtype=np.float64)
    seeds = np.zeros(len(t), dtype=np.uint64)
    dummy = C.c_void_p(256)   # never dereferenced: the call returns at the checks
    return lib.m3g_dyn_init(C.byref(params), int(offs[-1]), len(offs) - 1, offs.ctypes.data, m.ctypes.data, t.ctypes.data, seeds.ctypes.data,
                            dummy, dummy, 1 << 20, None)


@pytest.mark.parametrize("bad", [dict(ensemble=4), dict(ensemble=-1), dict(fix_com=2), dict(dt=0.0), dict(dt=float("nan")), dict(taut=0.0),
                                 dict(taup=-1.0), dict(compressibility=0.0), dict(compressibility=float("inf")), dict(friction=-0.1),
                                 dict(pressure=float("nan")), dict(ensemble=2, fix_com=1), dict(ensemble=1, taut=float("inf"))])
def test_c_abi_refuses_invalid_dynamics_parameters(bad):
    from torch_m3gnet import _lib

    lib = _lib.load_library()
    assert _init(_params(**bad)) == _lib.M3G_ERR_VALUE
    dummy = C.c_void_p(256)
    assert lib.m3g_dyn_step(C.byref(_params(**bad)), 2, 1, dummy, 1 << 20, dummy, dummy, dummy, dummy, dummy, 0, dummy, None) == _lib.M3G_ERR_VALUE


def test_c_abi_ignores_parameters_the_ensemble_does_not_use():
    from torch_m3gnet import _lib

    lib = _lib.load_library()
    p = _params(ensemble=_lib.DYN_NVE, taut=0.0, taup=0.0, compressibility=0.0)
    # valid parameters: the call gets past the checks and fails only on the deliberately too small state buffer
    offs, m, t, seeds = np.array([0, 2], np.int64), np.ones(2), np.array([300.0]), np.zeros(1, np.uint64)
    dummy = C.c_void_p(256)
    assert lib.m3g_dyn_init(C.byref(p), 2, 1, offs.ctypes.data, m.ctypes.data, t.ctypes.data, seeds.ctypes.data, dummy, dummy, 1, None) == _lib.M3G_ERR_SIZE


@pytest.mark.parametrize("case", [dict(offsets=(0, 3, 2, 4), masses=(1,) * 4, temps=(1,) * 3), dict(offsets=(0, 2, 2, 4), masses=(1,) * 4, temps=(1,) * 3),
                                  dict(offsets=(1, 2), masses=(1,) * 2), dict(masses=(1.0, 0.0)), dict(masses=(1.0, -2.0)),
                                  dict(masses=(1.0, float("nan"))), dict(temps=(-1.0,)), dict(temps=(float("nan"),)), dict(temps=(float("inf"),))])
def test_c_abi_refuses_bad_offsets_masses_and_temperatures(case):
    from torch_m3gnet import _lib

    assert _init(_params(), **case) == _lib.M3G_ERR_VALUE


def test_c_abi_refuses_npt_without_stresses_or_lattice():
    from torch_m3gnet import _lib

    lib = _lib.load_library()
    dummy = C.c_void_p(256)
    p = _params()
    assert lib.m3g_dyn_step(C.byref(p), 4, 1, dummy, 1 << 20, dummy, None, dummy, dummy, dummy, 0, None, None) == _lib.M3G_ERR_VALUE
    assert b"stresses" in lib.m3g_last_error()
    assert lib.m3g_dyn_step(C.byref(p), 4, 1, dummy, 1 << 20, dummy, dummy, dummy, None, None, 0, None, None) == _lib.M3G_ERR_VALUE
    size = C.c_size_t()
    assert lib.m3g_dyn_state_bytes(10000, 3, C.byref(size)) == _lib.M3G_OK and size.value > 10000 * 4 * 8
    assert lib.m3g_dyn_state_bytes(2, 3, C.byref(size)) == _lib.M3G_ERR_VALUE


def test_molecular_dynamics_argument_validation():
    from torch_m3gnet.dynamics import MolecularDynamics
    from torch_m3gnet.model.build import build_model

    model = build_model(5.0, 4.0, 3, 3, 95, 16, 1)
    with pytest.raises(TypeError):
        MolecularDynamics(model.model)
    with pytest.raises(TypeError, match="MolecularDynamics"):   # names the driver that was constructed
        MolecularDynamics(model.model)
    for kw in (dict(ensemble="nvt"), dict(ensemble="npt_berendsen"), dict(ensemble="npt_berendsen", compressibility=0.0),
               dict(timestep=0.0), dict(timestep=float("nan")), dict(taut=-1.0), dict(taup=0.0), dict(friction=-0.01),
               dict(pressure=float("inf")), dict(fix_com=True), dict(skin=0.0), dict(temperature=-5.0), dict(temperature=[[300.0]]),
               dict(temperature=float("nan"))):
        with pytest.raises(ValueError):
            MolecularDynamics(model, **kw)
    assert MolecularDynamics(model).fix_com is False and MolecularDynamics(model, ensemble="nve").fix_com is True
    md = MolecularDynamics(model, temperature=[100.0, 200.0])
    pos, lat = fcc(3.6)
    z = np.full(len(pos), 29)
    for kw in (dict(steps=-1), dict(steps=1.5), dict(steps=2, loginterval=0)):
        with pytest.raises(ValueError):
            MolecularDynamics(model).run([lat], [pos], [z], **kw)
    with pytest.raises(ValueError):   # two temperatures, one structure
        md.run([lat], [pos], [z], steps=1)
    with pytest.raises(ValueError):
        MolecularDynamics(model).run([lat], [pos], [z], steps=1, masses=[np.ones(3)])
    with pytest.raises(ValueError):
        MolecularDynamics(model).run([lat], [pos], [z], steps=1, velocities=[np.zeros((3, 3))])
    with pytest.raises(ValueError):
        MolecularDynamics(model, seed=[1, 2]).run([lat], [pos], [z], steps=1)
    z_bad = z.copy()
    z_bad[4] = 96
    with pytest.raises(ValueError):
        MolecularDynamics(model).run([lat], [pos], [z_bad], steps=1)
