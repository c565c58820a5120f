"""CPU checks of thermodynamic integration to an Einstein crystal: the numpy restatement (tests/ti_reference.py, the yardstick of
tests/test_gpu_ti.py) held to physics -- the centre of mass stays where it was, friction 0 at lambda = 1 is classical NVE, time
reversal, the exact free-energy difference of two Einstein crystals with the centre of mass held (3 (N - 1) / 2 kT ln(k_B / k_A), not
3 N / 2) by switching and the exact equilibrium mean of dH/dlambda --, the closed forms of `einstein_free_energy`, and the C ABI /
FreeEnergy / TiState refusing bad arguments before touching a device."""
import ctypes as C
import functools
import re
from pathlib import Path

import numpy as np
import pytest

import md_reference as mr
import ti_reference as tr
from test_nhc_cpu import SmoothLJ, _start, fcc

ROOT = Path(__file__).resolve().parent.parent


# ---- two Einstein crystals about the same sites: the "model" is the stiffer one -----------------------------------------------------
N_H, K_A, K_B, T_H = 8, 2.0, 6.0, 300.0
DOF = 3 * (N_H - 1)


def _harmonic(seed, friction=0.05, schedule="smooth"):
    """8 atoms of 20 .. 60 amu on random sites, started on them with Maxwell-Boltzmann velocities of zero total momentum."""
    from torch_m3gnet.dynamics import maxwell_boltzmann

    rng = np.random.default_rng(1000 + seed)
    m = rng.uniform(20.0, 60.0, N_H)
    sites = rng.uniform(0.0, 6.0, (N_H, 3))
    return tr.TiReference(sites, m, np.full(N_H, K_A), maxwell_boltzmann(m, T_H, seed), sites, T_H, seed=seed, schedule=schedule, dt=1.0,
                          friction=friction)


def _run_harmonic(ref, n_steps, rows=None):
    """n_steps steps (n_steps + 1 calls, the last finish_only) under the model E = 1/2 k_B sum |u|^2."""
    for k in range(n_steps + 1):
        u = ref.pos - ref.r0
        ref.step(-K_B * u, 0.5 * K_B * (u * u).sum(), finish_only=(k == n_steps))
        if rows is not None:
            rows.append(ref.obs)


def test_centre_of_mass_is_held():
    """Measured here: 3.7e-15 A after 2,000 thermostatted steps (the rounding of sum m x, not a drift)."""
    ref = _harmonic(0)
    ref.path(0.3, 0.3, 0)
    _run_harmonic(ref, 2000)
    off = np.abs((ref.m[:, None] * (ref.pos - ref.r0)).sum(0)).max() / ref.m.sum()
    p = np.abs((ref.m[:, None] * ref.v).sum(0)).max() / ref.m.sum()
    print(f"after 2,000 steps at 300 K: centre of mass {off:.1e} A from its start, its velocity {p:.1e} A/fs")
    assert np.abs(ref.pos - ref.r0).max() > 0.05 and ref.n_steps == 2000
    assert off < 1e-10 and p < 1e-12


def test_without_friction_at_lambda_one_is_classical_nve():
    pos, lat, m, v = _start()
    ti = tr.TiReference(pos, m, np.full(len(m), 3.0), v, pos, 300.0, dt=2.0, friction=0.0)
    nve = mr.DynReference(pos, lat, m, v, "nve", dt=2.0)
    pot_t, pot_c = SmoothLJ(), SmoothLJ()
    for k in range(51):
        e, f = pot_t(ti.pos, lat)[:2]
        ti.step(f, e, finish_only=(k == 50))
        nve.step(pot_c(nve.pos, lat)[1], finish_only=(k == 50))
        assert abs(ti.obs[0] - nve.obs[0]) < 1e-12 * nve.obs[0] and ti.obs[4] == 1.0
    assert np.abs(nve.pos - pos).max() > 0.05 and ti.n_steps == nve.n_steps == 50
    assert np.abs(ti.pos - nve.pos).max() < 1e-12 * np.abs(nve.pos).max()
    assert np.abs(ti.v - nve.v).max() < 1e-12 * np.abs(nve.v).max()


def test_restatement_is_time_reversible():
    pos, lat, m, v = _start()
    sites = fcc(3.61)[0]
    ref = tr.TiReference(pos, m, np.full(len(m), 2.0), v, sites, 300.0, dt=1.0, friction=0.0)
    ref.path(0.4, 0.4, 0)

    def run(n):
        pot = SmoothLJ()
        for k in range(n + 1):
            e, f = pot(ref.pos, lat)[:2]
            ref.step(f, e, finish_only=(k == n))

    run(100)
    assert np.abs(ref.pos - pos).max() > 0.05 and ref.n_steps == 100
    ref.reverse()
    run(100)
    assert np.abs(ref.pos - pos).max() < 1e-9


@functools.lru_cache(maxsize=None)
def _switch(seed):
    """2,000 steps at lambda = 1, 4,000 steps to 0, 2,000 steps there, 4,000 steps back: (W10, W01)."""
    ref, work = _harmonic(seed), []
    for lb, le, n in ((1.0, 1.0, 2000), (1.0, 0.0, 4000), (0.0, 0.0, 2000), (0.0, 1.0, 4000)):
        ref.path(lb, le, n if lb != le else 0)
        _run_harmonic(ref, n)
        if lb != le:
            work.append(ref.work)
    return tuple(work)


def test_switching_between_two_einstein_crystals_gives_the_exact_free_energy_difference():
    """Measured here (seeds 0 .. 5): delta_f = 0.3009 +- 0.0043 eV against 3 (N - 1) / 2 kT ln 3 = 0.2982 eV (0.6 standard errors off; the
    standard error is 1.4 % of it) and 9.4 standard errors from the 3 N / 2 value 0.3408 eV of a free centre of mass; the dissipation
    0.0050 eV per switch."""
    kt = mr.KB * T_H
    exact, free_com = 0.5 * DOF * kt * np.log(K_B / K_A), 1.5 * N_H * kt * np.log(K_B / K_A)
    w10, w01 = np.array([_switch(seed) for seed in range(6)]).T
    df = 0.5 * (w01 - w10)
    mean, se = df.mean(), df.std(ddof=1) / np.sqrt(len(df))
    print(f"delta_f = {mean:.4f} +- {se:.4f} eV against {exact:.4f} eV ({abs(mean - exact) / se:.1f} standard errors off); the 3 N / 2 value "
          f"{free_com:.4f} eV is {abs(mean - free_com) / se:.1f} standard errors away; dissipation {0.5 * (w01 + w10).mean():.4f} eV")
    assert se <= 0.02 * exact, se
    assert abs(mean - exact) <= 3.0 * se, (mean, exact, se)
    assert abs(mean - free_com) > 3.0 * se, (mean, free_com, se)
    assert (w10 < 0).all() and (w01 > 0).all() and 0.5 * (w01 + w10).mean() > 0   # the second law, on average


EQ_STEPS, EQ_DISCARD = 40000, 2000


@pytest.mark.parametrize("lam", [0.1, 0.5, 0.9])
def test_equilibrium_mean_of_dh_dlambda_is_exact(lam):
    """<D> = 3 (N - 1) / 2 kT (k_B - k_A) / (lambda k_B + (1 - lambda) k_A): 40,000 steps of 1 fs at friction 0.05 /fs, the first 2,000
    discarded, 20 block means of the rest.  Measured here (seed 3): lambda = 0.1: 0.4486 +- 0.0082 eV against 0.4524; 0.5: 0.2682 +- 0.0041
    against 0.2714; 0.9: 0.1915 +- 0.0025 against 0.1939 -- within 0.9 standard errors, which are at most 1.8 % of the exact value.  The
    device's Welford mean is that of the same samples."""
    ref, rows = _harmonic(3), []
    ref.path(lam, lam, 0, EQ_DISCARD)
    _run_harmonic(ref, EQ_STEPS, rows)
    d = np.array(rows)[EQ_DISCARD:, 3]
    exact = 0.5 * DOF * mr.KB * T_H * (K_B - K_A) / (lam * K_B + (1.0 - lam) * K_A)
    blocks = d[:len(d) // 20 * 20].reshape(20, -1).mean(1)
    se = blocks.std(ddof=1) / np.sqrt(20)
    print(f"lambda = {lam}: <dH/dlambda> = {d.mean():.4f} +- {se:.4f} eV against {exact:.4f} eV ({abs(d.mean() - exact) / se:.1f} standard errors off, "
          f"the standard error {100 * se / exact:.1f} % of it)")
    assert ref.count == len(d) == EQ_STEPS + 1 - EQ_DISCARD
    assert abs(ref.mean - d.mean()) < 1e-12 * abs(exact) and abs(ref.variance - d.var(ddof=1)) < 1e-10 * d.var()
    assert se <= 0.02 * exact, se
    assert abs(d.mean() - exact) <= 3.0 * se, (d.mean(), exact, se)
    t_mean = np.array(rows)[EQ_DISCARD:, 1].mean()
    assert abs(t_mean / T_H - 1.0) < 0.03, t_mean   # 3 n - 3 degrees of freedom


def test_work_is_the_trapezoid_sum_and_schedules_end_where_they_should():
    for schedule in ("linear", "smooth"):
        ref, rows = _harmonic(1, schedule=schedule), []
        ref.path(0.2, 0.9, 50, 10)
        _run_harmonic(ref, 60, rows)
        rows = np.array(rows)
        lam, d = rows[:, 4], rows[:, 3]
        assert lam[0] == 0.2 and np.all(np.abs(lam[50:] - 0.9) < 1e-15) and np.all(np.diff(lam[:51]) > 0)
        assert abs(ref.work - (np.diff(lam) * 0.5 * (d[1:] + d[:-1])).sum()) < 1e-13 and ref.count == 51 and ref.c == 60
        if schedule == "linear":
            assert np.abs(lam[:51] - (0.2 + 0.7 * np.arange(51) / 50)).max() < 1e-15
        else:
            assert abs(lam[25] - 0.55) < 1e-15 and lam[1] - 0.2 < 1e-6   # g(1/2) = 1/2; flat ends
        assert abs(ref.msd_sum.sum() - ((rows[10:, 2] * 2 / K_A).sum())) < 1e-12 * ref.msd_sum.sum()


def test_restatement_flags_non_finite_forces_and_energies_and_freezes():
    for bad_energy in (False, True):
        ref = _harmonic(2)
        _run_harmonic(ref, 3)
        u = ref.pos - ref.r0
        f = -K_B * u
        ref.step(f, 1.0)
        kept = (ref.pos.copy(), ref.v.copy(), ref.obs.copy(), ref.work, ref.count)
        bad = f.copy()
        bad[5, 1] = np.nan
        ref.step(f if bad_energy else bad, np.inf if bad_energy else 1.0)
        ref.step(f, 1.0)
        ref.path(0.0, 1.0, 10)
        assert ref.flags & mr.ERROR and ref.n_steps == 4
        assert np.array_equal(ref.pos, kept[0]) and np.array_equal(ref.v, kept[1]) and np.array_equal(ref.obs, kept[2])
        assert ref.work == kept[3] and ref.count == kept[4] and ref.lam_b == 1.0


def test_einstein_free_energy_closed_forms():
    from torch_m3gnet.free_energy import einstein_free_energy
    from torch_m3gnet.path_integral import HBAR

    n, m, k, t, vol = 32, 63.546, 3.5, 450.0, 380.0
    kt = mr.KB * t
    out = einstein_free_energy(np.full(n, m), k, t, vol)
    omega = np.sqrt(mr.KAPPA * k / m)
    assert abs(out["f_einstein"] - 3 * n * kt * np.log(HBAR * omega / kt)) < 1e-12 * abs(out["f_einstein"])
    freitas = kt * np.log((n / vol) * (2 * np.pi * kt / (n * k)) ** 1.5)   # eq. 24 of Freitas, Asta, de Koning (2016)
    assert abs(out["f_com"] - freitas) < 1e-12 * abs(freitas)
    # per-atom arrays and another count of primitive cells
    ms, ks = np.linspace(20, 60, n), np.linspace(1, 5, n)
    two = einstein_free_energy(ms, ks, t, vol, n_cells=8)
    s2 = kt * ((ms / ms.sum()) ** 2 / ks).sum()
    assert abs(two["f_com"] - (1.5 * kt * np.log(2 * np.pi * s2) + kt * np.log(8 / vol))) < 1e-12
    assert abs(two["f_einstein"] + 3 * kt * np.log(kt / (HBAR * np.sqrt(mr.KAPPA * ks / ms))).sum()) < 1e-12
    for kw, why in ((dict(temperature=0.0), "temperature"), (dict(volume=-1.0), "volume"), (dict(spring_constants=0.0), "spring_constants"),
                    (dict(masses=[1.0, -1.0]), "masses"), (dict(n_cells=0), "n_cells")):
        with pytest.raises(ValueError, match=why):
            einstein_free_energy(**dict(dict(masses=[1.0, 2.0], spring_constants=1.0, temperature=300.0, volume=10.0), **kw))


# ---- argument checks (no device needed: refused before any HIP call) ------------------------------------------------------------
def _params(**kw):
    from torch_m3gnet import _lib

    p = dict(schedule=_lib.TI_SMOOTH, reserved=0, dt=1.0, friction=0.01)
    p.update(kw)
    return _lib.M3GTiParams(**p)


def _init(params, offsets=(0, 2, 4), masses=(1.0, 2.0, 1.0, 2.0), springs=(1.0, 0.0, 2.0, 2.0), temps=(300.0, 300.0), state_bytes=1 << 20):
    from torch_m3gnet import _lib

    lib = _lib.load_library()
    offs = np.array(offsets, dtype=np.int64)
    m, k, t = (np.array(x, dtype=np.float64) for x in (masses, springs, temps))
    seeds = np.zeros(len(t), dtype=np.uint64)
    dummy = C.c_void_p(256)   # never dereferenced: the call returns at the checks
    return lib.m3g_ti_init(C.byref(params), int(offs[-1]), len(offs) - 1, offs.ctypes.data, m.ctypes.data, k.ctypes.data, t.ctypes.data,
                           seeds.ctypes.data, dummy, dummy, dummy, state_bytes, None)


@pytest.mark.parametrize("bad,why", [(dict(schedule=2), "schedule"), (dict(schedule=-1), "schedule"), (dict(dt=0.0), "dt"),
                                     (dict(dt=float("nan")), "dt"), (dict(dt=float("inf")), "dt"), (dict(friction=-0.1), "friction"),
                                     (dict(friction=float("nan")), "friction")])
def test_c_abi_refuses_invalid_ti_parameters(bad, why):
    from torch_m3gnet import _lib

    lib = _lib.load_library()
    assert _init(_params(**bad)) == _lib.M3G_ERR_VALUE
    assert why.encode() in lib.m3g_last_error()
    dummy = C.c_void_p(256)
    assert lib.m3g_ti_step(C.byref(_params(**bad)), 4, 2, dummy, 1 << 20, dummy, dummy, dummy, 0, dummy, None) == _lib.M3G_ERR_VALUE
    assert why.encode() in lib.m3g_last_error()


def test_c_abi_refuses_bad_temperatures_masses_springs_sizes_paths_and_missing_arrays():
    from torch_m3gnet import _lib

    lib = _lib.load_library()
    for kw, why in ((dict(temps=(300.0, 0.0)), b"temperature"), (dict(temps=(float("nan"), 300.0)), b"temperature"),
                    (dict(masses=(1.0, 0.0, 1.0, 2.0)), b"mass"), (dict(springs=(1.0, -1.0, 1.0, 1.0)), b"spring"),
                    (dict(springs=(1.0, float("inf"), 1.0, 1.0)), b"spring"), (dict(springs=(1.0, 1.0, 0.0, 0.0)), b"spring"),
                    (dict(offsets=(0, 2, 2), masses=(1.0, 2.0), springs=(1.0, 1.0)), b"offsets"),
                    (dict(offsets=(0, 1, 4)), b"at least two atoms"), (dict(offsets=(0, 3, 4)), b"at least two atoms")):
        assert _init(_params(), **kw) == _lib.M3G_ERR_VALUE and why in lib.m3g_last_error(), (kw, lib.m3g_last_error())
    assert _init(_params(), state_bytes=1) == _lib.M3G_ERR_SIZE and b"too small" in lib.m3g_last_error()   # valid: past the checks
    dummy = C.c_void_p(256)
    step = lambda *a: lib.m3g_ti_step(C.byref(_params()), *a)   # noqa: E731
    assert step(4, 2, dummy, 1 << 20, None, dummy, dummy, 0, None, None) == _lib.M3G_ERR_VALUE and b"forces" in lib.m3g_last_error()
    assert step(4, 2, dummy, 1 << 20, dummy, None, dummy, 0, None, None) == _lib.M3G_ERR_VALUE and b"energies" in lib.m3g_last_error()
    assert step(4, 2, dummy, 1 << 20, dummy, dummy, None, 0, None, None) == _lib.M3G_ERR_VALUE and b"pos" in lib.m3g_last_error()
    assert step(4, 2, dummy, 1, dummy, dummy, dummy, 0, None, None) == _lib.M3G_ERR_SIZE
    assert step(3, 2, dummy, 1 << 20, dummy, dummy, dummy, 0, None, None) == _lib.M3G_ERR_VALUE   # a structure of one atom
    size = C.c_size_t()
    assert lib.m3g_ti_state_bytes(10000, 4, C.byref(size)) == _lib.M3G_OK and size.value > 10000 * 9 * 8
    for n, s in ((1, 1), (3, 2), (0, 1), (4, 0)):
        assert lib.m3g_ti_state_bytes(n, s, C.byref(size)) == _lib.M3G_ERR_VALUE, (n, s)
    mass_at, vel_at = C.c_size_t(), C.c_size_t()
    assert lib.m3g_ti_state_view(100, 4, C.byref(mass_at), C.byref(vel_at)) == _lib.M3G_OK and 0 < mass_at.value < vel_at.value
    assert lib.m3g_ti_state_view(7, 4, C.byref(mass_at), C.byref(vel_at)) == _lib.M3G_ERR_VALUE
    lam = lambda *x: np.array(x, dtype=np.float64)   # noqa: E731
    ok, high, low, nan = lam(0.0, 1.0), lam(0.5, 1.5), lam(-0.1, 0.5), lam(0.5, float("nan"))
    for lb, le, n_switch, n_discard in ((high, ok, 10, 0), (ok, low, 10, 0), (nan, ok, 10, 0), (ok, ok, -1, 0), (ok, ok, 10, -1)):
        assert lib.m3g_ti_path(4, 2, dummy, 1 << 20, lb.ctypes.data, le.ctypes.data, n_switch, n_discard, None) == _lib.M3G_ERR_VALUE
        assert b"lambda" in lib.m3g_last_error() or b"n_switch" in lib.m3g_last_error()
    assert lib.m3g_ti_path(4, 2, dummy, 1, ok.ctypes.data, ok.ctypes.data, 10, 0, None) == _lib.M3G_ERR_SIZE
    assert lib.m3g_ti_path(4, 2, dummy, 1 << 20, None, ok.ctypes.data, 10, 0, None) == _lib.M3G_ERR_VALUE
    assert lib.m3g_ti_read(4, 2, dummy, 1, None, None, None, None, None, None, None, None, None) == _lib.M3G_ERR_SIZE
    assert lib.m3g_ti_read(3, 2, dummy, 1 << 20, None, None, None, None, None, None, None, None, None) == _lib.M3G_ERR_VALUE


def test_free_energy_driver_refuses_bad_arguments():
    import torch

    from torch_m3gnet.free_energy import FreeEnergy, TiState, ti_path
    from torch_m3gnet.model.build import build_model

    model = build_model(5.0, 4.0, 3, 3, 95, 16, 1)
    for kw, why in ((dict(temperature=0.0), "temperature"), (dict(temperature=float("nan")), "temperature"), (dict(spring_constant=0.0), "spring_constant"),
                    (dict(spring_constant=-2.0), "spring_constant"), (dict(spring_constant="auto"), "spring_constant"),
                    (dict(spring_constant={29: 0.0}), "spring_constant"), (dict(spring_constant={}), "spring_constant"),
                    (dict(timestep=0.0), "timestep"), (dict(friction=-1.0), "friction"), (dict(friction=float("inf")), "friction"),
                    (dict(schedule="cubic"), "schedule"), (dict(schedule=1), "schedule"), (dict(replicas=0), "replicas"),
                    (dict(replicas=2.5), "replicas"), (dict(structure_batches=1), "structure_batches"), (dict(skin=0.0), "skin"),
                    (dict(msd_steps=1), "msd_steps")):
        with pytest.raises(ValueError, match=why):
            FreeEnergy(model, **dict(dict(temperature=300.0, spring_constant=2.0), **kw))
    with pytest.raises(TypeError, match="Gradient"):
        FreeEnergy(model.model, 300.0, 2.0)
    fe = FreeEnergy(model, 300.0, 2.0)
    assert fe.schedule == "smooth" and fe.friction == 0.01 and fe.timestep == 1.0 and fe.replicas == 4 and fe.structure_batches
    pos, lat = fcc(3.6)
    z = np.full(len(pos), 29)
    with pytest.raises(ValueError, match="positions"):
        fe.switch([lat], [pos[:5]], [z], 10, 10)
    with pytest.raises(ValueError, match="at least two atoms"):
        fe.switch([lat], [pos[:1]], [z[:1]], 10, 10)
    with pytest.raises(ValueError, match="equilibration"):
        fe.switch([lat], [pos], [z], -1, 10)
    with pytest.raises(ValueError, match="switch_steps"):
        fe.switch([lat], [pos], [z], 10, 0)
    with pytest.raises(ValueError, match="loginterval"):
        fe.switch([lat], [pos], [z], 10, 10, loginterval=0)
    with pytest.raises(ValueError, match="masses"):
        fe.switch([lat], [pos], [z], 10, 10, masses=[np.zeros(len(pos))])
    with pytest.raises(ValueError, match="n_cells"):
        fe.switch([lat], [pos], [z], 10, 10, n_cells=0)
    with pytest.raises(ValueError, match="n_lambda"):
        fe.integrate([lat], [pos], [z], 10, 10, n_lambda=0)
    with pytest.raises(ValueError, match="steps"):
        fe.integrate([lat], [pos], [z], 10, 0)
    with pytest.raises(ValueError, match="species"):
        FreeEnergy(model, 300.0, {13: 2.0}).switch([lat], [pos], [z], 10, 10)
    with pytest.raises(ValueError, match="spring_constant"):
        FreeEnergy(model, 300.0, [np.full(3, 2.0)]).switch([lat], [pos], [z], 10, 10)
    x, v = torch.zeros(4, 3, dtype=torch.float64), torch.zeros(4, 3, dtype=torch.float64)
    with pytest.raises(ValueError, match="schedule"):
        TiState(x, [0, 2, 4], np.ones(4), np.ones(4), v, x, [300.0, 300.0], [0, 1], schedule="quintic")
    with pytest.raises(ValueError, match="seeds"):
        TiState(x, [0, 2, 4], np.ones(4), np.ones(4), v, x, [300.0, 300.0], [0])
    with pytest.raises(ValueError, match="springs"):
        TiState(x, [0, 2, 4], np.ones(4), np.ones(3), v, x, 300.0, [0, 1])
    with pytest.raises(ValueError, match="reference"):
        TiState(x, [0, 2, 4], np.ones(4), np.ones(4), v, x[:3], 300.0, [0, 1])
    assert ti_path.__doc__ and "n_discard" in ti_path.__doc__


def test_new_symbols_are_declared_bound_and_exported():
    from torch_m3gnet import _lib, dynamics, free_energy, path_integral

    header = (ROOT / "include" / "m3gnet_hip.h").read_text()
    lib = _lib.load_library()
    for name in ("m3g_ti_state_bytes", "m3g_ti_state_view", "m3g_ti_init", "m3g_ti_path", "m3g_ti_step", "m3g_ti_read"):
        assert re.search(rf"\bint {name}\(", header) and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert "m3g_ti_params" in header and C.sizeof(_lib.M3GTiParams) == 24
    for name, value in (("M3G_TI_LINEAR", _lib.TI_LINEAR), ("M3G_TI_SMOOTH", _lib.TI_SMOOTH), ("M3G_TI_OBS", _lib.TI_OBS)):
        assert re.search(rf"#define {name} {value}\b", header), name
    info = _lib.M3GInfo()
    assert lib.m3g_get_info(C.byref(info)) == 0 and info.abi_version == 11 == _lib.ABI_VERSION
    assert set(dynamics.ENSEMBLES) == {"nve", "nvt_berendsen", "nvt_langevin", "npt_berendsen"}
    assert set(path_integral.THERMOSTATS) == {"none", "pile_l"} and free_energy.HBAR is path_integral.HBAR
    assert set(free_energy.SCHEDULES) == {"linear", "smooth"} and set(tr.SCHEDULES) == set(free_energy.SCHEDULES)
    assert all(hasattr(free_energy, name) for name in ("TiState", "ti_path", "ti_step", "einstein_free_energy", "FreeEnergy", "state_tensor"))
