"""CPU checks of path-integral MD: the numpy restatement (tests/pimd_reference.py, the yardstick of tests/test_gpu_pimd.py) held to
physics -- the orthogonal normal-mode matrix, the classical limit P = 1, time reversal and second-order drift of the ring-polymer
Hamiltonian on the smooth Lennard-Jones cell of tests/test_nhc_cpu.py, the exact finite-P kinetic and potential energy of harmonic
oscillators under PILE-L with the thermostat's heat accounted for -- and the C ABI / PathIntegralMD refusing bad arguments before
touching a device."""
import ctypes as C
import functools
import re
from pathlib import Path

import numpy as np
import pytest

import md_reference as mr
import pimd_reference as pr
from test_nhc_cpu import SmoothLJ, _start, fcc

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("P", range(1, 65))
def test_mode_matrix_is_orthogonal(P):
    c = pr.mode_matrix(P)
    assert np.abs(c.T @ c - np.eye(P)).max() < 1e-13 and np.abs(c @ c.T - np.eye(P)).max() < 1e-13
    assert np.abs(c[:, 0] - np.sqrt(1.0 / P)).max() == 0.0   # mode 0 is the centroid


def test_single_bead_without_thermostat_is_classical_nve():
    pos, lat, m, v = _start()
    ring = pr.PimdReference(pos[None], m, v[None], 300.0, thermostat="none", dt=2.0)
    nve = mr.DynReference(pos, lat, m, v, "nve", dt=2.0)
    pot_r, pot_c = SmoothLJ(), SmoothLJ()
    for k in range(51):
        ring.step(pot_r(ring.pos[0], lat)[1][None], finish_only=(k == 50))
        nve.step(pot_c(nve.pos, lat)[1], finish_only=(k == 50))
        assert abs(ring.obs[0] - nve.obs[0]) < 1e-12 * nve.obs[0] and ring.obs[2] == 0.0
    assert np.abs(nve.pos - pos).max() > 0.05 and ring.n_steps == nve.n_steps == 50
    assert np.abs(ring.pos[0] - nve.pos).max() < 1e-12 * np.abs(nve.pos).max()
    assert np.abs(ring.v[0] - nve.v).max() < 1e-12 * np.abs(nve.v).max()


def _lj_ring(P, dt, thermostat="none", temperature=300.0, seed=3):
    """A ring on the smooth LJ cell: the beads spread about the start of tests/test_nhc_cpu.py, velocities at P T."""
    from torch_m3gnet.dynamics import maxwell_boltzmann

    pos, lat, m, _ = _start(seed, temperature)
    rng = np.random.default_rng(seed + 100)
    beads = pos[None] + rng.normal(0, 0.01, (P,) + pos.shape)
    vel = np.stack([maxwell_boltzmann(m, P * temperature, seed + 10 * j) for j in range(P)])
    return pr.PimdReference(beads, m, vel, temperature, seed=seed, thermostat=thermostat, dt=dt), lat


def _run_lj(ref, lat, n_steps):
    """n_steps steps (n_steps + 1 calls, the last finish_only): conserved = sum_j E_j + KE + E_spring - heat at every full step."""
    pots, h = [SmoothLJ() for _ in range(ref.P)], []
    for k in range(n_steps + 1):
        e, f = zip(*[pot(x, lat)[:2] for pot, x in zip(pots, ref.pos)])
        ref.step(np.stack(f), finish_only=(k == n_steps))
        h.append(sum(e) + ref.obs[0] + ref.obs[2] - ref.obs[5])
    return np.array(h)


def test_restatement_is_time_reversible():
    ref, lat = _lj_ring(4, 1.0)
    pos0 = ref.pos.copy()
    _run_lj(ref, lat, 100)
    assert np.abs(ref.pos - pos0).max() > 0.05 and ref.n_steps == 100
    ref.reverse()
    _run_lj(ref, lat, 100)
    assert np.abs(ref.pos - pos0).max() < 1e-9


def test_restatement_conserved_quantity_error_is_second_order():
    drift = []
    for dt in (0.5, 1.0, 2.0):
        h = _run_lj(*_lj_ring(4, dt), int(200 / dt))
        drift.append(np.abs(h - h[0]).max())
    print(f"P = 4 without thermostat: drift of H_P over 200 fs at dt = 0.5, 1, 2 fs: {drift}")
    assert drift[0] > 0
    assert 3.0 <= drift[1] / drift[0] <= 5.0 and 3.0 <= drift[2] / drift[1] <= 5.0, drift


# ---- harmonic oscillators: the exact finite-P energies ---------------------------------------------------------------------------
N_OSC, M_H, OMEGA, T_H, DT_H, STEPS_H = 16, 1.008, 0.2, 300.0, 0.25, 20000   # omega dt = 0.05


@functools.lru_cache(maxsize=None)
def _harmonic_run(P):
    """16 independent 3-D oscillators (m = 1.008 amu, omega = 0.2 /fs) at 300 K under PILE-L, 20,000 steps of 0.25 fs, seed 7; the
    centroid friction is omega itself, near critical damping, so that 5,000 fs hold many correlation times.  Returns the obs rows,
    the potential estimator and the conserved quantity of every step."""
    rng = np.random.default_rng(7)
    kt, k = mr.KB * T_H, M_H * OMEGA ** 2 / mr.KAPPA   # spring constant in eV/A^2
    pos = rng.normal(0, np.sqrt(kt / k), (P, N_OSC, 3))
    vel = rng.normal(0, np.sqrt(P * kt * mr.KAPPA / M_H), (P, N_OSC, 3))
    ref = pr.PimdReference(pos, np.full(N_OSC, M_H), vel, T_H, seed=7, thermostat="pile_l", dt=DT_H, centroid_friction=OMEGA)
    rows, pot, conserved = [], [], []
    for s in range(STEPS_H + 1):
        e = 0.5 * k * (ref.pos ** 2).sum()
        ref.step(-k * ref.pos, finish_only=(s == STEPS_H))
        rows.append(ref.obs)
        pot.append(e / P)
        conserved.append(e + ref.obs[0] + ref.obs[2] - ref.obs[5])
    return np.array(rows), np.array(pot), np.array(conserved)


@pytest.mark.parametrize("P", [1, 4, 8])
def test_harmonic_estimators_have_the_exact_finite_p_mean(P):
    """Measured here (seed 7): the nine means lie within 1.0 standard error of the exact value (seeds 8 and 9: 1.14), the largest
    standard error is 0.9 % of it.  At P = 1 both kinetic estimators are the constant 3 n kT / 2, whose standard error is 0: the
    gate adds the rounding of an fp64 mean, 1e-12 of the value."""
    rows, pot, _ = _harmonic_run(P)
    exact = 1.5 * N_OSC * mr.KB * T_H * (OMEGA ** 2 / (OMEGA ** 2 + pr.mode_frequencies(P, T_H) ** 2)).sum()
    cut = len(rows) // 10
    for name, x in (("K_prim", rows[cut:, 3]), ("K_cv", rows[cut:, 4]), ("potential", pot[cut:])):
        blocks = x[:len(x) // 20 * 20].reshape(20, -1).mean(1)
        se = blocks.std(ddof=1) / np.sqrt(20)
        print(f"P = {P}: <{name}> = {x.mean():.5f} +- {se:.5f} against {exact:.5f} ({abs(x.mean() - exact):.1e} off)")
        assert se <= 0.02 * exact, (name, se)
        assert abs(x.mean() - exact) <= 3.0 * se + 1e-12 * exact, (name, x.mean(), exact, se)
    t_mean = rows[cut:, 1].mean()
    assert abs(t_mean / T_H - 1.0) < 0.03, t_mean   # the ring kinetic energy: 3 n P^2 kT / 2


@pytest.mark.parametrize("P", [1, 4, 8])
def test_heat_accounting_keeps_the_conserved_quantity_bounded(P):
    """Measured here: over the 20,000 steps the conserved quantity stays within 1.9e-9 (P = 1), 2.3e-9 (P = 4) and 3.6e-9 eV (P = 8)
    per atom-step of its start -- about 1e-3 of the ring's kinetic energy in all -- while the thermostat's heat spans about that
    kinetic energy (1.3, 12 and 34 eV)."""
    rows, _, conserved = _harmonic_run(P)
    ke_mean = rows[:, 0].mean()
    drift = np.abs(conserved - conserved[0]).max()
    print(f"P = {P}: conserved within {drift:.2e} eV ({drift / (N_OSC * P * STEPS_H):.2e} eV per atom-step); heat spans {np.ptp(rows[:, 5]):.2f} eV, "
          f"mean ring kinetic energy {ke_mean:.2f} eV")
    assert np.ptp(rows[:, 5]) > 100.0 * drift   # the heat is what keeps it there: energy + KE + spring alone moves by its span
    assert drift < 0.02 * ke_mean, (drift, ke_mean)


def test_restatement_flags_non_finite_forces_and_freezes():
    ref, lat = _lj_ring(3, 1.0, thermostat="pile_l")
    f = np.stack([SmoothLJ()(x, lat)[1] for x in ref.pos])
    ref.step(f)
    pos, v, obs = ref.pos.copy(), ref.v.copy(), ref.obs.copy()
    bad = f.copy()
    bad[2, 5, 1] = np.nan
    ref.step(bad)
    ref.step(f)
    assert ref.flags & mr.ERROR and ref.n_steps == 1
    assert np.array_equal(ref.pos, pos) and np.array_equal(ref.v, v) and np.array_equal(ref.obs, obs)


# ---- argument checks (no device needed: refused before any HIP call) ------------------------------------------------------------
def _params(**kw):
    from torch_m3gnet import _lib

    p = dict(thermostat=_lib.PIMD_PILE_L, n_beads=2, dt=0.5, centroid_friction=0.01, pile_lambda=0.5)
    p.update(kw)
    return _lib.M3GPimdParams(**p)


def _init(params, offsets=(0, 2, 4), masses=(1.0, 2.0, 1.0, 2.0), temps=(300.0,), state_bytes=1 << 20):
    from torch_m3gnet import _lib

    lib = _lib.load_library()
    offs = np.array(offsets, dtype=np.int64)
    m = np.array(masses, dtype=np.float64)
    t = np.array(temps, dtype=np.float64)
    seeds = np.zeros(len(t), dtype=np.uint64)
    dummy = C.c_void_p(256)   # never dereferenced: the call returns at the checks
    return lib.m3g_pimd_init(C.byref(params), int(offs[-1]), len(offs) - 1, offs.ctypes.data, m.ctypes.data, t.ctypes.data,
                             seeds.ctypes.data, dummy, dummy, state_bytes, None)


@pytest.mark.parametrize("bad,why", [(dict(thermostat=2), "thermostat"), (dict(thermostat=-1), "thermostat"), (dict(n_beads=0), "n_beads"),
                                     (dict(n_beads=65), "n_beads"), (dict(dt=0.0), "dt"), (dict(dt=float("nan")), "dt"),
                                     (dict(dt=float("inf")), "dt"), (dict(centroid_friction=-0.1), "centroid_friction"),
                                     (dict(centroid_friction=float("nan")), "centroid_friction"), (dict(pile_lambda=-1.0), "pile_lambda"),
                                     (dict(pile_lambda=float("inf")), "pile_lambda")])
def test_c_abi_refuses_invalid_pimd_parameters(bad, why):
    from torch_m3gnet import _lib

    lib = _lib.load_library()
    assert _init(_params(**bad)) == _lib.M3G_ERR_VALUE
    assert why.encode() in lib.m3g_last_error()
    dummy = C.c_void_p(256)
    assert lib.m3g_pimd_step(C.byref(_params(**bad)), 4, 2, dummy, 1 << 20, dummy, dummy, 0, dummy, None) == _lib.M3G_ERR_VALUE
    assert why.encode() in lib.m3g_last_error()


def test_c_abi_refuses_bad_rings_temperatures_masses_sizes_and_missing_arrays():
    from torch_m3gnet import _lib

    lib = _lib.load_library()
    assert _init(_params(n_beads=3)) == _lib.M3G_ERR_VALUE and b"multiple of n_beads" in lib.m3g_last_error()
    assert _init(_params(), offsets=(0, 1, 4)) == _lib.M3G_ERR_VALUE and b"atom count" in lib.m3g_last_error()
    assert _init(_params(), masses=(1.0, 2.0, 1.0, 3.0)) == _lib.M3G_ERR_VALUE and b"masses" in lib.m3g_last_error()
    assert _init(_params(), temps=(0.0,)) == _lib.M3G_ERR_VALUE and b"temperature" in lib.m3g_last_error()
    assert _init(_params(), temps=(float("nan"),)) == _lib.M3G_ERR_VALUE and b"temperature" in lib.m3g_last_error()
    assert _init(_params(), masses=(1.0, 0.0, 1.0, 0.0)) == _lib.M3G_ERR_VALUE and b"mass" in lib.m3g_last_error()
    assert _init(_params(), offsets=(0, 2, 2), masses=(1.0, 2.0)) == _lib.M3G_ERR_VALUE and b"offsets" in lib.m3g_last_error()
    assert _init(_params(), state_bytes=1) == _lib.M3G_ERR_SIZE and b"too small" in lib.m3g_last_error()   # valid: past the checks
    dummy = C.c_void_p(256)
    assert lib.m3g_pimd_step(C.byref(_params()), 4, 2, dummy, 1 << 20, None, dummy, 0, None, None) == _lib.M3G_ERR_VALUE
    assert b"forces" in lib.m3g_last_error()
    assert lib.m3g_pimd_step(C.byref(_params()), 4, 2, dummy, 1 << 20, dummy, None, 0, None, None) == _lib.M3G_ERR_VALUE
    assert b"pos" in lib.m3g_last_error()
    assert lib.m3g_pimd_step(C.byref(_params()), 4, 2, dummy, 1, dummy, dummy, 0, None, None) == _lib.M3G_ERR_SIZE
    assert lib.m3g_pimd_step(C.byref(_params()), 6, 3, dummy, 1 << 20, dummy, dummy, 0, None, None) == _lib.M3G_ERR_VALUE   # 3 structures, P = 2
    size, small = C.c_size_t(), C.c_size_t()
    assert lib.m3g_pimd_state_bytes(64000, 64, 64, C.byref(size)) == _lib.M3G_OK and size.value > 64000 * 4 * 8 + 64 * 64 * 8
    assert lib.m3g_pimd_state_bytes(64000, 64, 1, C.byref(small)) == _lib.M3G_OK and small.value > 64000 * 4 * 8
    for n, s, p in ((2, 3, 1), (0, 1, 1), (4, 0, 1), (4, 2, 0), (130, 65, 65), (6, 3, 2), (5, 2, 2)):
        assert lib.m3g_pimd_state_bytes(n, s, p, C.byref(size)) == _lib.M3G_ERR_VALUE, (n, s, p)
    mass_at, vel_at = C.c_size_t(), C.c_size_t()
    assert lib.m3g_pimd_state_view(100, 4, 2, C.byref(mass_at), C.byref(vel_at)) == _lib.M3G_OK and 0 < mass_at.value < vel_at.value
    assert lib.m3g_pimd_state_view(100, 4, 3, C.byref(mass_at), C.byref(vel_at)) == _lib.M3G_ERR_VALUE
    assert lib.m3g_pimd_read(4, 2, 2, dummy, 1, None, None, None, None, None) == _lib.M3G_ERR_SIZE
    assert lib.m3g_pimd_read(4, 2, 3, dummy, 1 << 20, None, None, None, None, None) == _lib.M3G_ERR_VALUE


def test_path_integral_md_refuses_bad_arguments():
    import torch

    from torch_m3gnet.model.build import build_model
    from torch_m3gnet.path_integral import PathIntegralMD, PimdState

    model = build_model(5.0, 4.0, 3, 3, 95, 16, 1)
    for kw, why in ((dict(n_beads=0), "n_beads"), (dict(n_beads=65), "n_beads"), (dict(n_beads=2.5), "n_beads"), (dict(n_beads=True), "n_beads"),
                    (dict(thermostat="langevin"), "thermostat"), (dict(thermostat=1), "thermostat"), (dict(timestep=0.0), "timestep"),
                    (dict(timestep=float("nan")), "timestep"), (dict(centroid_friction=-1.0), "centroid_friction"),
                    (dict(pile_lambda=float("inf")), "pile_lambda"), (dict(temperature=0.0), "temperature"),
                    (dict(temperature=[300.0, float("nan")]), "temperature"), (dict(ring_batches=1), "ring_batches"), (dict(skin=0.0), "skin")):
        with pytest.raises(ValueError, match=why):
            PathIntegralMD(model, **dict(dict(n_beads=4), **kw))
    with pytest.raises(TypeError, match="Gradient"):
        PathIntegralMD(model.model, 4)
    md = PathIntegralMD(model, 4)
    assert md.thermostat == "pile_l" and md.pile_lambda == 0.5 and md.centroid_friction == 0.01 and md.timestep == 0.5 and md.ring_batches
    pos, lat = fcc(3.6)
    z = np.full(len(pos), 29)
    with pytest.raises(ValueError, match="n_beads = 4"):   # a ring of another bead count
        md.run([lat], [np.stack([pos] * 3)], [z], steps=1)
    with pytest.raises(ValueError, match="positions"):
        md.run([lat], [pos[:5]], [z], steps=1)
    with pytest.raises(ValueError, match="steps"):
        md.run([lat], [pos], [z], steps=-1)
    with pytest.raises(ValueError, match="temperature"):
        PathIntegralMD(model, 4, temperature=[300.0, 200.0]).run([lat], [pos], [z], steps=1)
    with pytest.raises(ValueError, match="masses"):
        md.run([lat], [pos], [z], steps=1, masses=[np.zeros(len(pos))])
    x, v = torch.zeros(4, 3, dtype=torch.float64), torch.zeros(4, 3, dtype=torch.float64)
    with pytest.raises(ValueError, match="multiple of n_beads"):
        PimdState(x, [0, 2, 4], np.ones(4), v, [300.0], [0], n_beads=3)
    with pytest.raises(ValueError, match="thermostat"):
        PimdState(x, [0, 2, 4], np.ones(4), v, [300.0], [0], n_beads=2, thermostat="nve")
    with pytest.raises(ValueError, match="seeds"):
        PimdState(x, [0, 2, 4], np.ones(4), v, [300.0], [0, 1], n_beads=2)


def test_new_symbols_are_declared_bound_and_exported():
    from torch_m3gnet import _lib, dynamics, path_integral

    header = (ROOT / "include" / "m3gnet_hip.h").read_text()
    lib = _lib.load_library()
    for name in ("m3g_pimd_state_bytes", "m3g_pimd_state_view", "m3g_pimd_init", "m3g_pimd_step", "m3g_pimd_read"):
        assert re.search(rf"\bint {name}\(", header) and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert "m3g_pimd_params" in header and C.sizeof(_lib.M3GPimdParams) == 2 * 4 + 3 * 8
    for name, value in (("M3G_PIMD_NONE", _lib.PIMD_NONE), ("M3G_PIMD_PILE_L", _lib.PIMD_PILE_L), ("M3G_PIMD_MAX_BEADS", _lib.PIMD_MAX_BEADS),
                        ("M3G_PIMD_OBS", _lib.PIMD_OBS)):
        assert re.search(rf"#define {name} {value}\b", header), name
    info = _lib.M3GInfo()
    assert lib.m3g_get_info(C.byref(info)) == 0 and info.abi_version == 11 == _lib.ABI_VERSION
    assert set(dynamics.ENSEMBLES) == {"nve", "nvt_berendsen", "nvt_langevin", "npt_berendsen"}
    assert set(dynamics.NHC_ENSEMBLES) == {"nvt_nose_hoover", "npt_mtk"}
    assert set(path_integral.THERMOSTATS) == {"none", "pile_l"} and path_integral.HBAR == pr.HBAR
    assert hasattr(path_integral, "PimdState") and hasattr(path_integral, "pimd_step") and hasattr(path_integral, "PathIntegralMD")
