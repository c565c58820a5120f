"""NormalModeAnalysis (torch_m3gnet.normal_modes) on the MI355X under the LJ-fitted model: fcc Cu, conventional cell at the model's
lattice constant, phonons on (3, 3, 3) as in tests/test_gpu_phonon_modes.py, MD supercell (2, 2, 2): 32 atoms, 8 q, 96 modes, 20 K,
dt = 2 fs.  Production runs are Langevin: under this fixture model a long NVE run drifts (tests/test_gpu_rnemd_driver.py), so "nve"
is covered by 300 steps.  Every measured figure goes to profiles/normal_modes.txt through helpers.record_line."""
import numpy as np
import pytest

from helpers import GOLDEN, record_line

pytestmark = pytest.mark.gpu
DEV = "cuda"
RECORD = "normal_modes.txt"
FCC_BASE = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])
A0, T, DT = 3.5025, 20.0, 2.0
KB, KAPPA = 8.617333262e-5, 9.648533215665e-3
SHAPE = (8, 12)


@pytest.fixture(scope="module")
def cu():
    from torch_m3gnet.model.build import build_model_from_npz
    from torch_m3gnet.phonons import Phonons

    model = build_model_from_npz(GOLDEN / "model_fitted_lj.npz").to(DEV)
    (res,) = Phonons(model).run([np.eye(3) * A0], [FCC_BASE * A0], [np.full(4, 29)], (3, 3, 3))
    return model, res


def _run(cu, production, friction, steps, equilibration, n_lags, timestep=DT):
    from torch_m3gnet.normal_modes import NormalModeAnalysis

    model, ph = cu
    nma = NormalModeAnalysis(model, temperature=T, timestep=timestep, friction=friction, production=production, n_lags=n_lags,
                             sample_interval=5, seed=11)
    (res,) = nma.run([ph], (2, 2, 2), steps, equilibration=equilibration, loginterval=5)
    assert res["error"] is False and res["nonfinite"] is False and res["n_steps"] == steps
    assert res["n_samples"] == steps // 5 + 1 and res["positions"].shape == (32, 3)
    for key in ("harmonic_frequencies", "effective_frequencies", "fitted_frequencies", "linewidths", "lifetimes", "mode_temperatures",
                "fit_residuals"):
        assert res[key].shape == SHAPE, key
    assert res["qpoints"].shape == (8, 3) and res["acf"].shape == SHAPE + (n_lags,) and res["lag_count"].shape == (n_lags,)
    assert res["lag_count"].tolist() == [res["n_samples"] - lag for lag in range(n_lags)]
    assert res["thermal_conductivity_rta"].shape == (3, 3) and res["sample_time"] == 5 * timestep
    return res


def _parseval(res):
    """(sum over modes of qdot2_sum, relative to kinetic_sum) from the mode temperatures the driver returns."""
    total = res["mode_temperatures"].sum() * res["n_samples"] * KAPPA * KB
    return total, abs(total - res["kinetic_sum"]) / res["kinetic_sum"]


def _gamma_acoustic(res):
    """The three modes of lowest frequency at q = 0 (the first q-point)."""
    assert np.array_equal(res["qpoints"][0], np.zeros(3)) and np.abs(res["harmonic_frequencies"][0, :3]).max() < 1e-2 < res["harmonic_frequencies"][0, 3]
    mask = np.zeros(SHAPE, dtype=bool)
    mask[0, :3] = True
    return mask


def test_langevin_run_equipartition(cu):
    """Run A: 500 + 4,000 Langevin steps, friction 0.01 / fs.  Parseval to 1e-10; the three acoustic modes at Gamma hold nothing (the
    centre of mass is removed); the mean kinetic temperature of the other 93 modes is 20 K within
    5 sqrt(2 tau_c / (T_prod 93)) + (w_max dt)^2 / 4: tau_c = 2 / friction is the correlation time of a mode's energy under this
    thermostat, taken on the long side, T_prod the production time, and the last term the integrator's known bias of the full-step
    kinetic energy."""
    friction, steps = 0.01, 4000
    res = _run(cu, "nvt_langevin", friction, steps, 500, 50)
    total, off = _parseval(res)
    acoustic = _gamma_acoustic(res)
    share = res["mode_temperatures"][acoustic].sum() / res["mode_temperatures"].sum()
    ratio = res["mode_temperatures"][~acoustic] / T
    w_max = 2.0 * np.pi * res["harmonic_frequencies"].max() * 1e-3
    bound = 5.0 * np.sqrt(2.0 * (2.0 / friction) / (steps * DT * 93)) + (w_max * DT) ** 2 / 4.0
    record_line(RECORD, f"run A (Langevin 0.01/fs, 500 + 4000 steps of 2 fs, 20 K): Parseval {off:.1e} relative; Gamma acoustic modes hold "
                        f"{share:.1e} of the kinetic sum; mode temperatures / T: mean {ratio.mean():.4f}, min {ratio.min():.2f}, max {ratio.max():.2f} "
                        f"(bound on |mean - 1|: {bound:.3f}); largest harmonic frequency {res['harmonic_frequencies'].max():.3f} THz")
    assert off <= 1e-10
    assert share < 1e-20
    assert abs(ratio.mean() - 1.0) <= bound
    assert np.isfinite(res["thermal_conductivity_rta"]).all() and res["rta_modes_excluded"] >= 3


def test_langevin_run_frequencies(cu):
    """Run B: friction 0.001 / fs, 500 + 6,000 steps, 400 lags of 10 fs.  Every mode but the three acoustic ones at Gamma is fitted
    within friction / 2 pi + 1 / (n_lags dt_sample) of its harmonic frequency: the thermostat's half width plus the window's
    resolution.  The fitted linewidths are printed beside friction / 2; their scatter is statistical and is not asserted."""
    friction, n_lags = 0.001, 400
    res = _run(cu, "nvt_langevin", friction, 6000, 500, n_lags)
    keep = ~_gamma_acoustic(res)
    off = np.abs(res["fitted_frequencies"] - res["harmonic_frequencies"])[keep]
    off_eff = np.abs(res["effective_frequencies"] - res["harmonic_frequencies"])[keep]
    bound = (friction / (2.0 * np.pi) + 1.0 / (n_lags * res["sample_time"])) * 1e3   # THz
    lw = res["linewidths"][keep]
    record_line(RECORD, f"run B (Langevin 0.001/fs, 500 + 6000 steps, 400 lags of 10 fs): |fitted - harmonic| max {off.max():.3f} THz, mean "
                        f"{off.mean():.3f} (bound {bound:.3f}); |effective - harmonic| max {off_eff.max():.3f}; linewidths (1/fs) median "
                        f"{np.median(lw):.2e}, min {lw.min():.2e}, max {lw.max():.2e} beside friction / 2 = {friction / 2:.1e}; fit residual max "
                        f"{res['fit_residuals'][keep].max():.2f}")
    record_line(RECORD, f"run B: kappa_RTA diagonal {np.diag(res['thermal_conductivity_rta']).round(2).tolist()} W/(m K), "
                        f"{res['rta_modes_excluded']} modes left out (thermostatted lifetimes of a 32-atom cell: a figure for the record, not a result)")
    assert np.isfinite(off).all() and off.max() <= bound, (off.max(), bound)
    assert _parseval(res)[1] <= 1e-10


def test_nve_production_runs_and_conserves_energy():
    """production="nve" in the setup of MolecularDynamics' own NVE test (tests/test_gpu_dynamics.py: the same weights under cutoffs
    4.76 / 4.38, in a gap of the fcc shells at a = 3.61, since the model's energy jumps where a pair crosses the two-body cutoff --
    under the archive's own cutoffs at a = 3.5025 the 300 steps below move the total energy by 4.3e-3 eV): phonons of that crystal,
    100 Langevin steps, then 300 NVE steps of 1 fs; shapes, Parseval, and the total energy kept to the 3e-4 eV of that test."""
    from torch_m3gnet.model.build import build_model_from_npz
    from torch_m3gnet.phonons import Phonons

    model = build_model_from_npz(GOLDEN / "model_fitted_lj.npz", cutoff=4.76, threebody_cutoff=4.38).to(DEV)
    (ph,) = Phonons(model).run([np.eye(3) * 3.61], [FCC_BASE * 3.61], [np.full(4, 29)], (3, 3, 3))
    res = _run((model, ph), "nve", 0.01, 300, 100, 20, timestep=1.0)
    e = res["log"]["e_pot"] + res["log"]["ke"]
    drift = float(np.abs(e - e[0]).max())
    _, off = _parseval(res)
    share = res["mode_temperatures"][_gamma_acoustic(res)].sum() / res["mode_temperatures"].sum()
    record_line(RECORD, f"nve production (cutoffs 4.76 / 4.38, a = 3.61), 300 steps of 1 fs after 100 Langevin steps: total energy within {drift:.1e} eV, "
                        f"Parseval {off:.1e} relative, Gamma acoustic share {share:.1e}, mean mode temperature {res['mode_temperatures'].mean():.2f} K")
    assert drift < 3e-4 and off <= 1e-10 and share < 1e-20
    assert np.isfinite(res["mode_temperatures"]).all() and np.isfinite(res["effective_frequencies"][~_gamma_acoustic(res)]).all()
