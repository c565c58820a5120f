#!/usr/bin/env python3
"""Phonon frequencies at temperature and phonon lifetimes by normal-mode decomposition of MD on the MI355X engine: harmonic phonons of
fcc Cu first (torch_m3gnet.phonons.Phonons), then an MD supercell whose trajectory is projected, on the device, on the harmonic
eigenvectors at the commensurate q-points (torch_m3gnet.normal_modes.NormalModeAnalysis; three launches per sample, no frame on the
host), and per mode the kinetic temperature, the frequency and linewidth fitted to the mode-velocity autocorrelation, and the
relaxation-time thermal conductivity from the lifetimes and the harmonic group velocities.

    python examples/phonon_lifetimes.py [steps] [temperature_K] [cells] [friction_per_fs]

The model is the default M3GNet architecture with the LJ-fitted fixture weights (tests/golden/model_fitted_lj.npz: fitted with the
reference's own code to Lennard-Jones Cu) at its own lattice constant.  Production is Langevin with a weak friction, which keeps the
run stationary where the fixture model does not conserve energy for long and ADDS friction / 2 to every linewidth: the last column
subtracts it.  Limits: diagonal supercells, at most 21 atoms per unit cell (3 n_u <= 64), classical statistics in kappa_RTA."""
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "torch-m3gnet_amd"):
    sys.path.insert(0, str(p))
from torch_m3gnet.model.build import build_model_from_npz  # noqa: E402
from torch_m3gnet.normal_modes import NormalModeAnalysis  # noqa: E402
from torch_m3gnet.phonons import Phonons  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
temperature = float(sys.argv[2]) if len(sys.argv) > 2 else 40.0
cells = int(sys.argv[3]) if len(sys.argv) > 3 else 3
friction = float(sys.argv[4]) if len(sys.argv) > 4 else 5e-4
model = build_model_from_npz(ROOT / "tests" / "golden" / "model_fitted_lj.npz").to("cuda")   # (weights as data)

a = 3.5025
base = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])
(ph,) = Phonons(model).run([np.eye(3) * a], [base * a], [np.full(4, 29)], (3, 3, 3))
dt, interval, n_lags = 2.0, 5, 600
nma = NormalModeAnalysis(model, temperature=temperature, timestep=dt, friction=friction, production="nvt_langevin", n_lags=n_lags,
                         sample_interval=interval, seed=0)
t0 = time.perf_counter()
(res,) = nma.run([ph], (cells, cells, cells), steps, equilibration=2000, loginterval=100)
elapsed = time.perf_counter() - t0
q, f0 = res["qpoints"], res["harmonic_frequencies"]
print(f"{4 * cells ** 3} atoms, {len(q)} q-points, {f0.size} modes: 2000 + {steps} Langevin steps of {dt} fs at {temperature} K, friction {friction}/fs, "
      f"{res['n_samples']} samples, {n_lags} lags of {interval * dt} fs, in {elapsed:.2f} s ({elapsed / (steps + 2000) * 1e3:.3f} ms per step)")
total = res["mode_temperatures"].sum() * res["n_samples"]
print(f"sum over modes of <|Qdot|^2> against sum m |v|^2: {abs(total * 9.648533215665e-3 * 8.617333262e-5 / res['kinetic_sum'] - 1):.1e} relative; "
      f"mean mode temperature {res['mode_temperatures'][f0 > 1e-2].mean():.2f} K")
print("    q                      harmonic  effective   fitted    Gamma      Gamma - friction/2   lifetime   T_mode")
print("                             (THz)     (THz)      (THz)    (1/ps)          (1/ps)           (ps)       (K)")
order = np.argsort(np.abs(q).sum(1))
for iq in order[:4]:
    for nu in range(f0.shape[1]):
        if f0[iq, nu] < 1e-2:
            continue
        g = res["linewidths"][iq, nu]
        print(f"  ({q[iq][0]:5.3f} {q[iq][1]:5.3f} {q[iq][2]:5.3f})  {f0[iq, nu]:8.3f}  {res['effective_frequencies'][iq, nu]:8.3f}  "
              f"{res['fitted_frequencies'][iq, nu]:8.3f}  {g * 1e3:8.3f}  {(g - friction / 2) * 1e3:14.3f}  {res['lifetimes'][iq, nu] * 1e-3:12.2f}  "
              f"{res['mode_temperatures'][iq, nu]:7.1f}")
keep = f0 > 1e-2
shift = (res["fitted_frequencies"] - f0)[keep]
print(f"all {keep.sum()} modes: fitted - harmonic mean {shift.mean():+.3f} THz, largest {np.abs(shift).max():.3f}; median linewidth "
      f"{np.median(res['linewidths'][keep]) * 1e3:.3f} / ps beside friction / 2 = {friction / 2 * 1e3:.3f} / ps")
print(f"kappa_RTA (classical, thermostatted lifetimes) diagonal {np.diag(res['thermal_conductivity_rta']).round(2).tolist()} W/(m K), "
      f"{res['rta_modes_excluded']} modes left out")
ok = not res["error"] and not res["nonfinite"] and np.isfinite(res["fitted_frequencies"][keep]).all() and np.abs(shift).max() < 1.0
sys.exit(0 if ok else 1)
