#!/usr/bin/env python3
"""Thermodynamic response functions of fcc Cu at temperature from fluctuations, on the MI355X engine: a 256-atom cell under the
flexible-cell MTK barostat ("npt_mtk_cell") gives C_p, the thermal expansion, the isothermal bulk modulus and the elastic constants
from the fluctuations of enthalpy, volume and strain, accumulated on the device while it is integrated
(torch_m3gnet.thermo.ThermoObservables: nothing but the final 11 means and 66 co-moments goes to the host), printed beside the 0 K
numbers of `Elasticity`; a short Nose-Hoover NVT run then gives the Green-Kubo running integrals of the shear and bulk viscosity.

    python examples/thermo.py [npt_steps] [nvt_steps] [dt_fs] [T_K]

The model is the default M3GNet architecture with the LJ-fitted fixture weights (tests/golden/model_fitted_lj.npz: fitted with the
reference's own code to Lennard-Jones Cu).  Fluctuation estimates converge slowly -- C_ij wants some 10^5 steps, the defaults here
show the machinery in a minute -- and a crystal's Green-Kubo integral has no plateau worth the name: eta(t) is printed as it runs."""
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "torch-m3gnet_amd"):
    sys.path.insert(0, str(p))
from torch_m3gnet.dynamics import MolecularDynamics  # noqa: E402
from torch_m3gnet.elasticity import Elasticity  # noqa: E402
from torch_m3gnet.model.build import build_model_from_npz  # noqa: E402
from torch_m3gnet.thermo import KB, ThermoObservables  # noqa: E402

npt_steps = int(sys.argv[1]) if len(sys.argv) > 1 else 4000
nvt_steps = int(sys.argv[2]) if len(sys.argv) > 2 else 2000
dt = float(sys.argv[3]) if len(sys.argv) > 3 else 2.0
temp = float(sys.argv[4]) if len(sys.argv) > 4 else 300.0
model = build_model_from_npz(ROOT / "tests" / "golden" / "model_fitted_lj.npz").to("cuda")   # (weights as data)

a, n = 3.5, 4
base = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])
gi = np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij"), -1)
pos = (gi.reshape(-1, 1, 3) + base[None]).reshape(-1, 3) * a
lat = np.eye(3) * n * a
z = np.full(len(pos), 29)

t0 = time.perf_counter()
(el,) = Elasticity(model).run([np.eye(3) * a], [base * a], [np.full(4, 29)])
print(f"0 K (Elasticity, a = {a} A, {time.perf_counter() - t0:.2f} s): C11 {el.C_gpa[0, 0]:.1f}  C12 {el.C_gpa[0, 1]:.1f}  C44 {el.C_gpa[3, 3]:.1f}  "
      f"K_Hill {el.k_hill_gpa:.1f} GPa")

thermo = ThermoObservables(sample_interval=2)
md = MolecularDynamics(model, ensemble="npt_mtk_cell", timestep=dt, temperature=temp, pressure=0.0, taut=100.0, taup=500.0, seed=0)
t0 = time.perf_counter()
(npt,) = md.run([lat], [pos], [z], npt_steps, loginterval=100, observables=thermo)
elapsed = time.perf_counter() - t0
th = npt["thermo"]
print(f"npt_mtk_cell, {len(z)} atoms at {temp:g} K, 0 GPa: {npt_steps} steps of {dt} fs in {elapsed:.2f} s ({elapsed / max(npt_steps, 1) * 1e3:.3f} ms "
      f"per step), {th['n_samples']} samples, {th['n_skipped']} skipped")
print(f"  <T> {th['t']:.1f} K  <V> {th['v']:.2f} A^3  <p> {th['p']:.3f} GPa  <h> {th['h']:.3f} eV  mean strain " + " ".join(f"{x:+.4f}" for x in th["strain"]))
print(f"  C_p {th['heat_capacity_kb']:.2f} kB per atom (Dulong-Petit: 3)   alpha_V {th['thermal_expansion']:.2e} 1/K   B_T {th['bulk_modulus']:.1f} GPa "
      f"(kappa_T {th['compressibility']:.2e} 1/GPa)")
c = th["elastic_constants"]
print("  C (GPa) from the strain fluctuations, Voigt order xx yy zz yz zx xy:")
for row in c:
    print("    " + " ".join(f"{x:8.1f}" for x in row))
print(f"  cubic averages: C11 {np.mean(np.diag(c)[:3]):.1f}  C12 {np.mean([c[0, 1], c[0, 2], c[1, 2]]):.1f}  C44 {np.mean(np.diag(c)[3:]):.1f} GPa")

lags = 200
visc = ThermoObservables(n_lags=lags, sample_interval=2, plateau_window=(0.5, 1.0))
nvt = MolecularDynamics(model, ensemble="nvt_nose_hoover", timestep=dt, temperature=temp, taut=100.0, seed=1)
t0 = time.perf_counter()
(run,) = nvt.run([npt["lattice"]], [npt["positions"]], [z], nvt_steps, velocities=[npt["velocities"]], loginterval=100, observables=visc)
elapsed = time.perf_counter() - t0
gk = run["thermo"]
print(f"nvt_nose_hoover from the last NPT frame: {nvt_steps} steps in {elapsed:.2f} s, {gk['n_samples']} samples, C_v {gk['heat_capacity_kb']:.2f} kB "
      f"per atom, <P> (eV/A^3) " + " ".join(f"{x:+.5f}" for x in gk["tensor_mean"][:6]))
print("   time fs   shear ACF   bulk ACF (eV^2/A^6)   eta_shear   eta_bulk (mPa s)   samples")
for k in range(0, lags, lags // 10):
    print(f"  {gk['time'][k]:8.1f}  {gk['shear_acf'][k]:10.3e}  {gk['bulk_acf'][k]:10.3e}            {gk['eta_shear'][k]:9.4f}  {gk['eta_bulk'][k]:9.4f}"
          f"            {gk['lag_count'][k]:7d}")
print(f"  mean of the running integrals over the last half of the lags: shear {gk['viscosity_shear']:.4f}, bulk {gk['viscosity_bulk']:.4f} mPa s "
      f"(kB T = {KB * temp:.4f} eV)")
ok = (not npt["error"] and not run["error"] and th["n_skipped"] == 0 and gk["n_skipped"] == 0 and np.isfinite(th["heat_capacity"])
      and np.isfinite(th["bulk_modulus"]) and np.isfinite(c).all() and np.isfinite(gk["eta_shear"]).all())
sys.exit(0 if ok else 1)
