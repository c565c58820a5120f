#!/usr/bin/env python3
"""Trajectory observables of a Langevin run on the MI355X engine: the 256-atom Cu cell at 300 K, sampled on the device while it is
integrated (torch_m3gnet.trajectory.TrajectoryObservables: no frame goes to the host).

    python examples/md_observables.py [steps] [dt_fs]

The model is the default M3GNet architecture with the LJ-fitted fixture weights (tests/golden/model_fitted_lj.npz: fitted with the
reference's own code to Lennard-Jones Cu).  Prints the first peak of g(r) and the coordination number at the first minimum, the
diffusion coefficient from the MSD slope and from the VACF integral (a solid: both near zero), and the peak of the vibrational
density of states."""
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "torch-m3gnet_amd"):
    sys.path.insert(0, str(p))
from torch_m3gnet.dynamics import MolecularDynamics  # noqa: E402
from torch_m3gnet.model.build import build_model_from_npz  # noqa: E402
from torch_m3gnet.trajectory import TrajectoryObservables  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
dt = float(sys.argv[2]) if len(sys.argv) > 2 else 2.0
model = build_model_from_npz(ROOT / "tests" / "golden" / "model_fitted_lj.npz").to("cuda")   # (weights as data)

a, n = 3.61, 4
base = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])
gi = np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij"), -1)
pos = (gi.reshape(-1, 1, 3) + base[None]).reshape(-1, 3) * a
lat = np.eye(3) * n * a
z = np.full(len(pos), 29)

observables = TrajectoryObservables(rdf_bins=200, n_lags=256, sample_interval=2)   # rdf_r_max: half the cell, the largest exact range
md = MolecularDynamics(model, ensemble="nvt_langevin", timestep=dt, temperature=300.0, friction=0.02, seed=0)
t0 = time.perf_counter()
(res,) = md.run([lat], [pos], [z], steps, loginterval=10, observables=observables)
elapsed = time.perf_counter() - t0
obs = res["observables"]
print(f"Langevin, {len(z)} atoms: {steps} steps of {dt} fs in {elapsed:.2f} s ({elapsed / steps * 1e3:.3f} ms per step), "
      f"{obs['n_samples']} samples")

g, r = obs["g"][0][0], obs["r"]
peak = int(np.argmax(g))
minimum = peak + int(np.argmin(g[peak:peak + len(g) // 4]))   # the first minimum behind the peak
print(f"  g(r): first peak {g[peak]:.2f} at {r[peak]:.3f} A (fcc nearest neighbours: {a / np.sqrt(2):.3f} A); "
      f"coordination up to {obs['r_edges'][minimum + 1]:.2f} A: {obs['coordination'][0][0][minimum]:.2f}")
print(f"  D from the MSD slope {obs['diffusion_msd_cm2_s'][0]:.2e} cm^2/s, from the VACF integral {obs['diffusion_vacf_cm2_s'][0]:.2e} cm^2/s; "
      f"MSD at {obs['time'][-1]:.0f} fs: {obs['msd'][0][-1]:.4f} A^2")
k = int(np.argmax(obs["vdos"][0]))
print(f"  VDOS peak at {obs['vdos_frequency'][k]:.2f} THz (resolution {obs['vdos_frequency'][1]:.2f} THz)")
ok = not res["error"] and obs["rdf_valid"] and abs(r[peak] - a / np.sqrt(2)) < 0.15 and abs(obs["coordination"][0][0][minimum] - 12) < 1
sys.exit(0 if ok else 1)
