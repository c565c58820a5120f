#!/usr/bin/env python3
"""Scattering observables of a Langevin run on the MI355X engine: the 256-atom Cu cell at 300 K, sampled on the device while it is
integrated, in real space (torch_m3gnet.trajectory.TrajectoryObservables) and in reciprocal space
(torch_m3gnet.scattering.ScatteringObservables) at once: no frame goes to the host.

    python examples/structure_factor.py [steps] [dt_fs]

The model is the default M3GNet architecture with the LJ-fitted fixture weights (tests/golden/model_fitted_lj.npz: fitted with the
reference's own code to Lennard-Jones Cu).  Prints S(q) per |q| shell -- in a crystal it is large at the Bragg shells (those that
hold a reciprocal lattice vector of the fcc cell) and of order k T / (m c^2) between them -- and the longitudinal dispersion: the
frequency at which the spectrum of the longitudinal current correlation C_L(q, t) of a shell is largest."""
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "torch-m3gnet_amd"):
    sys.path.insert(0, str(p))
from torch_m3gnet.dynamics import MolecularDynamics  # noqa: E402
from torch_m3gnet.model.build import build_model_from_npz  # noqa: E402
from torch_m3gnet.scattering import ScatteringObservables  # noqa: E402
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

observables = [TrajectoryObservables(rdf_bins=200, n_lags=256, sample_interval=2),
               ScatteringObservables(q_max=3.1, n_lags=256, sample_interval=2, max_per_shell=None)]   # every vector up to the (111) Bragg
                                                                                                      # shell at 3.01 1/A: none thinned away
md = MolecularDynamics(model, ensemble="nvt_langevin", timestep=dt, temperature=300.0, friction=0.02, seed=0)
t0 = time.perf_counter()
(res,) = md.run([lat], [pos], [z], steps, loginterval=10, observables=observables)
elapsed = time.perf_counter() - t0
sq = res["scattering"]
print(f"Langevin, {len(z)} atoms: {steps} steps of {dt} fs in {elapsed:.2f} s ({elapsed / steps * 1e3:.3f} ms per step), "
      f"{sq['n_samples']} samples, {len(sq['hkl'])} q-vectors in {len(sq['q_shell'])} shells")
print("  |q| 1/A   vectors   S(q)        longitudinal peak THz")
for q, count, s, f in zip(sq["q_shell"], sq["shell_count"], sq["s_shell"], sq["dispersion_l"]):
    print(f"  {q:7.3f}   {count:7d}   {s:10.4f}  {f:8.2f}")
bragg = 2 * np.pi / a * np.sqrt(3.0)   # (111) of the conventional cell
at_bragg = sq["s"][np.abs(sq["q_modulus"] - bragg) < 1e-6]
between = sq["s"][sq["q_modulus"] < 0.9 * bragg]
print(f"  S at the (111) vectors: {at_bragg.mean():.1f} of {len(z)} at most; below them: {between.mean():.4f} on average")
ok = not res["error"] and sq["cell_valid"] and (sq["s"] >= 0).all() and len(at_bragg) > 0 and at_bragg.mean() > 50 * between.mean()
sys.exit(0 if ok else 1)
