#!/usr/bin/env python3
"""Local order of a Langevin run on the MI355X engine: the 256-atom Cu cell at 300 K and, in the same batch, at a temperature well
above melting, sampled on the device while it is integrated (torch_m3gnet.local_order.LocalOrderObservables): no frame goes to the
host.

    python examples/local_order.py [steps] [dt_fs] [hot_K]

The model is the default M3GNet architecture with the LJ-fitted fixture weights (tests/golden/model_fitted_lj.npz: fitted with the
reference's own code to Lennard-Jones Cu).  Prints, over time, the share of solid-like atoms (ten Wolde-Frenkel: at least 7 bonds with
q6 . q6 > 0.5), the largest cluster of them and the mean neighbour-averaged <qbar6> (0.575 in perfect fcc, near 0 in a liquid): the
cold crystal keeps all three, the superheated one loses them as it melts."""
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "torch-m3gnet_amd"):
    sys.path.insert(0, str(p))
from torch_m3gnet.dynamics import MolecularDynamics  # noqa: E402
from torch_m3gnet.local_order import LocalOrderObservables  # noqa: E402
from torch_m3gnet.model.build import build_model_from_npz  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 3000
dt = float(sys.argv[2]) if len(sys.argv) > 2 else 2.0
hot = float(sys.argv[3]) if len(sys.argv) > 3 else 3000.0
model = build_model_from_npz(ROOT / "tests" / "golden" / "model_fitted_lj.npz").to("cuda")   # (weights as data)

a, n = 3.61, 4
base = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])
gi = np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij"), -1)
pos = (gi.reshape(-1, 1, 3) + base[None]).reshape(-1, 3) * a
lat = np.eye(3) * n * a
z = np.full(len(pos), 29)

# between the first (2.55 A) and the second (3.61 A) neighbour shell of fcc Cu
local = LocalOrderObservables(r_cut={29: 3.1}, degrees=(4, 6), sample_interval=20, max_samples=1024)
md = MolecularDynamics(model, ensemble="nvt_langevin", timestep=dt, temperature=[300.0, hot], friction=0.02, seed=0)
t0 = time.perf_counter()
cold, melt = md.run([lat, lat], [pos, pos], [z, z], steps, loginterval=50, observables=local)
elapsed = time.perf_counter() - t0
lo_cold, lo_hot = cold["local_order"], melt["local_order"]
print(f"Langevin, 2 x {len(z)} atoms at 300 K and {hot:g} K: {steps} steps of {dt} fs in {elapsed:.2f} s ({elapsed / steps * 1e3:.3f} ms per "
      f"step), {lo_cold['n_samples']} samples, flags {lo_cold['flags']} / {lo_hot['flags']}")
print("  time ps   300 K: solid  largest  <qbar6>      hot: solid  largest  <qbar6>   clusters")
rows = range(0, len(lo_cold["step"]), max(1, len(lo_cold["step"]) // 15))
for k in rows:
    print(f"  {lo_cold['time'][k] * 1e-3:7.2f}   {lo_cold['solid_fraction'][k]:12.3f}  {lo_cold['largest_cluster'][k]:7d}  "
          f"{lo_cold['mean_qbar'][k, 1]:7.4f}   {lo_hot['solid_fraction'][k]:11.3f}  {lo_hot['largest_cluster'][k]:7d}  "
          f"{lo_hot['mean_qbar'][k, 1]:7.4f}   {lo_hot['n_clusters'][k]:8d}")
print(f"  over the run: <q6> {lo_cold['q_mean'][0, 1]:.4f} / {lo_hot['q_mean'][0, 1]:.4f}, <qbar6> {lo_cold['qbar_mean'][0, 1]:.4f} / "
      f"{lo_hot['qbar_mean'][0, 1]:.4f}, most frequent coordination {int(np.argmax(lo_cold['coordination_hist'][0]))} / "
      f"{int(np.argmax(lo_hot['coordination_hist'][0]))}")
ok = (not cold["error"] and not melt["error"] and lo_cold["n_skipped"] == 0 and lo_cold["solid_fraction"][-1] > 0.9
      and lo_hot["mean_qbar"][-1, 1] < lo_cold["mean_qbar"][-1, 1])
sys.exit(0 if ok else 1)
