#!/usr/bin/env python3
"""Thermostatted molecular dynamics (Langevin, BAOAB) on the MI355X engine: the 256-atom Cu cell at 300 K, then a replica batch of the
same cell at four temperatures in one run (torch_m3gnet.dynamics.MolecularDynamics, every structure with its own target and random
stream).

    python examples/md_nvt.py [steps] [dt_fs]

The model is the default M3GNet architecture with the LJ-fitted fixture weights (tests/golden/model_fitted_lj.npz: fitted with the
reference's own code to Lennard-Jones Cu).  Prints the mean temperature of the second half of each run against its target."""
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "torch-m3gnet_amd"):
    sys.path.insert(0, str(p))
from torch_m3gnet.dynamics import MolecularDynamics  # noqa: E402
from torch_m3gnet.model.build import build_model_from_npz  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
dt = float(sys.argv[2]) if len(sys.argv) > 2 else 2.0
model = build_model_from_npz(ROOT / "tests" / "golden" / "model_fitted_lj.npz").to("cuda")   # (weights as data)

a, n = 3.61, 4
base = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])
gi = np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij"), -1)
pos = (gi.reshape(-1, 1, 3) + base[None]).reshape(-1, 3) * a
lat = np.eye(3) * n * a
z = np.full(len(pos), 29)


def report(title, temps, res, elapsed):
    print(f"{title}: {steps} steps of {dt} fs in {elapsed:.2f} s ({elapsed / steps * 1e3:.3f} ms per step)")
    ok = True
    for t0, r in zip(temps, res):
        t = r["log"]["t"][len(r["log"]["t"]) // 2:].mean()
        ok &= abs(t / t0 - 1.0) < 0.1 and not r["error"]
        print(f"  target {t0:6.1f} K   mean T (second half) {t:7.2f} K   E_pot {r['log']['e_pot'][-1] / len(z):.4f} eV/atom")
    return ok


md = MolecularDynamics(model, ensemble="nvt_langevin", timestep=dt, temperature=300.0, friction=0.02, seed=0)
t0 = time.perf_counter()
res = md.run([lat], [pos], [z], steps, loginterval=5)
ok = report(f"Langevin, {len(z)} atoms", [300.0], res, time.perf_counter() - t0)

temps = [100.0, 200.0, 300.0, 400.0]
md = MolecularDynamics(model, ensemble="nvt_langevin", timestep=dt, temperature=temps, friction=0.02, seed=1)
t0 = time.perf_counter()
res = md.run([lat] * 4, [pos] * 4, [z] * 4, steps, loginterval=5)
ok &= report(f"Langevin replica batch, 4 x {len(z)} atoms", temps, res, time.perf_counter() - t0)
sys.exit(0 if ok else 1)
