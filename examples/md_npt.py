#!/usr/bin/env python3
"""Deterministic thermostat and barostat on the MI355X engine: the 256-atom Cu cell under a Nose-Hoover chain at 300 K (NVT), then
under the isotropic Martyna-Tobias-Klein barostat at 300 K and zero pressure (NPT), continued from the NVT run
(torch_m3gnet.dynamics.MolecularDynamics, ensembles "nvt_nose_hoover" and "npt_mtk").

    python examples/md_npt.py [steps] [dt_fs]

The model is the default M3GNet architecture with the LJ-fitted fixture weights (tests/golden/model_fitted_lj.npz: fitted with the
reference's own code to Lennard-Jones Cu).  Prints, over the second half of each run, <T> against its canonical mean t0 g / (3 n),
<P>, the mean lattice constant <a>, and the drift of the conserved quantity (at 300 K pairs cross the model's cutoffs, where its
energy jumps: the drift is the model's, and falls to the integrator's O(dt^2) on trajectories that keep inside one shell)."""
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

a, n, t0 = 3.52, 4, 300.0
base = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])
gi = np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij"), -1)
pos = (gi.reshape(-1, 1, 3) + base[None]).reshape(-1, 3) * a
lat = np.eye(3) * n * a
z = np.full(len(pos), 29)
t_canonical = t0 * (3 * len(z) - 3) / (3 * len(z))


def report(title, res, elapsed):
    log = res["log"]
    half = len(log["t"]) // 2
    t, p = log["t"][half:].mean(), log["p"][half:].mean()
    a_mean = (log["v"][half:] ** (1 / 3)).mean() / n
    drift = np.abs(log["conserved"] - log["conserved"][0]).max()
    print(f"{title}: {steps} steps of {dt} fs in {elapsed:.2f} s ({elapsed / steps * 1e3:.3f} ms per step)")
    print(f"  <T> {t:7.2f} K (canonical mean {t_canonical:.2f} K)   <P> {p:8.4f} GPa   <a> {a_mean:.4f} A   "
          f"conserved within {drift:.2e} eV ({drift / len(z):.1e} eV/atom)")
    return abs(t / t_canonical - 1.0) < 0.1 and not res["error"]


md = MolecularDynamics(model, ensemble="nvt_nose_hoover", timestep=dt, temperature=t0, taut=50.0, chain_length=3)
start = time.perf_counter()
(nvt,) = md.run([lat], [pos], [z], steps, loginterval=1)
ok = report(f"Nose-Hoover chain NVT, {len(z)} atoms", nvt, time.perf_counter() - start)

md = MolecularDynamics(model, ensemble="npt_mtk", timestep=dt, temperature=t0, taut=50.0, taup=500.0, pressure=0.0, chain_length=3)
start = time.perf_counter()
(npt,) = md.run([nvt["lattice"]], [nvt["positions"]], [z], steps, velocities=[nvt["velocities"]], loginterval=1)
ok &= report(f"MTK NPT at 0 GPa, {len(z)} atoms", npt, time.perf_counter() - start)
sys.exit(0 if ok else 1)
