#!/usr/bin/env python3
"""Nuclear quantum effects on the MI355X engine: the 32-atom Cu cell at 50 K as a classical system (one bead) and as a ring polymer
of 8 beads under the PILE-L thermostat (torch_m3gnet.path_integral.PathIntegralMD).

    python examples/pimd.py [steps] [dt_fs]

The model is the default M3GNet architecture with the LJ-fitted fixture weights (tests/golden/model_fitted_lj.npz: fitted with the
reference's own code to Lennard-Jones Cu).  Prints, over the second half of each run, the primitive and the centroid-virial
estimator of the kinetic energy against the classical 3 n kT / 2, the potential estimator, the temperature of the ring and the
drift of the conserved quantity.  At 50 K, a seventh of copper's Debye temperature, the atoms hold several times the classical
kinetic energy: their zero-point motion."""
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "torch-m3gnet_amd"):
    sys.path.insert(0, str(p))
from torch_m3gnet.dynamics import KB  # noqa: E402
from torch_m3gnet.model.build import build_model_from_npz  # noqa: E402
from torch_m3gnet.path_integral import PathIntegralMD  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 3000
dt = float(sys.argv[2]) if len(sys.argv) > 2 else 2.0
model = build_model_from_npz(ROOT / "tests" / "golden" / "model_fitted_lj.npz").to("cuda")   # (weights as data)

a, n, t0 = 3.61, 2, 50.0
base = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])
gi = np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij"), -1)
pos = (gi.reshape(-1, 1, 3) + base[None]).reshape(-1, 3) * a
lat = np.eye(3) * n * a
z = np.full(len(pos), 29)
classical = 1.5 * len(z) * KB * t0

ok = True
for beads in (1, 8):
    md = PathIntegralMD(model, n_beads=beads, temperature=t0, timestep=dt)
    start = time.perf_counter()
    (res,) = md.run([lat], [pos], [z], steps, loginterval=1)
    elapsed = time.perf_counter() - start
    log = res["log"]
    half = len(log["time"]) // 2
    prim, cv = log["kinetic_primitive"][half:].mean(), log["kinetic_centroid_virial"][half:].mean()
    drift = np.abs(log["conserved"] - log["conserved"][0]).max()
    print(f"P = {beads}: {steps} steps of {dt} fs in {elapsed:.2f} s ({elapsed / steps * 1e3:.3f} ms per step)")
    print(f"  K_prim {prim:.4f} eV   K_cv {cv:.4f} eV   3 n kT / 2 = {classical:.4f} eV (K_cv / classical {cv / classical:.2f})   "
          f"<V> {log['potential'][half:].mean() - log['potential'][0]:+.4f} eV above the lattice")
    print(f"  <T> of the ring {log['temperature'][half:].mean():.1f} K   conserved within {drift:.2e} eV "
          f"({drift / (len(z) * beads * steps):.1e} eV per atom-step)")
    ok &= not res["error"] and (cv > 1.5 * classical if beads > 1 else abs(cv / classical - 1.0) < 1e-9)
sys.exit(0 if ok else 1)
