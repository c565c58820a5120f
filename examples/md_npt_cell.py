#!/usr/bin/env python3
"""A cell that changes shape on the MI355X engine: the 256-atom Cu cell, sheared by 1 % in xy, relaxing under the fully flexible
Martyna-Tobias-Klein barostat at 0 GPa (torch_m3gnet.dynamics.MolecularDynamics, ensemble "npt_mtk_cell", cell_mask "full").

    python examples/md_npt_cell.py [steps] [dt_fs] [temperature_K]

The model is the default M3GNet architecture with the LJ-fitted fixture weights (tests/golden/model_fitted_lj.npz: fitted with the
reference's own code to Lennard-Jones Cu).  Prints the cell angles at the start and averaged over the second half of the run, the
mean pressure tensor and lattice constant over that half, and the drift of the conserved quantity (pairs that cross the model's
cutoffs make its energy jump: the drift is then the model's, and falls to the integrator's O(dt^2) on trajectories that keep inside
one shell)."""
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
t0 = float(sys.argv[3]) if len(sys.argv) > 3 else 100.0
model = build_model_from_npz(ROOT / "tests" / "golden" / "model_fitted_lj.npz").to("cuda")   # (weights as data)

a, n, shear = 3.505, 4, 0.01
base = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])
gi = np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij"), -1)
strain = np.eye(3)
strain[0, 1] = strain[1, 0] = shear
pos = (gi.reshape(-1, 1, 3) + base[None]).reshape(-1, 3) * a @ strain
lat = np.eye(3) * n * a @ strain
z = np.full(len(pos), 29)


def angles(cells):
    """alpha, beta, gamma (degrees) of cells [..., 3, 3], rows = lattice vectors."""
    unit = cells / np.linalg.norm(cells, axis=-1, keepdims=True)
    cos = [(unit[..., i, :] * unit[..., j, :]).sum(-1) for i, j in ((1, 2), (2, 0), (0, 1))]
    return np.degrees(np.arccos(np.stack(cos, -1)))


md = MolecularDynamics(model, ensemble="npt_mtk_cell", cell_mask="full", timestep=dt, temperature=t0, taut=100.0, taup=2000.0, pressure=0.0)
start = time.perf_counter()
(res,) = md.run([lat], [pos], [z], steps, loginterval=1)
elapsed = time.perf_counter() - start
log = res["log"]
half = len(log["t"]) // 2
drift = np.abs(log["conserved"] - log["conserved"][0]).max()
angle0, angle = angles(log["lattice"][0]), angles(log["lattice"][half:]).mean(0)
print(f"flexible-cell MTK NPT at 0 GPa, {len(z)} atoms: {steps} steps of {dt} fs in {elapsed:.2f} s ({elapsed / steps * 1e3:.3f} ms per step)")
print(f"  cell angles {np.round(angle0, 3)} deg at the start, {np.round(angle, 3)} deg over the second half")
print(f"  <pressure tensor> xx yy zz yz zx xy = {np.round(log['pressure_tensor'][half:].mean(0), 4)} GPa")
print(f"  <T> {log['t'][half:].mean():.2f} K   <a> {(log['v'][half:] ** (1 / 3)).mean() / n:.4f} A   "
      f"conserved within {drift:.2e} eV ({drift / len(z):.1e} eV/atom)")
sys.exit(0 if not res["error"] and np.abs(angle - 90.0).max() < 0.5 * np.abs(angle0 - 90.0).max() else 1)
