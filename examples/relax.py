#!/usr/bin/env python3
"""Structure relaxation with the cell relaxed (FIRE, then L-BFGS, over a unit-cell filter) on the MI355X engine: the scenario of the reference's
relaxation script (scripts/relax_org.py: m3gnet's Relaxer, fmax = 0.1, steps = 500) on the weights this project ships.

    python examples/relax.py [fmax] [steps]

The model is the default M3GNet architecture with the LJ-fitted fixture weights (tests/golden/model_fitted_lj.npz: fitted with the
reference's own code to Lennard-Jones Cu).  The structure is a compressed (a = 3.40 A) and rattled 2 x 2 x 2 fcc Cu cell; the
relaxation expands it to the model's own lattice constant.  Runs FIRE and L-BFGS from the same start and prints, for each, the steps
taken, the final lattice constant and the energy per atom."""
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "torch-m3gnet_amd"):
    sys.path.insert(0, str(p))
from torch_m3gnet.model.build import build_model_from_npz  # noqa: E402
from torch_m3gnet.relax import Relaxer  # noqa: E402

fmax = float(sys.argv[1]) if len(sys.argv) > 1 else 0.1
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 500
model = build_model_from_npz(ROOT / "tests" / "golden" / "model_fitted_lj.npz").to("cuda")   # (weights as data)

a, n = 3.40, 2
base = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])
gi = np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij"), -1)
pos = (gi.reshape(-1, 1, 3) + base[None]).reshape(-1, 3) * a + np.random.default_rng(0).normal(0, 0.05, (4 * n ** 3, 3))
lat = np.eye(3) * n * a

ok = True
for optimizer in ("fire", "lbfgs"):
    relaxer = Relaxer(model, relax_cell=True, optimizer=optimizer)
    t0 = time.perf_counter()
    (res,) = relaxer.relax([lat], [pos], [np.full(len(pos), 29)], fmax=fmax, steps=steps)
    elapsed = time.perf_counter() - t0
    lat_f = res["lattice"]
    a_f = abs(np.linalg.det(lat_f)) ** (1 / 3) / n
    f_max = float(np.sqrt((res["forces"] ** 2).sum(1).max()))
    print(f"{optimizer}: converged={res['converged']}  steps={res['n_steps']}  ({elapsed:.2f} s)")
    print(f"  lattice constant {a:.4f} -> {a_f:.4f} A   (cell diagonal / {n}: {np.round(np.diag(lat_f) / n, 4)}, largest off-diagonal "
          f"{np.abs(lat_f - np.diag(np.diag(lat_f))).max():.1e} A)")
    print(f"  energy {res['total_energy'] / len(pos):.5f} eV/atom   max |f| {f_max:.4f} eV/A   stresses (pair virial) {np.round(res['stresses'], 5)}")
    ok = ok and res["converged"]
sys.exit(0 if ok else 1)
