#!/usr/bin/env python3
"""Vacancy migration barrier in fcc Cu with the climbing-image NEB on the MI355X engine.

    python examples/neb.py [fmax] [steps]

The model is the default M3GNet architecture with the LJ-fitted fixture weights (tests/golden/model_fitted_lj.npz: fitted with the
reference's own code to Lennard-Jones Cu).  A 2 x 2 x 2 fcc cell (a = 3.60 A) without one atom; a nearest neighbour hops into the
vacancy.  The endpoints are relaxed first, then 5 interior images are optimised with the climbing image on.  Prints the steps taken,
the energy profile and the barrier."""
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "torch-m3gnet_amd"):
    sys.path.insert(0, str(p))
from torch_m3gnet.model.build import build_model_from_npz  # noqa: E402
from torch_m3gnet.neb import NEB, interpolate  # noqa: E402

fmax = float(sys.argv[1]) if len(sys.argv) > 1 else 0.02
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 500
model = build_model_from_npz(ROOT / "tests" / "golden" / "model_fitted_lj.npz").to("cuda")   # (weights as data)

a, n = 3.60, 2
base = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])
gi = np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij"), -1)
sites = (gi.reshape(-1, 1, 3) + base[None]).reshape(-1, 3) * a
lat = np.eye(3) * n * a
initial = sites[1:].copy()     # vacancy on site 0
final = initial.copy()
final[0] = sites[0]            # the atom on site 1 has moved into it
images = interpolate(lat, initial, final, 7)

t0 = time.perf_counter()
(res,) = NEB(model, k=0.1, climb=True).run([(lat, np.full(len(initial), 29), images)], fmax=fmax, steps=steps, relax_endpoints=True,
                                          endpoint_fmax=0.005)
elapsed = time.perf_counter() - t0
print(f"converged={res['converged']}  steps={res['n_steps']}  climbing image {res['climbing_image']}  ({elapsed:.2f} s)")
path = np.concatenate([[0.0], np.cumsum(np.linalg.norm(np.diff(res["positions"], axis=0).reshape(len(images) - 1, -1), axis=1))])
for j, (s, e) in enumerate(zip(path, res["energies"])):
    print(f"  image {j}  path {s:6.3f} A  E - E0 {e - res['energies'][0]:+.4f} eV" + ("  <- climbing" if j == res["climbing_image"] else ""))
print(f"barrier forward {res['barrier_forward']:.4f} eV  backward {res['barrier_backward']:.4f} eV")
sys.exit(0 if res["converged"] else 1)
