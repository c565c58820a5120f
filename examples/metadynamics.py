#!/usr/bin/env python3
"""Free-energy barrier of a vacancy hop in fcc Cu at finite temperature by well-tempered metadynamics with four walkers, beside the
0 K barrier of the climbing-image NEB, on the MI355X engine.

    python examples/metadynamics.py [steps] [temperature]

The model is the default M3GNet architecture with the LJ-fitted fixture weights (tests/golden/model_fitted_lj.npz).  A 2 x 2 x 2 fcc
cell (a = 3.60 A) without one atom: 31 atoms; the atom on site 1 hops into the vacancy on site 0.  The collective variable is the
projection of that atom, relative to the centre of the other 30, on the hop direction: 0 at its own site, |hop| = a / sqrt 2 = 2.55 A
in the vacancy.  Walls keep it between -0.4 A and |hop| + 0.4 A, so the run samples this hop and not the eleven others the atom could
make.  Prints the free energy along the hop and its barrier beside NEB's.

Caveats: a run of a few thousand steps is far from converged (the estimate's error is several hill heights); the model's energy
steps by a few meV where a pair crosses its two-body cutoff, which the hop drags pairs through; and the free energy at
temperature T differs from the 0 K barrier by the entropy of the saddle."""
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "torch-m3gnet_amd"):
    sys.path.insert(0, str(p))
from torch_m3gnet.metadynamics import Metadynamics, projection  # noqa: E402
from torch_m3gnet.model.build import build_model_from_npz  # noqa: E402
from torch_m3gnet.neb import NEB, interpolate  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 4000
temperature = float(sys.argv[2]) if len(sys.argv) > 2 else 800.0
model = build_model_from_npz(ROOT / "tests" / "golden" / "model_fitted_lj.npz").to("cuda")   # (weights as data)

a, n = 3.60, 2
base = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])
gi = np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij"), -1)
sites = (gi.reshape(-1, 1, 3) + base[None]).reshape(-1, 3) * a
lat, z = np.eye(3) * n * a, np.full(31, 29)
initial = sites[1:].copy()     # vacancy on site 0; atom 0 of the cell sits on site 1
hop = sites[0] - sites[1]
length = float(np.linalg.norm(hop))

final = initial.copy()
final[0] = sites[0]
(neb,) = NEB(model, k=0.1, climb=True).run([(lat, z, interpolate(lat, initial, final, 7))], fmax=0.02, steps=500, relax_endpoints=True,
                                           endpoint_fmax=0.005)

cv = projection([0], list(range(1, 31)), hop)
meta = Metadynamics(model, cv, temperature, height=0.03, sigma=[0.12], pace=20, bias_factor=12.0, walkers=4,
                    walls=[[-0.4, 20.0, length + 0.4, 20.0]], timestep=2.0, friction=0.02, seed=0)
t0 = time.perf_counter()
(res,) = meta.run([lat], [initial], [z], steps=steps, equilibration=200)
elapsed = time.perf_counter() - t0
grid = np.linspace(-0.3, length + 0.3, 33)
free = res["free_energy"](grid)
print(f"{steps} steps of 2 fs, 4 walkers, {res['n_hills']} hills at {temperature:.0f} K ({elapsed:.1f} s); the CV ran over "
      f"{res['cv'].min():.2f} .. {res['cv'].max():.2f} A of a hop of {length:.2f} A")
for s, f in zip(grid, free):
    print(f"  s {s:6.3f} A   F {f:7.4f} eV")
inner = (grid > 0.25 * length) & (grid < 0.75 * length)
barrier = free[inner].max() - free[grid < 0.25 * length].min()
print(f"free-energy barrier {barrier:.3f} eV at {temperature:.0f} K (metadynamics, not converged at this length)   "
      f"NEB {neb['barrier_forward']:.3f} eV at 0 K")
sys.exit(0 if not res["error"] else 1)
