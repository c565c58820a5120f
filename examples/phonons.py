#!/usr/bin/env python3
"""Phonons of fcc Cu by finite displacements on the MI355X engine: band structure, density of states and harmonic free energy.

    python examples/phonons.py [supercell]

The model is the default M3GNet architecture with the LJ-fitted fixture weights (tests/golden/model_fitted_lj.npz: fitted with the
reference's own code to Lennard-Jones Cu).  The 32-atom cubic cell is relaxed with its cell first (Relaxer); the 4-atom conventional
cell at the relaxed lattice constant then goes through Phonons with an n x n x n supercell (default 3).  Prints the residual force,
the acoustic sum rule violation, the frequencies at the special points of Gamma-X-W-K-Gamma-L (conventional-cell coordinates: the
primitive bands folded), the sound velocities along [100] (group velocities at a small q), a coarse DOS and F(T)."""
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "torch-m3gnet_amd"):
    sys.path.insert(0, str(p))
from torch_m3gnet.model.build import build_model_from_npz  # noqa: E402
from torch_m3gnet.phonons import Phonons  # noqa: E402
from torch_m3gnet.relax import Relaxer  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 3
model = build_model_from_npz(ROOT / "tests" / "golden" / "model_fitted_lj.npz").to("cuda")   # (weights as data)

base = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])
grid = np.stack(np.meshgrid(*[np.arange(2)] * 3, indexing="ij"), -1).reshape(-1, 1, 3)
a = 3.55
(rel,) = Relaxer(model, relax_cell=True).relax([np.eye(3) * 2 * a], [(grid + base[None]).reshape(-1, 3) * a], [np.full(32, 29)], fmax=1e-3)
a0 = float(np.trace(rel["lattice"])) / 6
print(f"relaxed: a0 = {a0:.4f} A  ({rel['n_steps']} FIRE steps, converged={rel['converged']})")

t0 = time.perf_counter()
(res,) = Phonons(model).run([np.eye(3) * a0], [base * a0], [np.full(4, 29)], (n, n, n))
points = {"G": (0, 0, 0), "X": (0, 1, 0), "W": (0.5, 1, 0), "K": (0.75, 0.75, 0), "L": (0.5, 0.5, 0.5)}
bands = res.band_structure([points[k] for k in "GXWKGL"], npts=41)
dos = res.dos(mesh=(12, 12, 12), sigma=0.15, npts=61)
thermal = res.thermal_properties([0, 100, 300, 600, 1000], mesh=(12, 12, 12))
print(f"phonons ({n}x{n}x{n} supercell, {4 * n ** 3} atoms, {1 + 24} evaluations): {time.perf_counter() - t0:.2f} s")
print(f"residual fmax {res.residual_fmax:.2e} eV/A  raw ASR violation {res.asr_violation:.2e} eV/A^2  error={res.error}")
f = bands["frequencies"]
for k, i in zip("GXWKGL", range(0, len(f) + 1, 41)):
    i = min(i, len(f) - 1)
    print(f"  {k}  " + " ".join(f"{x:6.3f}" for x in f[i]) + "  THz")
v = res.group_velocities(np.array([[0.01, 0.0, 0.0]]) @ res.lattice.T)[0, :3, 0]   # q = 0.01 1/A along x (Cartesian, no 2 pi)
print(f"sound velocities along [100]: TA {100 * v[0]:.0f}, {100 * v[1]:.0f} m/s  LA {100 * v[2]:.0f} m/s")
print(f"band range {f.min():.3f} .. {f.max():.3f} THz  (imaginary modes: {(f < -0.05).sum()})")
g, fp = dos["dos"], dos["frequency_points"]
print("DOS (states/THz per cell):")
for x, y in zip(fp[::6], g[::6]):
    print(f"  {x:6.2f} THz  {y:7.4f}  " + "#" * int(round(20 * y / g.max())))
print("T (K)    F (eV/cell)   S (meV/K/cell)   Cv (meV/K/cell)   E (eV/cell)")
for i, T in enumerate(thermal["temperatures"]):
    print(f"{T:6.0f}  {thermal['free_energy'][i]:+.6f}   {1e3 * thermal['entropy'][i]:10.5f}   {1e3 * thermal['heat_capacity'][i]:10.5f}"
          f"   {thermal['energy'][i]:+.6f}")
print(f"modes left out below {res.cutoff_frequency} THz: {thermal['n_excluded']}")
