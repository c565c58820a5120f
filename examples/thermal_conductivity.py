#!/usr/bin/env python3
"""Lattice thermal conductivity by reverse non-equilibrium MD (Mueller-Plathe) on the MI355X engine: an elongated fcc Cu cell, the
hottest atom of slab 0 and the coldest of the middle slab exchange their velocities every `swap_interval` steps, and the temperature
profile between the two slabs is the response (torch_m3gnet.transport.ReverseNEMD; two launches per exchange, plain NVE otherwise).

    python examples/thermal_conductivity.py [steps] [temperature_K] [cells_along_z] [swap_interval]

The model is the default M3GNet architecture with the LJ-fitted fixture weights (tests/golden/model_fitted_lj.npz: fitted with the
reference's own code to Lennard-Jones Cu).  The lattice constant (3.35 A) keeps every neighbour shell a quarter of an angstrom from the
model's two-body cutoff, where its energy is not continuous.  Prints the temperature of every slab with its standard error over blocks,
the slopes on both sides of the source slab, the flux and kappa.  kappa of a cell this short is far below the bulk value: phonons
whose mean free path exceeds the distance between the exchange slabs are cut off.  Run several lengths and extrapolate 1 / kappa
against 1 / L."""
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "torch-m3gnet_amd"):
    sys.path.insert(0, str(p))
from torch_m3gnet.dynamics import KAPPA, KB  # noqa: E402
from torch_m3gnet.model.build import build_model_from_npz  # noqa: E402
from torch_m3gnet.transport import ReverseNEMD  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 6000
temperature = float(sys.argv[2]) if len(sys.argv) > 2 else 40.0
nz = int(sys.argv[3]) if len(sys.argv) > 3 else 12
swap_interval = int(sys.argv[4]) if len(sys.argv) > 4 else 20
model = build_model_from_npz(ROOT / "tests" / "golden" / "model_fitted_lj.npz").to("cuda")   # (weights as data)

a, nx = 3.35, 3
base = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])
gi = np.stack(np.meshgrid(np.arange(nx), np.arange(nx), np.arange(nz), indexing="ij"), -1)
pos = (gi.reshape(-1, 1, 3) + base[None]).reshape(-1, 3) * a + [0.0, 0.0, 0.25 * a]   # atomic planes inside the slabs, not on their faces
lat = np.diag([nx, nx, nz]) * a
z = np.full(len(pos), 29)

blocks, discard = 5, steps // 3
md = ReverseNEMD(model, kind="heat", temperature=temperature, timestep=2.0, axis=2, n_slabs=nz, n_swaps=1, swap_interval=swap_interval,
                 sample_interval=10, friction=0.02, seed=0)
t0 = time.perf_counter()
(res,) = md.run([lat], [pos], [z], steps, equilibration=1000, discard=discard, loginterval=50, blocks=blocks)
elapsed = time.perf_counter() - t0
e_tot = res["log"]["e_pot"] + res["log"]["ke"]
print(f"{len(z)} atoms, {nz} slabs of {a} A: 1000 Langevin steps at {temperature} K, then {steps} NVE steps of 2 fs with an exchange every "
      f"{swap_interval}, in {elapsed:.2f} s ({elapsed / (steps + 1000) * 1e3:.3f} ms per step)")
print(f"pairs exchanged {res['n_exchanged']} in {res['n_calls']} calls; {res['transferred']:.4f} eV through 2 x {(nx * a) ** 2:.1f} A^2 in "
      f"{(steps - discard) * 2.0:.0f} fs after step {discard}; total energy within {np.abs(e_tot - e_tot[0]).max():.2e} eV")
with np.errstate(invalid="ignore", divide="ignore"):
    t_blocks = res["block_sums"][:, :, 4] / (3.0 * KB * KAPPA * res["block_counts"])
err = t_blocks.std(axis=0, ddof=1) / np.sqrt(len(t_blocks)) if len(t_blocks) > 1 else np.full(nz, np.nan)
print("  slab   z (A)    T (K)    +-    atoms")
for b in range(nz):
    mark = "  sink" if b == 0 else ("  source" if b == nz // 2 else "")
    print(f"  {b:4d}  {res['slab_centres'][b]:6.2f}  {res['temperature_profile'][b]:7.2f}  {err[b]:5.2f}  {res['counts'][b] / max(res['n_samples'], 1):6.1f}{mark}")
print(f"slopes {res['gradient_sides'][0]:+.3f} / {res['gradient_sides'][1]:+.3f} K/A, flux {res['flux']:.3e} eV/(A^2 fs), "
      f"kappa({nz * a:.1f} A) = {res['thermal_conductivity']:.3f} W/(m K)")
ok = not res["error"] and res["transferred"] > 0 and np.isfinite(res["thermal_conductivity"]) and res["thermal_conductivity"] > 0
ok &= bool(res["gradient_sides"][0] > 0 > res["gradient_sides"][1])
sys.exit(0 if ok else 1)
