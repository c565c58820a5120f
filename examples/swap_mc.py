#!/usr/bin/env python3
"""Atom-swap Monte Carlo on the MI355X engine (torch_m3gnet.monte_carlo.SwapMonteCarlo): which arrangement of 16 Cu and 16 Au atoms on
the sites of a 32-atom fcc cell does the model prefer?  A pure lattice Monte Carlo run (positions fixed, one energy-only evaluation per
trial) and a hybrid MC/MD run (a swap after every 10 Langevin steps; masses and velocities travel with the atoms).

    python examples/swap_mc.py [trials] [T_K]

The model is the default architecture with the fixture weights tests/golden/model_fitted_lj.npz: fitted to Lennard-Jones Cu, so its
Au embedding is the untrained one -- NOT a Cu-Au potential.  A swap moves its energy by ~0.01 eV, the size that matters at a few
hundred kelvin, which is all this example needs: the ordering it finds is the model's, not nature's.  Prints the acceptance, the
mean energy and the first-shell Warren-Cowley parameter alpha(Cu, Au) before and after."""
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "torch-m3gnet_amd"):
    sys.path.insert(0, str(p))
from torch_m3gnet.model.build import build_model_from_npz  # noqa: E402
from torch_m3gnet.monte_carlo import SwapMonteCarlo, short_range_order  # noqa: E402

trials = int(sys.argv[1]) if len(sys.argv) > 1 else 400
T = float(sys.argv[2]) if len(sys.argv) > 2 else 600.0
model = build_model_from_npz(ROOT / "tests" / "golden" / "model_fitted_lj.npz").to("cuda")   # (weights as data)

a, n = 3.7, 2
base = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])
gi = np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij"), -1)
rng = np.random.default_rng(0)
pos = (gi.reshape(-1, 1, 3) + base[None]).reshape(-1, 3) * a
pos = pos + rng.normal(0, 0.02, pos.shape)
lat = np.eye(3) * n * a
z = rng.permutation(np.repeat([29, 79], 16))
shell = 0.5 * (a / np.sqrt(2) + a)   # between the first and the second neighbour shell

ok = True
for name, kw, k in (("pure lattice MC", dict(), trials), ("hybrid MC/MD, 10 steps of 2 fs per trial", dict(md_steps=10, timestep=2.0, friction=0.02),
                                                        max(trials // 10, 1))):
    mc = SwapMonteCarlo(model, T, seed=0, **kw)
    t0 = time.perf_counter()
    (res,) = mc.run([lat], [pos], [z], k, loginterval=max(k // 10, 1))
    elapsed = time.perf_counter() - t0
    before = short_range_order(lat, pos, z, shell)[29, 79]
    after = short_range_order(res["lattice"], res["positions"], res["atomic_numbers"], shell)[29, 79]
    print(f"{name}: {k} trials at {T:.0f} K in {elapsed:.2f} s ({elapsed / k * 1e3:.3f} ms per trial)")
    print(f"  acceptance {res['acceptance']:.2f} ({res['attempts']} attempts, {res['nonfinite']} non-finite)   <E> {res['mean_energy'] / 32:.5f} eV/atom"
          f"   Cv / (N kB) {res['heat_capacity'] / (32 * 8.617333262e-5):.3f}")
    print(f"  E (eV) every {max(k // 10, 1)} trials: " + " ".join(f"{e:.3f}" for e in res["energy"]))
    print(f"  first-shell alpha(Cu, Au): {before:+.3f} before, {after:+.3f} after")
    ok &= not res["error"] and res["attempts"] == k and sorted(res["atomic_numbers"]) == sorted(z) and np.isfinite(res["mean_energy"])
sys.exit(0 if ok else 1)
