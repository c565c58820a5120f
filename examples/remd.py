#!/usr/bin/env python3
"""Replica-exchange molecular dynamics (parallel tempering) on the MI355X engine: a six-temperature ladder of the 32-atom Cu cell in
one batch (torch_m3gnet.replica_exchange.ReplicaExchange; Langevin, an exchange attempt every 20 steps, two launches each).

    python examples/remd.py [steps] [dt_fs]

The model is the default M3GNet architecture with the LJ-fitted fixture weights (tests/golden/model_fitted_lj.npz: fitted with the
reference's own code to Lennard-Jones Cu).  Prints the acceptance of every neighbouring pair, the mean potential energy and the heat
capacity var(E) / (kB T^2) at every temperature, and the round trips of the copies."""
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "torch-m3gnet_amd"):
    sys.path.insert(0, str(p))
from torch_m3gnet.model.build import build_model_from_npz  # noqa: E402
from torch_m3gnet.replica_exchange import KB, ReplicaExchange  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 4000
dt = float(sys.argv[2]) if len(sys.argv) > 2 else 2.0
model = build_model_from_npz(ROOT / "tests" / "golden" / "model_fitted_lj.npz").to("cuda")   # (weights as data)

a, n = 3.61, 2
base = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])
gi = np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij"), -1)
pos = (gi.reshape(-1, 1, 3) + base[None]).reshape(-1, 3) * a
lat = np.eye(3) * n * a
z = np.full(len(pos), 29)

temps = [300.0, 345.0, 395.0, 450.0, 515.0, 590.0]   # geometric: equal acceptance for a constant heat capacity
rx = ReplicaExchange(model, temps, timestep=dt, friction=0.02, exchange_interval=20, seed=0)
t0 = time.perf_counter()
(res,) = rx.run([lat], [pos], [z], steps, loginterval=20)
elapsed = time.perf_counter() - t0
n_att = len(res["temperature_index"]) - 1
print(f"{len(temps)} x {len(z)} atoms: {steps} steps of {dt} fs, {n_att} exchange attempts, in {elapsed:.2f} s "
      f"({elapsed / max(steps, 1) * 1e3:.3f} ms per step)")
print("   T (K)   <E_pot> (eV/atom)   Cv / (N kB)   mean T of the holder (K)   acceptance with the next")
ok = not res["error"]
for k, t in enumerate(temps):
    rep = res["replicas"][k]
    held = res["temperature_index"][1:] == k                      # [attempts, R]: who held T_k after every attempt
    t_kin = res["kinetic_temperature"][:, 1][held].mean() if n_att else float("nan")
    acc = f"{res['acceptance'][k]:.2f} ({res['attempts'][k]} attempts)" if k + 1 < len(temps) else ""
    print(f"  {t:6.1f}   {res['mean_energy'][k] / len(z):12.4f}   {res['heat_capacity'][k] / (len(z) * KB):11.2f}   {t_kin:12.1f}"
          f"               {acc}")
    ok &= rep["temperature"] == t == rep["target_temperature"]
print("round trips of the copies:", res["round_trips"].tolist(), "  final temperature index of every copy:",
      res["temperature_index"][-1].tolist())
ok &= bool((np.sort(res["temperature_index"], axis=1) == np.arange(len(temps))[None]).all())
if n_att >= 50:   # with enough attempts every pair exchanges and the mean energy rises with the temperature
    ok &= bool((res["acceptance"] > 0.05).all()) and bool((np.diff(res["mean_energy"]) > 0).all())
sys.exit(0 if ok else 1)
