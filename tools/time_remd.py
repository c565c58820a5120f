#!/usr/bin/env python3
"""Cost of batched replica exchange (torch_m3gnet.replica_exchange): the device time of the two m3g_remd_exchange launches beside the
three m3g_dyn_step launches (synthetic forces and energies, 200 calls back to back, CUDA events), for 4 x 32, 64 x 32 (16 ladders of
4) and 4 x 10,000 atoms; and the per-step cost of a ReplicaExchange run at exchange_interval = 10 against MolecularDynamics on the
same batch without exchanges (LJ-fitted fixture model, 32-atom Cu cell, Langevin, no log steps).

    python tools/time_remd.py [steps]
Prints one JSON line per case."""
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "torch-m3gnet_amd"):
    sys.path.insert(0, str(p))
from torch_m3gnet.dynamics import DynState, MolecularDynamics, dyn_step, maxwell_boltzmann  # noqa: E402
from torch_m3gnet.model.build import build_model_from_npz  # noqa: E402
from torch_m3gnet.replica_exchange import RemdState, ReplicaExchange, remd_exchange  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 500
dev = torch.device("cuda")
TEMPS = [300.0, 350.0, 410.0, 480.0]
CALLS = 200


def events(fn):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(CALLS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / CALLS * 1e3   # us


def launches(name, n_ladders, n_atoms):
    rng = np.random.default_rng(0)
    S, N = 4 * n_ladders, 4 * n_ladders * n_atoms
    offsets = np.arange(S + 1) * n_atoms
    temps = np.tile(TEMPS, n_ladders)
    pos = torch.tensor(rng.uniform(0, 10, (N, 3)), device=dev)
    vel = torch.tensor(np.concatenate([maxwell_boltzmann(np.full(n_atoms, 63.546), t, s) for s, t in enumerate(temps)]), device=dev)
    dyn = DynState(pos, None, offsets, np.full(N, 63.546), vel, temps, np.arange(S), ensemble="nvt_langevin", dt=1.0, friction=0.01)
    remd = RemdState(np.arange(n_ladders + 1) * 4, temps, np.arange(n_ladders), device=dev)
    f = torch.tensor(rng.normal(0, 0.5, (N, 3)).astype(np.float32), device=dev)
    e = torch.tensor(rng.normal(-1.0, 0.1, S).astype(np.float32), device=dev)
    step_us = events(lambda: dyn_step(dyn, f))
    dyn_step(dyn, f, finish_only=True)   # a synchronous point: the pairs are attempted, accepted ones rescale their velocities
    exchange_us = events(lambda: remd_exchange(remd, dyn, e))
    r = remd.read()
    print(json.dumps({"case": name, "atoms": N, "replicas": S, "ladders": n_ladders, "dyn_step_3_launches_us": round(step_us, 2),
                      "remd_exchange_2_launches_us": round(exchange_us, 2), "pair_attempts": int(r["attempts"].sum()),
                      "pair_accepts": int(r["accepts"].sum())}), flush=True)


def run_cost(name, n_ladders, ladder_batches=True):
    model = build_model_from_npz(ROOT / "tests" / "golden" / "model_fitted_lj.npz").to(dev)
    base = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])
    gi = np.stack(np.meshgrid(np.arange(2), np.arange(2), np.arange(2), indexing="ij"), -1)
    pos = (gi.reshape(-1, 1, 3) + base[None]).reshape(-1, 3) * 3.61
    lat, z = np.eye(3) * 7.22, np.full(32, 29)
    kw = dict(timestep=2.0, friction=0.02)
    S = 4 * n_ladders
    md = MolecularDynamics(model, ensemble="nvt_langevin", temperature=np.tile(TEMPS, n_ladders), seed=0, **kw)
    rx = ReplicaExchange(model, TEMPS, exchange_interval=10, seed=0, ladder_batches=ladder_batches, **kw)
    out = {}
    for key, fn in (("md_ms_per_step", lambda n: md.run([lat] * S, [pos] * S, [z] * S, n, loginterval=n)),
                    ("remd_ms_per_step", lambda n: rx.run([lat] * n_ladders, [pos] * n_ladders, [z] * n_ladders, n, loginterval=n))):
        fn(20)
        wall = []
        for n in (steps // 5, steps):   # the slope between two run lengths: set-up and the final copies cancel
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(n)
            torch.cuda.synchronize()
            wall.append(time.perf_counter() - t0)
        out[key] = round((wall[1] - wall[0]) / (steps - steps // 5) * 1e3, 4)
    out["extra_ms_per_step"] = round(out["remd_ms_per_step"] - out["md_ms_per_step"], 4)
    print(json.dumps(dict({"case": name, "replicas": S, "ladders": n_ladders, "ladder_batches": ladder_batches, "exchange_interval": 10,
                           "steps": steps}, **out)), flush=True)


launches("4x32", 1, 32)
launches("64x32", 16, 32)
launches("4x10000", 1, 10000)
run_cost("cu32 ladder of 4", 1)
run_cost("16 cu32 ladders of 4, one engine batch per ladder", 16, True)
run_cost("16 cu32 ladders of 4, one engine batch", 16, False)
