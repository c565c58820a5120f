#!/usr/bin/env python3
"""Cost of reverse non-equilibrium MD (torch_m3gnet.transport): the device time of the two m3g_rnemd_exchange launches beside the three
m3g_dyn_step launches (synthetic forces, 200 calls back to back, CUDA events) for one structure of 128 and of 10,000 atoms and for 64
structures of 128, at 8 and 64 slabs and 1 and 8 swaps; and the per-step cost of a ReverseNEMD run at swap_interval = 10 against the
same run without exchanges (LJ-fitted fixture model, 2 x 2 x 8 Cu cell of 128 atoms, no log steps).

    python tools/time_rnemd.py [steps]
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
from torch_m3gnet.dynamics import DynState, dyn_step, maxwell_boltzmann  # noqa: E402
from torch_m3gnet.model.build import build_model_from_npz  # noqa: E402
from torch_m3gnet.transport import ReverseNEMD, RnemdState, rnemd_exchange  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 500
dev = torch.device("cuda")
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


def launches(n_structs, n_atoms, n_slabs, n_swaps, kind="heat"):
    rng = np.random.default_rng(0)
    S, N = n_structs, n_structs * n_atoms
    offsets = np.arange(S + 1) * n_atoms
    side = (12.0 * n_atoms) ** (1 / 3)
    lat = np.stack([np.eye(3) * side] * S)
    pos = torch.tensor(rng.uniform(0, side, (N, 3)), device=dev)
    vel = torch.tensor(np.concatenate([maxwell_boltzmann(np.full(n_atoms, 63.546), 300.0, s) for s in range(S)]), device=dev)
    dyn = DynState(pos, None, offsets, np.full(N, 63.546), vel, 300.0, np.arange(S), ensemble="nve", dt=1.0)
    rn = RnemdState(offsets, lat, kind, 2, n_slabs, n_swaps, device=dev)
    f = torch.tensor(rng.normal(0, 0.5, (N, 3)).astype(np.float32), device=dev)
    step_us = events(lambda: dyn_step(dyn, f))
    dyn_step(dyn, f, finish_only=True)   # a synchronous point: the exchange is made and the profile sampled at every call
    exchange_us = events(lambda: rnemd_exchange(rn, dyn, pos))
    r = rn.read()
    print(json.dumps({"case": f"{S} x {n_atoms}", "kind": kind, "atoms": N, "n_slabs": n_slabs, "n_swaps": n_swaps,
                      "dyn_step_3_launches_us": round(step_us, 2), "rnemd_exchange_2_launches_us": round(exchange_us, 2),
                      "calls": int(r["n_calls"][0]), "pairs_exchanged": int(r["n_exchanged"].sum())}), flush=True)


def run_cost():
    model = build_model_from_npz(ROOT / "tests" / "golden" / "model_fitted_lj.npz").to(dev)
    base = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])
    gi = np.stack(np.meshgrid(np.arange(2), np.arange(2), np.arange(8), indexing="ij"), -1)
    pos = (gi.reshape(-1, 1, 3) + base[None]).reshape(-1, 3) * 3.35 + [0.0, 0.0, 0.25 * 3.35]
    lat, z = np.diag([2, 2, 8]) * 3.35, np.full(128, 29)
    out = {}
    for key, interval in (("nve_ms_per_step", 10 ** 9), ("rnemd_ms_per_step", 10)):
        md = ReverseNEMD(model, temperature=40.0, n_slabs=8, swap_interval=interval, sample_interval=interval, seed=0)
        fn = lambda n: md.run([lat], [pos], [z], n, loginterval=max(n, 1))
        fn(20)
        wall = []
        for n in (steps // 5, steps):   # the slope between two run lengths: set-up and the final copies cancel
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(n)
            torch.cuda.synchronize()
            wall.append(time.perf_counter() - t0)
        out[key] = round((wall[1] - wall[0]) / (steps - steps // 5) * 1e3, 4)
    out["extra_ms_per_step"] = round(out["rnemd_ms_per_step"] - out["nve_ms_per_step"], 4)
    print(json.dumps(dict({"case": "cu128 2x2x8, exchange and sample every 10 steps", "steps": steps}, **out)), flush=True)


launches(1, 128, 8, 1)
launches(1, 128, 64, 8)
launches(1, 10000, 8, 1)
launches(1, 10000, 64, 8)
launches(1, 10000, 20, 1, kind="momentum")
launches(64, 128, 8, 1)
run_cost()
