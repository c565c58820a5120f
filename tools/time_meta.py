#!/usr/bin/env python3
"""Cost of collective-variable biasing (torch_m3gnet.metadynamics): the device time of the three m3g_meta_bias launches beside the
three m3g_dyn_step launches (Langevin; synthetic forces, 200 calls back to back, device events) for one structure of 32, 864 and
10,000 atoms, with a DISTANCE CV over the whole structure (half the atoms in A, half in B) and, at 32 and 864 atoms, a COORDINATION CV
with |A| = |B| = the whole structure, under 0, 1,000 and 10,000 hills; and the per-step cost of a Metadynamics run of the 32-atom Cu
cell with four walkers against MolecularDynamics on the same cell (LJ-fitted fixture model, no log steps).

    python tools/time_meta.py [steps]
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
from torch_m3gnet.metadynamics import BiasState, Metadynamics, bias_forces, coordination, distance, projection  # noqa: E402
from torch_m3gnet.model.build import build_model_from_npz  # noqa: E402

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


def launches(n_atoms, kind, n_hills):
    rng = np.random.default_rng(0)
    N = n_atoms
    offsets = np.array([0, N])
    side = (12.0 * N) ** (1 / 3)     # the density of copper
    lat = np.eye(3)[None] * side
    pos = torch.tensor(rng.uniform(0, side, (N, 3)), device=dev)
    m = np.full(N, 63.546)
    dyn = DynState(pos.clone(), None, offsets, m, torch.tensor(maxwell_boltzmann(m, 300.0, 0), device=dev), 300.0, np.arange(1),
                   ensemble="nvt_langevin", dt=1.0, friction=0.01)
    everyone = list(range(N))
    cv = distance(everyone[:N // 2], everyone[N // 2:]) if kind == "distance" else coordination(everyone, everyone, 2.5, 3, min(4.0, 0.49 * side))
    bias = BiasState(offsets, lat, [cv], m, [0.1], height=0.01, inv_kdt=5.0, max_hills=max(n_hills, 1), device=dev)
    if n_hills:
        bias.set_hills([rng.normal(0.0, 1.0, (n_hills, 1))], [rng.uniform(0.001, 0.01, n_hills)])
    f = torch.tensor(rng.normal(0, 0.5, (N, 3)).astype(np.float32), device=dev)
    step_us = events(lambda: dyn_step(dyn, f))
    bias_us = events(lambda: bias_forces(bias, pos, f))
    print(json.dumps({"atoms": N, "cv": kind, "hills": n_hills, "dyn_step_3_launches_us": round(step_us, 2),
                      "meta_bias_3_launches_us": round(bias_us, 2), "cv_value": float(bias.obs[0, 0])}), flush=True)


def run_cost():
    model = build_model_from_npz(ROOT / "tests" / "golden" / "model_fitted_lj.npz").to(dev)
    base = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])
    gi = np.stack(np.meshgrid(np.arange(2), np.arange(2), np.arange(2), indexing="ij"), -1)
    pos = (gi.reshape(-1, 1, 3) + base[None]).reshape(-1, 3) * 3.35
    lat, z = np.eye(3) * 2 * 3.35, np.full(32, 29)
    cv = projection([0], list(range(1, 32)), [1.0, 1.0, 0.0])
    meta = Metadynamics(model, cv, 300.0, height=0.01, sigma=[0.05], pace=10, bias_factor=8.0, walkers=4, timestep=2.0, seed=0)
    md = MolecularDynamics(model, "nvt_langevin", timestep=2.0, temperature=300.0, seed=0)
    out = {}
    for key, fn in (("md_4_structures_ms_per_step", lambda n: md.run([lat] * 4, [pos] * 4, [z] * 4, n, loginterval=max(n, 1))),
                    ("metadynamics_4_walkers_ms_per_step", lambda n: meta.run([lat], [pos], [z], n, loginterval=max(n, 1)))):
        fn(20)
        wall = []
        for n in (steps // 5, steps):   # the slope between two run lengths: set-up and the final copies cancel
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(n)
            torch.cuda.synchronize()
            wall.append(time.perf_counter() - t0)
        out[key] = round((wall[1] - wall[0]) / (steps - steps // 5) * 1e3, 4)
    out["extra_ms_per_step"] = round(out["metadynamics_4_walkers_ms_per_step"] - out["md_4_structures_ms_per_step"], 4)
    print(json.dumps(dict({"case": "cu32 x 4 walkers, a hill from every walker every 10 steps", "steps": steps}, **out)), flush=True)


for n_atoms in (32, 864, 10000):
    for hills in (0, 1000, 10000):
        launches(n_atoms, "distance", hills)
for n_atoms in (32, 864):
    for hills in (0, 1000):
        launches(n_atoms, "coordination", hills)
run_cost()
