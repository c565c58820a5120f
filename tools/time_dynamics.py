#!/usr/bin/env python3
"""Per-step cost of batched molecular dynamics (torch_m3gnet.dynamics): one MolecularDynamics step (VerletGraph.step + the three
m3g_dyn_step launches, Langevin at 300 K, no log step) against the bare VerletGraph.step at fixed positions and against the torch-op
velocity-Verlet loop of examples/md_nve.py (VerletGraph.step + ~ten elementwise launches and two copies), for the 32-atom cell, a
256 x 32-atom batch and the 10,000-atom cell (10 x 10 x 25, bench config3), plus the three launches alone.  Default model
(bench.default_model), pair-virial engine in all three loops.

    python tools/time_dynamics.py [steps]
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
import bench  # noqa: E402
from torch_m3gnet.data import MaterialGraphKey as K  # noqa: E402
from torch_m3gnet.data.md import VerletGraph  # noqa: E402
from torch_m3gnet.dynamics import KAPPA, DynState, dyn_step, maxwell_boltzmann  # noqa: E402
from torch_m3gnet.nn import Gradient  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
dev = torch.device("cuda")
model = Gradient(bench.default_model(dev).model, pair_virial=True)
base = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])
MASS, DT = 63.546, 1.0


def fcc(nx, ny, nz, a=3.61, seed=0):
    gi = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1)
    pos = (gi.reshape(-1, 1, 3) + base[None]).reshape(-1, 3) * a
    return pos + np.random.default_rng(seed).normal(0, 0.03, pos.shape), np.diag([nx * a, ny * a, nz * a])


def timed(fn, n):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def case(name, cells):
    lats = [c[1] for c in cells]
    z = [np.full(len(c[0]), 29) for c in cells]
    offsets = np.concatenate([[0], np.cumsum([len(c[0]) for c in cells])])
    n = int(offsets[-1])
    pos0 = np.concatenate([c[0] for c in cells])
    vel0 = np.concatenate([maxwell_boltzmann(np.full(len(c[0]), MASS), 300.0, s) for s, c in enumerate(cells)])
    # bare step: positions fixed
    vg = VerletGraph(lats, z, 5.0, 4.0, skin=0.5, device=dev)
    pos = torch.tensor(pos0, device=dev)
    bare = timed(lambda: vg.step(model, pos), steps)
    # MolecularDynamics' loop: vg.step + dyn_step
    vg = VerletGraph(lats, z, 5.0, 4.0, skin=0.5, device=dev)
    pos = torch.tensor(pos0, device=dev)
    lat64 = vg.lattice.clone()
    dyn = DynState(pos, lat64, offsets, np.full(n, MASS), torch.tensor(vel0, device=dev), 300.0, np.arange(len(cells)), ensemble="nvt_langevin",
                   dt=DT, friction=0.01)

    def md_it():
        out = vg.step(model, pos)
        dyn_step(dyn, out[K.FORCES], out[K.STRESSES])

    stats0 = dict(vg.stats)
    md = timed(md_it, steps)
    paths = {k: vg.stats[k] - stats0.get(k, 0) for k in vg.stats}
    # the torch-op loop of examples/md_nve.py
    vg = VerletGraph(lats, z, 5.0, 4.0, skin=0.5, device=dev)
    state = {"pos": torch.tensor(pos0, device=dev), "vel": torch.tensor(vel0, device=dev)}
    state["f"] = vg.step(model, state["pos"])[K.FORCES].double().clone()

    def torch_it():
        state["vel"] = state["vel"] + 0.5 * DT * KAPPA / MASS * state["f"]
        state["pos"] = state["pos"] + DT * state["vel"]
        out = vg.step(model, state["pos"])
        state["f"] = out[K.FORCES].double().clone()
        state["vel"] = state["vel"] + 0.5 * DT * KAPPA / MASS * state["f"]

    torch_ms = timed(torch_it, steps)
    # the three launches alone (the same forces over and over), timed with events
    out = vg.step(model, state["pos"])
    f, s = out[K.FORCES], out[K.STRESSES]
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(200):
        dyn_step(dyn, f, s)
    e1.record()
    torch.cuda.synchronize()
    print(json.dumps({"case": name, "atoms": n, "structures": len(cells), "bare_step_ms": round(bare, 4), "md_step_ms": round(md, 4),
                      "torch_op_step_ms": round(torch_ms, 4), "dyn_launches_ms": round(e0.elapsed_time(e1) / 200, 4),
                      "paths_in_timed_md_loop": paths, "steps": steps}), flush=True)


case("cu32", [fcc(2, 2, 2, seed=0)])
case("cu32x256", [fcc(2, 2, 2, seed=s) for s in range(256)])
case("cu10k", [fcc(10, 10, 25)])
