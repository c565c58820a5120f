#!/usr/bin/env python3
"""Per-iteration cost of batched FIRE relaxation (torch_m3gnet.relax): one relax iteration (VerletGraph.step + the FIRE launches) against
the bare VerletGraph.step on the same cells, for the 32-atom cell, a 256 x 32-atom batch and the 10,000-atom cell (10 x 10 x 25, bench
config3) with the cell fixed, and the variable-cell iteration (new cell -> host copy -> set_lattice -> candidate search) of the 32-atom
cell and the batch.  fmax is tiny so that nothing converges inside the timed loop.  Default model (bench.default_model).

    python tools/time_relax.py [iterations]
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
from torch_m3gnet.nn import Gradient  # noqa: E402
from torch_m3gnet.relax import FireState, fire_step  # noqa: E402

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 50
dev = torch.device("cuda")
model = Gradient(bench.default_model(dev).model, pair_virial=True)
base = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])


def fcc(nx, ny, nz, a=3.61, seed=0):
    gi = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1)
    pos = (gi.reshape(-1, 1, 3) + base[None]).reshape(-1, 3) * a
    return pos + np.random.default_rng(seed).normal(0, 0.03, pos.shape), np.diag([nx * a, ny * a, nz * a])


def case(name, cells, relax_cell):
    lats = [c[1] for c in cells]
    z = [np.full(len(c[0]), 29) for c in cells]
    offsets = np.concatenate([[0], np.cumsum([len(c[0]) for c in cells])])
    # bare step: the same cells, positions fixed
    vg = VerletGraph(lats, z, 5.0, 4.0, skin=0.5, device=dev)
    pos = torch.tensor(np.concatenate([c[0] for c in cells]), device=dev)
    for _ in range(3):
        vg.step(model, pos)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        vg.step(model, pos)
    torch.cuda.synchronize()
    bare = (time.perf_counter() - t0) / iters * 1e3
    # relax iterations
    vg = VerletGraph(lats, z, 5.0, 4.0, skin=0.5, device=dev)
    pos = torch.tensor(np.concatenate([c[0] for c in cells]), device=dev)
    lat64 = vg.lattice.clone()
    fire = FireState(pos, lat64, offsets, relax_cell=relax_cell, fmax=1e-9)

    def it():
        out = vg.step(model, pos)
        fire_step(fire, out[K.FORCES], out[K.STRESSES])
        if relax_cell:
            vg.set_lattice(list(lat64.cpu().numpy()))
        return fire.n_unconverged

    for _ in range(3):
        it()
    torch.cuda.synchronize()
    stats0 = dict(vg.stats)
    t0 = time.perf_counter()
    for _ in range(iters):
        it()
    torch.cuda.synchronize()
    relax = (time.perf_counter() - t0) / iters * 1e3
    paths = {k: vg.stats[k] - stats0.get(k, 0) for k in vg.stats}
    # FIRE launches alone (the same forces over and over), timed with events
    out = vg.step(model, pos)
    f, s = out[K.FORCES], out[K.STRESSES]
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(200):
        fire_step(fire, f, s)
    e1.record()
    torch.cuda.synchronize()
    fire_ms = e0.elapsed_time(e1) / 200
    print(json.dumps({"case": name, "atoms": int(offsets[-1]), "structures": len(cells), "relax_cell": relax_cell,
                      "bare_step_ms": round(bare, 4), "relax_iteration_ms": round(relax, 4), "fire_launches_ms": round(fire_ms, 4),
                      "paths_in_timed_relax_loop": paths, "iterations": iters}), flush=True)


c32 = [fcc(2, 2, 2, seed=0)]
batch = [fcc(2, 2, 2, seed=s) for s in range(256)]
case("cu32", c32, False)
case("cu32x256", batch, False)
case("cu10k", [fcc(10, 10, 25)], False)
case("cu32_cell", c32, True)
case("cu32x256_cell", batch, True)
