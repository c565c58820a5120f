#!/usr/bin/env python3
"""Per-iteration cost of batched FIRE relaxation (torch_m3gnet.relax): one relax iteration (VerletGraph.step + the FIRE launches) against
the bare VerletGraph.step on the same cells, for the 32-atom cell, a 256 x 32-atom batch and the 10,000-atom cell (10 x 10 x 25, bench
config3) with the cell fixed, and the variable-cell iteration (new cell -> host copy -> set_lattice -> candidate search) of the 32-atom
cell and the batch.  fmax is tiny so that nothing converges inside the timed loop.  Default model (bench.default_model).

    python tools/time_relax.py [iterations] [lbfgs]      ("lbfgs": the lbfgs_cases only)
Prints one JSON line per case.  Each case also times, with events around 200 back-to-back calls on the same forces, the FIRE launches
and the L-BFGS launches (memory 1 and 100, the ring full), and -- the
"lbfgs_cases" at the end -- the 10,000-atom cell and the 4,096 x 64-atom batch (BASELINE config 4): one energy/force step (events around `iterations`
VerletGraph.step calls at fixed positions) beside one m3g_fire_step and one m3g_lbfgs_step at history depth 1 and 100."""
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
from torch_m3gnet.relax import FireState, LbfgsState, fire_step, lbfgs_step  # noqa: E402

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 50
dev = torch.device("cuda")
model = Gradient(bench.default_model(dev).model, pair_virial=True)
base = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])


def fcc(nx, ny, nz, a=3.61, seed=0):
    gi = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1)
    pos = (gi.reshape(-1, 1, 3) + base[None]).reshape(-1, 3) * a
    return pos + np.random.default_rng(seed).normal(0, 0.03, pos.shape), np.diag([nx * a, ny * a, nz * a])


def events_ms(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def lbfgs_launches(cells, relax_cell, f, s):
    """{memory: ms} of one m3g_lbfgs_step with a full ring, memory 1 and 100: `memory` + 1 calls with seeded forces that differ from
    call to call fill the ring, then events around 200 calls on the same forces (the ring stays full whether a call's pair is stored
    or, with y = 0, not; every call runs all five kernels and moves the structures)."""
    offsets = np.concatenate([[0], np.cumsum([len(c[0]) for c in cells])])
    out = {}
    for memory in (1, 100):
        pos = torch.tensor(np.concatenate([c[0] for c in cells]), device=dev)
        lat = torch.tensor(np.stack([c[1] for c in cells]), device=dev)
        st = LbfgsState(pos, lat, offsets, relax_cell=relax_cell, fmax=1e-9, memory=memory)
        gen = torch.Generator(device=dev).manual_seed(0)
        for _ in range(memory + 2):
            lbfgs_step(st, f + 0.05 * torch.randn(f.shape, device=dev, generator=gen), s)
        depth = st.read()["n_pairs"]
        ms = events_ms(lambda: lbfgs_step(st, f, s), 200)
        r = st.read()
        out[f"memory_{memory}"] = {"ms": round(ms, 4), "depth_min_before": int(depth.min()), "depth_min_after": int(r["n_pairs"].min()),
                                   "failed_or_converged_structures": int((r["flags"] & 6 != 0).sum())}
    return out


def lbfgs_case(name, cells):
    """One optimiser step of each kind on seeded forces (they need no model), then one energy/force step of the same cells."""
    lats = [c[1] for c in cells]
    z = [np.full(len(c[0]), 29) for c in cells]
    offsets = np.concatenate([[0], np.cumsum([len(c[0]) for c in cells])])
    pos = torch.tensor(np.concatenate([c[0] for c in cells]), device=dev)
    lat = torch.tensor(np.stack(lats), device=dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    f = 0.1 * torch.randn((len(pos), 3), device=dev, generator=gen)
    s = 1e-3 * torch.randn((len(cells), 6), device=dev, generator=gen)
    fire = FireState(pos.clone(), lat.clone(), offsets, relax_cell=True, fmax=1e-9)
    fire_step(fire, f, s)
    fire_ms = events_ms(lambda: fire_step(fire, f, s), 200)
    res = {"lbfgs_case": name, "atoms": int(offsets[-1]), "structures": len(cells), "relax_cell": True, "memory": 100,
           "fire_step_ms": round(fire_ms, 4), "lbfgs_step_full_ring": lbfgs_launches(cells, True, f, s)}
    print(json.dumps(res), flush=True)
    vg = VerletGraph(lats, z, 5.0, 4.0, skin=0.5, device=dev)
    for _ in range(3):
        vg.step(model, pos)
    res["energy_force_step_ms"] = round(events_ms(lambda: vg.step(model, pos), iters), 4)
    print(json.dumps(res), flush=True)


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
    lbfgs_ms = lbfgs_launches(cells, relax_cell, f, s)
    print(json.dumps({"case": name, "atoms": int(offsets[-1]), "structures": len(cells), "relax_cell": relax_cell,
                      "bare_step_ms": round(bare, 4), "relax_iteration_ms": round(relax, 4), "fire_launches_ms": round(fire_ms, 4),
                      "lbfgs_launches_full_ring": lbfgs_ms,
                      "paths_in_timed_relax_loop": paths, "iterations": iters}), flush=True)


if "lbfgs" not in sys.argv[2:]:
    c32 = [fcc(2, 2, 2, seed=0)]
    batch = [fcc(2, 2, 2, seed=s) for s in range(256)]
    case("cu32", c32, False)
    case("cu32x256", batch, False)
    case("cu10k", [fcc(10, 10, 25)], False)
    case("cu32_cell", c32, True)
    case("cu32x256_cell", batch, True)
lbfgs_case("cu10k", [fcc(10, 10, 25)])
lbfgs_case("cu64x4096", [fcc(2, 2, 4, seed=s) for s in range(4096)])   # BASELINE config 4's structures, all on one GPU
