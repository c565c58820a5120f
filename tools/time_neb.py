#!/usr/bin/env python3
"""Per-iteration cost of the batched NEB (torch_m3gnet.neb): one NEB iteration (VerletGraph.step of every interior image + the NEB
projection + FIRE) against the bare VerletGraph.step on the same images, and the NEB and FIRE launches alone (device events), for
1 band x 5 interior images x 31 atoms, 16 bands x 5 x 107 atoms and 1 band x 5 x 4,000 atoms.  Rattled fcc Cu images along a
path that moves one atom; fmax is tiny so that nothing converges inside the timed loop.  Default model (bench.default_model).

    python tools/time_neb.py [iterations]
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
from torch_m3gnet.neb import NEBState, interpolate, neb_forces  # noqa: E402
from torch_m3gnet.nn import Gradient  # noqa: E402
from torch_m3gnet.relax import FireState, fire_step  # noqa: E402

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 50
dev = torch.device("cuda")
model = Gradient(bench.default_model(dev).model, pair_virial=True)
base = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])


def band(n, vacancy, seed, a=3.61, m=7):
    gi = np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij"), -1)
    sites = (gi.reshape(-1, 1, 3) + base[None]).reshape(-1, 3) * a
    lat = np.eye(3) * n * a
    init = sites[1:] if vacancy else sites.copy()
    init = init + np.random.default_rng(seed).normal(0, 0.03, init.shape)
    final = init.copy()
    final[0] = sites[0] if vacancy else final[0] + 0.5
    return lat, interpolate(lat, init, final, m)


def case(name, bands):
    img_lat = [lat for lat, imgs in bands for _ in imgs[1:-1]]
    img_pos = [p for _, imgs in bands for p in imgs[1:-1]]
    z = [np.full(len(p), 29) for p in img_pos]
    image_offsets = np.concatenate([[0], np.cumsum([len(p) for p in img_pos])])
    band_images = np.concatenate([[0], np.cumsum([len(imgs) - 2 for _, imgs in bands])])
    ep = torch.tensor(np.concatenate([p for _, imgs in bands for p in (imgs[0], imgs[-1])]), device=dev)
    # bare step: the same images, positions fixed
    vg = VerletGraph(img_lat, z, 5.0, 4.0, skin=0.5, device=dev)
    pos = torch.tensor(np.concatenate(img_pos), device=dev)
    for _ in range(3):
        vg.step(model, pos)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        vg.step(model, pos)
    torch.cuda.synchronize()
    bare = (time.perf_counter() - t0) / iters * 1e3
    # NEB iterations
    vg = VerletGraph(img_lat, z, 5.0, 4.0, skin=0.5, device=dev)
    pos = torch.tensor(np.concatenate(img_pos), device=dev)
    neb = NEBState(image_offsets, band_images, 0.1, True, ep, np.zeros((len(bands), 2)))
    fire = FireState(pos, None, neb.band_offsets, relax_cell=False, fmax=1e-9)

    def it():
        out = vg.step(model, pos)
        neb_forces(neb, pos, out[K.TOTAL_ENERGY], out[K.FORCES])
        fire_step(fire, neb.forces)
        return fire.n_unconverged

    for _ in range(3):
        it()
    torch.cuda.synchronize()
    stats0 = dict(vg.stats)
    t0 = time.perf_counter()
    for _ in range(iters):
        it()
    torch.cuda.synchronize()
    neb_ms = (time.perf_counter() - t0) / iters * 1e3
    paths = {k: vg.stats[k] - stats0.get(k, 0) for k in vg.stats}
    # the NEB projection and the FIRE launches alone (the same evaluation over and over), timed with events
    out = vg.step(model, pos)
    e, f = out[K.TOTAL_ENERGY], out[K.FORCES]
    torch.cuda.synchronize()
    times = {}
    for what, fn in (("neb_launches_ms", lambda: neb_forces(neb, pos, e, f)), ("fire_launches_ms", lambda: fire_step(fire, neb.forces))):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(200):
            fn()
        e1.record()
        torch.cuda.synchronize()
        times[what] = round(e0.elapsed_time(e1) / 200, 4)
    print(json.dumps({"case": name, "bands": len(bands), "images": len(img_pos), "atoms": int(image_offsets[-1]),
                      "bare_step_ms": round(bare, 4), "neb_iteration_ms": round(neb_ms, 4), **times,
                      "paths_in_timed_neb_loop": paths, "iterations": iters}), flush=True)


case("1x5x31", [band(2, True, 0)])
case("16x5x107", [band(3, True, s) for s in range(16)])
case("1x5x4000", [band(10, False, 0)])
