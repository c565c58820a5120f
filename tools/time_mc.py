#!/usr/bin/env python3
"""Cost of batched atom-swap Monte Carlo (torch_m3gnet.monte_carlo): the device time of m3g_mc_propose + m3g_mc_decide, tracking
energies only (two launches: pure lattice Monte Carlo) and with forces and stresses (three: hybrid runs), on synthetic energies --
1,000 calls back to back between two device events -- for the three sizes of profiles/dynamics.txt: 1 x 32, 256 x 32 and 1 x 10,000
atoms (two species, half and half); beside it the yardstick this change does not touch, the bare VerletGraph.step of the same batch
without and with forces (default model, host clock around a loop that ends in a synchronise: the step waits for its skin test, so
events would time the same thing); and the trials per second, summed over the batch, of a SwapMonteCarlo run (pure, one engine call
per trial) at S = 1 and S = 256, from the slope between two run lengths.

    python tools/time_mc.py [trials]
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
from torch_m3gnet.data.md import VerletGraph  # noqa: E402
from torch_m3gnet.monte_carlo import McState, SwapMonteCarlo, mc_decide, mc_propose  # noqa: E402
from torch_m3gnet.nn import Gradient  # noqa: E402

trials = int(sys.argv[1]) if len(sys.argv) > 1 else 500
dev = torch.device("cuda")
model = Gradient(bench.default_model(dev).model, pair_virial=True)
base = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])
CALLS = 1000


def fcc(nx, ny, nz, a=3.9, seed=0):
    gi = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1)
    pos = (gi.reshape(-1, 1, 3) + base[None]).reshape(-1, 3) * a
    rng = np.random.default_rng(seed)
    z = rng.permutation(np.repeat([29, 79], len(pos) // 2))
    return pos + rng.normal(0, 0.03, pos.shape), np.diag([nx * a, ny * a, nz * a]), z


def events(fn):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(CALLS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / CALLS * 1e3   # us


def wall(fn, n):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e6   # us


def case(name, cells, run_too):
    S = len(cells)
    offsets = np.concatenate([[0], np.cumsum([len(c[0]) for c in cells])])
    N = int(offsets[-1])
    rng = np.random.default_rng(1)
    f32 = lambda x: torch.tensor(np.asarray(x, dtype=np.float32), device=dev)
    types = torch.tensor(np.concatenate([c[2] for c in cells]) - 1, dtype=torch.int64, device=dev)
    mc = McState(offsets, 600.0, np.arange(S), np.ones(N, bool), device=dev)
    # the trial energies stay fixed: after a structure's first acceptance dE = 0 and every trial is accepted, so every call runs the
    # dearer branch of k_mc_commit (the row copy); a rejection instead exchanges two rows back, as the proposal did
    e, e_trial = f32(np.full(S, -1.0)), f32(rng.normal(-1.0, 0.05, S))
    f, f_trial, s, s_trial = f32(np.zeros((N, 3))), f32(rng.normal(0, 0.5, (N, 3))), f32(np.zeros((S, 6))), f32(rng.normal(0, 0.01, (S, 6)))

    def energies_only():
        mc_propose(mc, types, e)
        mc_decide(mc, types, e_trial, e)

    def with_forces():
        mc_propose(mc, types, e)
        mc_decide(mc, types, e_trial, e, f_trial, f, s_trial, s)

    out = {"case": name, "atoms": N, "structures": S, "propose_decide_2_launches_us": round(events(energies_only), 2)}
    r0 = mc.read()
    out["propose_decide_with_forces_3_launches_us"] = round(events(with_forces), 2)
    r = mc.read()
    out["acceptance_in_timed_calls"] = round(float((r["accepts"] - r0["accepts"]).sum() / max((r["attempts"] - r0["attempts"]).sum(), 1)), 3)
    lats, zs = [c[1] for c in cells], [c[2] for c in cells]
    pos = torch.tensor(np.concatenate([c[0] for c in cells]), device=dev)
    vg = VerletGraph(lats, zs, 5.0, 4.0, skin=0.5, device=dev)
    n = max(trials // 5, 20)
    out["bare_step_energy_only_us"] = round(wall(lambda: vg.step(model, pos, forces=False), n), 1)
    out["bare_step_with_forces_us"] = round(wall(lambda: vg.step(model, pos), n), 1)
    if run_too:
        driver = SwapMonteCarlo(model, 600.0, seed=0)
        run = lambda k: driver.run(lats, [c[0] for c in cells], zs, k, loginterval=max(k, 1))
        run(10)
        t = []
        for k in (trials // 5, trials):   # the slope between two run lengths: set-up and the final copies cancel
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = run(k)
            torch.cuda.synchronize()
            t.append(time.perf_counter() - t0)
        per_trial = (t[1] - t[0]) / (trials - trials // 5)
        out.update(run_us_per_trial=round(per_trial * 1e6, 1), run_trials_per_s_over_the_batch=round(S / per_trial, 1),
                   run_acceptance=round(float(np.mean([x["acceptance"] for x in res])), 3), run_trials=trials)
    print(json.dumps(out), flush=True)


case("cu16au16", [fcc(2, 2, 2)], True)
case("cu16au16 x 256", [fcc(2, 2, 2, seed=s) for s in range(256)], True)
case("cu5k au5k", [fcc(10, 10, 25)], False)
