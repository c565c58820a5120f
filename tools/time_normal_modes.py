#!/usr/bin/env python3
"""Cost of the normal-mode projection (torch_m3gnet.normal_modes): the device time of the three m3g_nma_sample launches beside the three
m3g_dyn_step launches (synthetic forces and velocities, random unitary eigenvectors, 200 calls back to back, CUDA events) for one fcc
supercell of 32, 256 and 2,048 atoms (conventional cell, n_u = 4: (2,2,2), (4,4,4), (8,8,8)) with ALL commensurate q-points (8, 64,
512) at 0, 100 and 1,000 lags, for a unit cell of 21 atoms (3 n_u = 63, the largest eigenvector matrices) in (4,4,2), and for 64
structures of 32 atoms.

    python tools/time_normal_modes.py
Prints one JSON line per case."""
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "torch-m3gnet_amd"):
    sys.path.insert(0, str(p))
from torch_m3gnet.dynamics import DynState, dyn_step, maxwell_boltzmann  # noqa: E402
from torch_m3gnet.normal_modes import NmaState, commensurate_qpoints, nma_sample  # noqa: E402

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


def unitary(rng, n):
    q, _ = np.linalg.qr(rng.normal(size=(n, n)) + 1j * rng.normal(size=(n, n)))
    return q


def launches(n_structs, n_unit, supercell, n_lags):
    rng = np.random.default_rng(0)
    cells = int(np.prod(supercell))
    n = n_unit * cells
    S, N = n_structs, n_structs * n
    lattice = np.eye(3) * 3.6 * (n_unit / 4) ** (1 / 3)
    frac = rng.uniform(0, 1, (n_unit, 3))
    q = commensurate_qpoints(supercell)
    eig = np.stack([unitary(rng, 3 * n_unit) for _ in q])
    masses = np.full(n_unit, 63.546)
    state = NmaState([lattice] * S, [frac] * S, [masses] * S, [supercell] * S, [q] * S, [eig] * S, n_lags, device=dev)
    grid = np.stack(np.meshgrid(*(np.arange(c) for c in supercell), indexing="ij"), -1).reshape(-1, 1, 3)
    sites = np.tile(((frac[None] + grid).reshape(-1, 3)) @ lattice, (S, 1))
    pos = torch.tensor(sites + rng.normal(0, 0.05, sites.shape), device=dev)
    vel = torch.tensor(np.concatenate([maxwell_boltzmann(np.full(n, 63.546), 300.0, s) for s in range(S)]), device=dev)
    offsets = np.arange(S + 1) * n
    dyn = DynState(pos.clone(), None, offsets, np.full(N, 63.546), vel, 300.0, np.arange(S), ensemble="nve", dt=1.0)
    f = torch.tensor(rng.normal(0, 0.5, (N, 3)).astype(np.float32), device=dev)
    step_us = events(lambda: dyn_step(dyn, f))
    sample_us = events(lambda: nma_sample(state, pos, vel, f, 0.5))
    r = state.read()
    print(json.dumps({"case": f"{S} x {n}", "atoms": N, "n_unit": n_unit, "supercell": list(supercell), "q_per_structure": len(q),
                      "modes": state.M, "n_lags": n_lags, "state_MB": round(state.state.numel() / 2 ** 20, 2),
                      "dyn_step_3_launches_us": round(step_us, 2), "nma_sample_3_launches_us": round(sample_us, 2),
                      "samples": int(r["n_samples"][0]), "flags": int(r["flags"].max())}), flush=True)


for sc in ((2, 2, 2), (4, 4, 4), (8, 8, 8)):
    for lags in (0, 100, 1000):
        launches(1, 4, sc, lags)
launches(1, 21, (4, 4, 2), 100)
launches(64, 4, (2, 2, 2), 100)
