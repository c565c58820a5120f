#!/usr/bin/env python3
"""Timing of the trajectory observables (profiles/trajectory.txt).

    python tools/time_trajectory.py sample S ATOMS N_LAGS [REPS]   back-to-back traj_sample calls on S structures of ATOMS atoms, rdf_bins =
                                                                    200, ring full: CUDA-event time per sample; under
                                                                    `rocprofv3 --kernel-trace --stats -- ...` the time of each launch
    python tools/time_trajectory.py md TREE none|obs               ms per MD step (Langevin, 256 and 10,000 Cu atoms) of the checkout at
                                                                    TREE, without observables or with sample_interval = 1: run it on
                                                                    a checkout of the parent commit (none) for the baseline
"""
import json
import sys
import time
from pathlib import Path

import numpy as np


def sample(argv):
    import torch

    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "torch-m3gnet_amd"))
    from torch_m3gnet.trajectory import TrajState, traj_sample

    S, n, G = int(argv[0]), int(argv[1]), int(argv[2])
    reps = int(argv[3]) if len(argv) > 3 else 50
    rng = np.random.default_rng(0)
    N = S * n
    side = (12.0 * n) ** (1 / 3)
    lat = torch.tensor(np.stack([np.eye(3) * side] * S), device="cuda")
    pos = torch.tensor(rng.uniform(0, side, (N, 3)), device="cuda")
    vel = torch.tensor(rng.normal(0, 0.01, (N, 3)), device="cuda")
    f = torch.tensor(rng.normal(0, 0.5, (N, 3)).astype(np.float32), device="cuda")
    st = TrajState(N, np.arange(S + 1) * n, rng.integers(0, 2, N), np.full(N, 63.5), side / 2 * 0.999, 200, G, True, max_species=2)
    for _ in range(G + 5):   # fill the ring: every later sample reads all of it
        traj_sample(st, pos, lat, vel, f, 1.0)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        traj_sample(st, pos, lat, vel, f, 1.0)
    e1.record()
    torch.cuda.synchronize()
    print(json.dumps(dict(n_structs=S, atoms=n, n_lags=G, reps=reps, sample_ms=e0.elapsed_time(e1) / reps,
                          ring_bytes_read_per_sample=(G + 1) * N * 48)))


def md(argv):
    tree, mode = Path(argv[0]).resolve(), argv[1]
    sys.path.insert(0, str(tree / "torch-m3gnet_amd"))
    sys.path.insert(0, str(tree))
    import torch
    from torch_m3gnet.dynamics import MolecularDynamics
    from torch_m3gnet.model.build import build_model_from_npz

    model = build_model_from_npz(tree / "tests" / "golden" / "model_fitted_lj.npz").to("cuda")
    base = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])
    for shape, lags in (((4, 4, 4), 64), ((10, 10, 25), 64), ((10, 10, 25), 512)):
        gi = np.stack(np.meshgrid(*[np.arange(k) for k in shape], indexing="ij"), -1)
        pos, lat = (gi.reshape(-1, 1, 3) + base[None]).reshape(-1, 3) * 3.61, np.diag(shape) * 3.61
        z = np.full(len(pos), 29)
        run = MolecularDynamics(model, ensemble="nvt_langevin", timestep=2.0, temperature=300.0, friction=0.02, seed=0).run
        kw = {}
        if mode == "obs":
            from torch_m3gnet.trajectory import TrajectoryObservables
            kw["observables"] = TrajectoryObservables(rdf_bins=200, n_lags=lags, sample_interval=1)
        times = {}
        for steps in (20, 60, 260, 60, 260):   # the first run warms up; per step from the difference of a long and a short run
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run([lat], [pos], [z], steps, loginterval=50, **kw)
            torch.cuda.synchronize()
            times.setdefault(steps, []).append(time.perf_counter() - t0)
        per_step = [round((b - a) / 200 * 1e3, 4) for a, b in zip(times[60], times[260])]
        print(json.dumps(dict(tree=tree.name, mode=mode, atoms=len(pos), n_lags=lags if mode == "obs" else None, ms_per_step=per_step)))


if __name__ == "__main__":
    {"sample": sample, "md": md}[sys.argv[1]](sys.argv[2:])
