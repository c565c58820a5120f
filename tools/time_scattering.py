#!/usr/bin/env python3
"""Timing of the scattering observables (profiles/scattering.txt).

    python tools/time_scattering.py sample S [REPS]   back-to-back sq_sample calls on S copies of the 256-atom Cu cell (fcc 4 x 4 x 4,
                                                      a = 3.61 A, thermal displacements), q_max = 3.0 1/A thinned to 32 per shell (302
                                                      vectors per structure), n_lags = 256, remove_com, ring full: CUDA-event time
                                                      per sample; under `rocprofv3 --kernel-trace --stats -- ...` the time of each launch
    python tools/time_scattering.py md none|sq|both   ms per MD step (Langevin, the same cell) without observables, with
                                                      ScatteringObservables(sample_interval = 1), or with both kinds of observables
(the rate of the sampler's fp64 sincospi: tools/sincospi_rate.hip)
"""
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "torch-m3gnet_amd"))
sys.path.insert(0, str(ROOT))
A, SHAPE, Q_MAX, PER_SHELL, N_LAGS = 3.61, (4, 4, 4), 3.0, 32, 256
BASE = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])


def cell():
    gi = np.stack(np.meshgrid(*[np.arange(k) for k in SHAPE], indexing="ij"), -1)
    return (gi.reshape(-1, 1, 3) + BASE[None]).reshape(-1, 3) * A, np.diag(SHAPE) * A


def sample(argv):
    import torch

    from torch_m3gnet.scattering import SqState, q_vectors, sq_sample

    S = int(argv[0])
    reps = int(argv[1]) if len(argv) > 1 else 200
    rng = np.random.default_rng(0)
    pos0, lat0 = cell()
    n = len(pos0)
    hkl = q_vectors(lat0, Q_MAX, PER_SHELL)
    lat = torch.tensor(np.stack([lat0] * S), device="cuda")
    pos = torch.tensor(np.concatenate([pos0 + rng.normal(0, 0.08, pos0.shape) for _ in range(S)]), device="cuda")
    vel = torch.tensor(rng.normal(0, 0.003, (S * n, 3)), device="cuda")
    f = torch.tensor(rng.normal(0, 0.5, (S * n, 3)).astype(np.float32), device="cuda")
    st = SqState(S * n, np.arange(S + 1) * n, np.zeros(S * n, np.int32), np.full(S * n, 63.546), [hkl] * S, N_LAGS, True)
    for _ in range(N_LAGS + 5):   # fill the ring: every later sample reads all of it
        sq_sample(st, pos, lat, vel, f, 1.0)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(5):
        e0.record()
        for _ in range(reps):
            sq_sample(st, pos, lat, vel, f, 1.0)
        e1.record()
        torch.cuda.synchronize()
        times.append(round(e0.elapsed_time(e1) / reps * 1e3, 2))
    print(json.dumps(dict(n_structs=S, atoms=n, q_per_struct=len(hkl), n_lags=N_LAGS, reps=reps, sample_us=times,
                          sincospi_per_sample=S * n * len(hkl), state_bytes=st.state.numel())))


def md(argv):
    import torch

    from torch_m3gnet.dynamics import MolecularDynamics
    from torch_m3gnet.model.build import build_model_from_npz
    from torch_m3gnet.scattering import ScatteringObservables
    from torch_m3gnet.trajectory import TrajectoryObservables

    mode = argv[0]
    model = build_model_from_npz(ROOT / "tests" / "golden" / "model_fitted_lj.npz").to("cuda")
    pos, lat = cell()
    z = np.full(len(pos), 29)
    run = MolecularDynamics(model, ensemble="nvt_langevin", timestep=2.0, temperature=300.0, friction=0.02, seed=0).run
    sq = ScatteringObservables(q_max=Q_MAX, n_lags=N_LAGS, sample_interval=1, max_per_shell=PER_SHELL)
    traj = TrajectoryObservables(rdf_bins=200, n_lags=64, sample_interval=1)
    obs = {"none": None, "sq": sq, "both": [traj, sq]}[mode]
    times = {}
    for steps in (20, 60, 260, 60, 260):   # the first run warms up; per step from the difference of a long and a short run
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run([lat], [pos], [z], steps, loginterval=50, observables=obs)
        torch.cuda.synchronize()
        times.setdefault(steps, []).append(time.perf_counter() - t0)
    per_step = [round((b - a) / 200 * 1e3, 4) for a, b in zip(times[60], times[260])]
    print(json.dumps(dict(mode=mode, atoms=len(pos), ms_per_step=per_step)))


if __name__ == "__main__":
    {"sample": sample, "md": md}[sys.argv[1]](sys.argv[2:])
