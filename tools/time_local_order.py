#!/usr/bin/env python3
"""Timing of the local-order observables (profiles/local_order.txt).

    python tools/time_local_order.py sample NX NY NZ [REPS]      back-to-back lo_sample calls on one fcc Cu cell of NX x NY x NZ cells
                                                                 (a = 3.61 A, thermal displacements; 4 4 4: 256 atoms, 10 10 25: the
                                                                 10,000-atom cell of bench.py), r_cut = 3.1 A, degrees (4, 6):
                                                                 CUDA-event time per sample; under `rocprofv3 --kernel-trace --stats
                                                                 -- ...` the time of each launch
    python tools/time_local_order.py md NX NY NZ none|lo [EVERY]  ms per MD step (Langevin, the same cell) without observables or with
                                                                 LocalOrderObservables(sample_interval = EVERY, default 1)
"""
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "torch-m3gnet_amd"))
sys.path.insert(0, str(ROOT))
R_CUT, DEGREES = 3.1, (4, 6)


def cell(shape):
    from torch_m3gnet.data.synthetic import fcc_cu_arrays

    lat, pos, z = fcc_cu_arrays(*shape, jitter=0.0)
    return np.asarray(lat, dtype=np.float64), np.asarray(pos, dtype=np.float64) + np.random.default_rng(0).normal(0, 0.08, np.shape(pos)), np.asarray(z)


def sample(argv):
    import torch

    from torch_m3gnet.local_order import LoState, lo_sample

    shape = tuple(int(x) for x in argv[:3])
    reps = int(argv[3]) if len(argv) > 3 else 200
    lat0, pos0, _ = cell(shape)
    n = len(pos0)
    lat, pos = torch.tensor(lat0[None], device="cuda"), torch.tensor(pos0, device="cuda")
    st = LoState(n, [0, n], np.zeros(n, np.int32), [R_CUT], DEGREES)
    for _ in range(5):
        lo_sample(st, pos, lat)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(5):
        e0.record()
        for _ in range(reps):
            lo_sample(st, pos, lat)
        e1.record()
        torch.cuda.synchronize()
        times.append(round(e0.elapsed_time(e1) / reps * 1e3, 2))
    acc, fr = st.read(), st.frame()
    print(json.dumps(dict(atoms=n, reps=reps, sample_us=times, state_bytes=st.state.numel(), flags=int(acc["flags"][0]),
                          n_samples=int(acc["n_samples"][0]), mean_neighbors=float(fr["n_neighbors"].mean()),
                          mean_q6=float(fr["ql"][:, 1].mean()), n_solid=int(fr["solid"].sum()))))


def md(argv):
    import torch

    from torch_m3gnet.dynamics import MolecularDynamics
    from torch_m3gnet.local_order import LocalOrderObservables
    from torch_m3gnet.model.build import build_model_from_npz

    shape, mode = tuple(int(x) for x in argv[:3]), argv[3]
    every = int(argv[4]) if len(argv) > 4 else 1
    model = build_model_from_npz(ROOT / "tests" / "golden" / "model_fitted_lj.npz").to("cuda")
    lat, pos, z = cell(shape)
    run = MolecularDynamics(model, ensemble="nvt_langevin", timestep=2.0, temperature=300.0, friction=0.02, seed=0).run
    obs = {"none": None, "lo": LocalOrderObservables(R_CUT, DEGREES, sample_interval=every)}[mode]
    short, long = (60, 260) if len(pos) <= 1000 else (10, 50)
    times = {}
    for steps in (short, short, long, short, long):   # the first run warms up; per step from the difference of a long and a short run
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run([lat], [pos], [z], steps, loginterval=50, observables=obs)
        torch.cuda.synchronize()
        times.setdefault(steps, []).append(time.perf_counter() - t0)
    per_step = [round((b - a) / (long - short) * 1e3, 4) for a, b in zip(times[short][1:], times[long])]
    print(json.dumps(dict(mode=mode, atoms=len(pos), sample_interval=every, ms_per_step=per_step)))


if __name__ == "__main__":
    {"sample": sample, "md": md}[sys.argv[1]](sys.argv[2:])
