#!/usr/bin/env python3
"""Timing of the thermo observables (profiles/thermo.txt).

    python tools/time_thermo.py sample NX NY NZ [REPS] [N_LAGS]   back-to-back mode-(a) thermo_sample calls on one fcc Cu cell of NX x
                                                                 NY x NZ cells (10 10 25: the 10,000-atom cell of bench.py) with
                                                                 random velocities and forces, kicked, and beside them, alternating
                                                                 in the same process, a velocity-only traj_sample (rdf_bins = 0,
                                                                 n_lags = 4) on the same atoms, which reads the same velocities and
                                                                 forces once: CUDA-event time per sample of either, five windows
                                                                 each; under `rocprofv3 --kernel-trace --stats -- ...` the time of
                                                                 each launch
"""
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "torch-m3gnet_amd"))
sys.path.insert(0, str(ROOT))


def sample(argv):
    import torch

    from torch_m3gnet.data.synthetic import fcc_cu_arrays
    from torch_m3gnet.thermo import ThermoState, thermo_sample
    from torch_m3gnet.trajectory import TrajState, traj_sample

    shape = tuple(int(x) for x in argv[:3])
    reps = int(argv[3]) if len(argv) > 3 else 500
    lags = int(argv[4]) if len(argv) > 4 else 64
    lat0, pos0, _ = fcc_cu_arrays(*shape, jitter=0.0)
    lat0, pos0 = np.asarray(lat0, dtype=np.float64), np.asarray(pos0, dtype=np.float64)
    n = len(pos0)
    rng = np.random.default_rng(0)
    dev = lambda x: torch.tensor(x, device="cuda")
    lat, pos, vel = dev(lat0[None]), dev(pos0), dev(rng.normal(0, 0.004, (n, 3)))
    forces, energies = dev(rng.normal(0, 1.0, (n, 3)).astype(np.float32)), dev(np.array([-3.5 * n], np.float32))
    stresses = dev(rng.normal(0, 0.01, (1, 6)).astype(np.float32))
    masses = np.full(n, 63.546)
    th = ThermoState(n, [0, n], masses, [0.0], lat0[None], n_lags=lags, remove_com=True)
    tr = TrajState(n, [0, n], np.zeros(n, np.int32), masses, rdf_bins=0, n_lags=4, remove_com=True)
    calls = {"thermo": lambda: thermo_sample(th, energies, stresses, lat, vel, forces, 0.5),
             "traj": lambda: traj_sample(tr, pos, None, vel, forces, 0.5)}
    for call in calls.values():
        for _ in range(10):
            call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {name: [] for name in calls}
    for _ in range(5):   # alternating: either sees the same machine
        for name, call in calls.items():
            e0.record()
            for _ in range(reps):
                call()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(round(e0.elapsed_time(e1) / reps * 1e3, 2))
    acc = th.read()
    print(json.dumps(dict(atoms=n, reps=reps, thermo_n_lags=lags, thermo_sample_us=times["thermo"], traj_sample_us=times["traj"],
                          thermo_state_bytes=th.state.numel(), traj_state_bytes=tr.state.numel(), n_samples=int(acc["n_samples"][0]),
                          flags=int(acc["flags"][0]), ke=float(acc["mean"][0, 1]))))


if __name__ == "__main__":
    {"sample": sample}[sys.argv[1]](sys.argv[2:])
