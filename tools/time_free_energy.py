#!/usr/bin/env python3
"""The three launches of one m3g_ti_step call (thermodynamic integration: centre-of-mass-conserving Langevin under the mixed force,
with and without friction: what the two Philox draws cost) against the three of m3g_dyn_step (Langevin) on the same rows in the same
process, back to back on one stream and timed with device events: one cell of 32, 864 and 10,000 atoms.  No model: zero forces and
energies at lambda = 1/2, so the springs pull; that costs the kernels what any other input does.  The variants alternate inside every
repeat, so a drift of the machine falls on all of them.

    python tools/time_free_energy.py [calls per window] [repeats] [case]
Prints one JSON line per case: microseconds per call, the median and the spread over the repeats.  Under a kernel trace
(rocprofv3 --kernel-trace --stats -- python tools/time_free_energy.py 200 1 cu864) the k_ti_* / k_dyn_* rows give the split by launch
of that case."""
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "torch-m3gnet_amd"))
from torch_m3gnet.dynamics import DynState, dyn_step, maxwell_boltzmann  # noqa: E402
from torch_m3gnet.free_energy import TiState, ti_path, ti_step  # noqa: E402

calls = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
dev = torch.device("cuda")
MASS, T0, VOL_PER_ATOM = 63.546, 300.0, 11.76


def states(n):
    """One cell of n atoms as a thermodynamic-integration structure (friction 0.01 /fs and 0) and as a Langevin structure."""
    rng = np.random.default_rng(0)
    pos0 = rng.uniform(0, 1, (n, 3)) * (VOL_PER_ATOM * n) ** (1 / 3)
    vel0 = maxwell_boltzmann(np.full(n, MASS), T0, 0)
    made = {}
    for name, friction in (("ti_langevin", 0.01), ("ti_no_friction", 0.0)):
        pos = torch.tensor(pos0, device=dev)
        st = TiState(pos, [0, n], np.full(n, MASS), np.full(n, 2.0), torch.tensor(vel0, device=dev), pos.clone(), T0, [1], dt=1.0,
                     friction=friction)
        ti_path(st, 0.5, 0.5, 0)
        made[name] = (st, lambda s, f, e: ti_step(s, f, e))
    langevin = DynState(torch.tensor(pos0, device=dev), None, [0, n], np.full(n, MASS), torch.tensor(vel0, device=dev), T0, [1],
                        ensemble="nvt_langevin", dt=1.0, friction=0.01)
    made["nvt_langevin"] = (langevin, lambda s, f, e: dyn_step(s, f))
    return made


def case(name, n):
    made = states(n)
    f = torch.zeros(n, 3, dtype=torch.float32, device=dev)
    e = torch.zeros(1, dtype=torch.float32, device=dev)
    for st, step in made.values():   # warm up: code objects, first launches
        for _ in range(20):
            step(st, f, e)
    torch.cuda.synchronize()
    us = {key: [] for key in made}
    for _ in range(repeats):
        for key, (st, step) in made.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                step(st, f, e)
            e1.record()
            torch.cuda.synchronize()
            us[key].append(e0.elapsed_time(e1) / calls * 1e3)
    ok = all(bool(torch.isfinite(st.pos).all()) and not (st.read()["flags"] & 2).any() for st, _ in made.values())
    print(json.dumps({"case": name, "atoms": n, "calls_per_window": calls, "repeats": repeats, "finite": ok,
                      "us_per_call_median": {k: round(float(np.median(v)), 2) for k, v in us.items()},
                      "us_per_call_min_max": {k: [round(min(v), 2), round(max(v), 2)] for k, v in us.items()}}), flush=True)


only = sys.argv[3] if len(sys.argv) > 3 else None   # one case by name (for a kernel trace of that case alone)
for name, n in (("cu32", 32), ("cu864", 864), ("cu10k", 10000)):
    if only in (None, name):
        case(name, n)
