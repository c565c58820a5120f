#!/usr/bin/env python3
"""The three launches of one m3g_pimd_step call (ring polymers under PILE-L, and without thermostat: what the noise costs) against the three of m3g_dyn_step (Langevin) on the same
rows in the same process, back to back on one stream and timed with device events: a 32-atom cell as a ring of 8 beads (256 rows)
and a 10,000-atom cell as a ring of 4 (40,000 rows); then the bead-count buckets of k_pimd_apply on 32-atom rings of 8, 16, 32 and
64 beads.  No model: zero forces on an ideal gas at 300 K, which costs the kernels what any other input does.  The variants alternate
inside every repeat, so a drift of the machine falls on all of them.

    python tools/time_path_integral.py [calls per window] [repeats] [case]
Prints one JSON line per case: microseconds per call, the median and the spread over the repeats.  Under a kernel trace
(rocprofv3 --kernel-trace --stats -- python tools/time_path_integral.py 200 1 cu32x8) the k_pimd_* / k_dyn_* rows give the split by
launch of that case."""
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "torch-m3gnet_amd"))
from torch_m3gnet.dynamics import DynState, dyn_step, maxwell_boltzmann  # noqa: E402
from torch_m3gnet.path_integral import PimdState, pimd_step  # noqa: E402

calls = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
dev = torch.device("cuda")
MASS, T0, VOL_PER_ATOM = 63.546, 300.0, 11.76


def states(n, beads):
    """One ring of `beads` beads of n atoms, and the same rows as `beads` Langevin structures."""
    rows = n * beads
    offsets = n * np.arange(beads + 1)
    rng = np.random.default_rng(0)
    pos0 = np.tile(rng.uniform(0, 1, (n, 3)) * (VOL_PER_ATOM * n) ** (1 / 3), (beads, 1))
    vel0 = np.concatenate([maxwell_boltzmann(np.full(n, MASS), beads * T0, j) for j in range(beads)])
    ring = {name: PimdState(torch.tensor(pos0, device=dev), offsets, np.full(rows, MASS), torch.tensor(vel0, device=dev), T0, [1], beads,
                            thermostat=name, dt=0.5) for name in ("pile_l", "none")}
    langevin = DynState(torch.tensor(pos0, device=dev), None, offsets, np.full(rows, MASS), torch.tensor(vel0, device=dev), T0,
                        np.arange(beads), ensemble="nvt_langevin", dt=0.5, friction=0.01)
    return rows, {"pimd_pile_l": (ring["pile_l"], pimd_step), "pimd_none": (ring["none"], pimd_step), "nvt_langevin": (langevin, dyn_step)}


def case(name, n, beads):
    rows, made = states(n, beads)
    f = torch.zeros(rows, 3, dtype=torch.float32, device=dev)
    for st, step in made.values():   # warm up: code objects, first launches
        for _ in range(20):
            step(st, f)
    torch.cuda.synchronize()
    us = {key: [] for key in made}
    for _ in range(repeats):
        for key, (st, step) in made.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                step(st, f)
            e1.record()
            torch.cuda.synchronize()
            us[key].append(e0.elapsed_time(e1) / calls * 1e3)
    ok = all(bool(torch.isfinite(st.pos).all()) and not (st.read()["flags"] & 2).any() for st, _ in made.values())
    print(json.dumps({"case": name, "rows": rows, "atoms": n, "beads": beads, "calls_per_window": calls, "repeats": repeats, "finite": ok,
                      "us_per_call_median": {k: round(float(np.median(v)), 2) for k, v in us.items()},
                      "us_per_call_min_max": {k: [round(min(v), 2), round(max(v), 2)] for k, v in us.items()}}), flush=True)


only = sys.argv[3] if len(sys.argv) > 3 else None   # one case by name (for a kernel trace of that case alone)
for name, n, beads in (("cu32x8", 32, 8), ("cu10kx4", 10000, 4), ("cu32x16", 32, 16), ("cu32x32", 32, 32), ("cu32x64", 32, 64)):
    if only in (None, name):
        case(name, n, beads)
