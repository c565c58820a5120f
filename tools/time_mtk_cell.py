#!/usr/bin/env python3
"""The three launches of one m3g_mtk_step call (flexible-cell MTK NPT, both cell masks; chain_length 3) against the three of
m3g_nhc_step in NPT (the isotropic MTK barostat), back to back on one stream and timed with device events, in the style of
tools/time_nose_hoover.py: the 32-atom cell, a 256 x 32-atom batch and one 10,000-atom cell.  No model: zero forces and stresses on
an ideal gas at 300 K whose velocities are whitened (sum m v v^T is a multiple of the identity, so no shear force acts on the cell)
at its own pressure n kT / V, which costs the kernels what any other input does.  The variants alternate inside every repeat, so a
drift of the machine falls on all of them.

    python tools/time_mtk_cell.py [calls per window] [repeats]
Prints one JSON line per case: microseconds per call, the median and the spread over the repeats.  Under a kernel trace
(rocprofv3 --kernel-trace --stats -- python tools/time_mtk_cell.py 200 1) the k_mtk_* / k_nhc_* rows give the split by launch."""
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "torch-m3gnet_amd"))
from torch_m3gnet.dynamics import KB, MtkCellState, NhcState, maxwell_boltzmann, mtk_cell_step, nhc_step  # noqa: E402

calls = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
dev = torch.device("cuda")
MASS, T0, VOL_PER_ATOM = 63.546, 300.0, 11.76


def whitened(v):
    """v times the symmetric matrix that makes v^T v a multiple of the identity, at the same kinetic energy."""
    w, u = np.linalg.eigh(v.T @ v)
    return v @ (u * np.sqrt(w.mean() / w)) @ u.T


def states(sizes):
    offsets = np.concatenate([[0], np.cumsum(sizes)])
    n = int(offsets[-1])
    rng = np.random.default_rng(0)
    lats = np.stack([np.eye(3) * (VOL_PER_ATOM * k) ** (1 / 3) for k in sizes])
    pos0 = np.concatenate([rng.uniform(0, 1, (k, 3)) @ L for k, L in zip(sizes, lats)])
    vel0 = np.concatenate([whitened(maxwell_boltzmann(np.full(k, MASS), T0, s)) for s, k in enumerate(sizes)])
    p_gas = KB * T0 / VOL_PER_ATOM

    def tensors():
        return (torch.tensor(pos0, device=dev), torch.tensor(lats, device=dev), offsets, np.full(n, MASS), torch.tensor(vel0, device=dev))

    common = dict(dt=1.0, taut=100.0, pressure=p_gas, taup=1000.0, fix_com=True, chain_length=3, chain_substeps=1)
    made = {"npt_mtk": (NhcState(*tensors(), T0, ensemble="npt_mtk", **common), nhc_step)}
    for mask in ("full", "orthorhombic"):
        made[f"npt_mtk_cell {mask}"] = (MtkCellState(*tensors(), T0, cell_mask=mask, **common), mtk_cell_step)
    return n, made


def case(name, sizes):
    n, made = states(sizes)
    f = torch.zeros(n, 3, dtype=torch.float32, device=dev)
    s = torch.zeros(len(sizes), 6, dtype=torch.float32, device=dev)
    for st, step in made.values():   # warm up: code objects, first launches
        for _ in range(20):
            step(st, f, s)
    torch.cuda.synchronize()
    us = {key: [] for key in made}
    for _ in range(repeats):
        for key, (st, step) in made.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                step(st, f, s)
            e1.record()
            torch.cuda.synchronize()
            us[key].append(e0.elapsed_time(e1) / calls * 1e3)
    ok = all(bool(torch.isfinite(st.pos).all()) and not (st.read()["flags"] & 2).any() for st, _ in made.values())
    print(json.dumps({"case": name, "atoms": n, "structures": len(sizes), "calls_per_window": calls, "repeats": repeats, "finite": ok,
                      "us_per_call_median": {k: round(float(np.median(v)), 2) for k, v in us.items()},
                      "us_per_call_min_max": {k: [round(min(v), 2), round(max(v), 2)] for k, v in us.items()}}), flush=True)


case("cu32", [32])
case("cu32x256", [32] * 256)
case("cu10k", [10000])
