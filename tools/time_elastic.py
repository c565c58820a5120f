#!/usr/bin/env python3
"""Time of the batched elastic constants and equation of state (torch_m3gnet.elasticity) for fcc Cu (4-atom conventional cell and
32-atom cell, a = 3.61 A) and rutile TiO2 (6-atom cell, a = 4.594 A, c = 2.959 A, u = 0.305), clamped ions, default model
(bench.default_model).  Per case: the three calls (deform, elastic fit, EOS fit) under device events around `reps` back-to-back
repetitions -- the time per call of a queue that the host keeps fed, an upper bound of the kernel's own time (that one comes from
`rocprofv3 --kernel-trace --stats -- python tools/time_elastic.py`); a whole `Elasticity.run` and `EquationOfState.run` (host clock
around `reps / 10` calls that end in a device synchronise, first call excluded);
and the baseline a user has without the driver: the same 25 (11) copies deformed on the host and evaluated one `VerletGraph` at a
time, each stress (energy) copied back, the lines (the cubic) fitted with numpy.  The ratio is reported, nothing is gated on it.

    python tools/time_elastic.py [reps]
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
from torch_m3gnet.elasticity import (Elasticity, ElasticState, EquationOfState, el_deform, el_fit_elastic, el_fit_eos,  # noqa: E402
                                     elastic_deformations, eos_deformations)

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
dev = torch.device("cuda")
model = bench.default_model(dev)


def events(fn, n=reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / n, 4)


def wall(fn, n=max(3, reps // 10)):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return round((time.perf_counter() - t0) / n * 1e3, 3)


def host_loop(pv, lat, pos, z, components, magnitudes):
    """The copies one at a time: deform on the host, build the graph, evaluate, copy the results back; then the fits in numpy."""
    voigt = ((0, 0), (1, 1), (2, 2), (1, 2), (2, 0), (0, 1))
    sigma, energy = [], []
    for c, d in [(0, 0.0)] + list(zip(components, magnitudes)):
        D = np.eye(3)
        if c == 6:
            D *= 1.0 + d
        elif c < 3:
            D[c, c] += d
        else:
            a, b = voigt[c]
            D[a, b] = D[b, a] = 0.5 * d
        vg = VerletGraph([lat @ D], [z], 5.0, 4.0, skin=0.5, device=dev)
        out = vg.step(pv, torch.tensor(pos @ D, device=dev))
        sigma.append(-out[K.STRESSES].double().cpu().numpy().reshape(6))
        energy.append(float(out[K.TOTAL_ENERGY].double().reshape(-1)[0]))
    sigma = np.array(sigma)
    if components[0] == 6:
        t = np.concatenate([[0.0], (1.0 + np.asarray(magnitudes)) ** -2.0 - 1.0])
        return np.polyfit(t, energy, 3)
    c_raw = np.zeros((6, 6))
    for j in range(6):
        rows = np.concatenate([[0], 1 + np.flatnonzero(np.asarray(components) == j)])
        x = np.concatenate([[0.0], np.asarray(magnitudes)[rows[1:] - 1]])
        c_raw[:, j] = np.polyfit(x, sigma[rows], 1)[0]
    return c_raw


def case(name, lat, pos, z):
    el, eos = Elasticity(model, relax_atoms=False), EquationOfState(model, relax_atoms=False)
    t = {}
    for mode, (comp, mag) in (("elastic", elastic_deformations()), ("eos", eos_deformations())):
        st = ElasticState([lat], [pos], comp, mag, device=dev)
        t[f"deform_{mode}_ms"] = events(lambda: el_deform(st))
        if mode == "elastic":
            s = torch.randn(st.copies, 6, device=dev)
            t["fit_elastic_ms"] = events(lambda: el_fit_elastic(st, s))
        else:
            e = torch.randn(st.copies, device=dev)
            t["fit_eos_ms"] = events(lambda: el_fit_eos(st, e))
    t["elasticity_run_ms"] = wall(lambda: el.run([lat], [pos], [z]))
    t["eos_run_ms"] = wall(lambda: eos.run([lat], [pos], [z]))
    t["elasticity_host_loop_ms"] = wall(lambda: host_loop(el.model, lat, pos, z, el.components, el.magnitudes))
    t["eos_host_loop_ms"] = wall(lambda: host_loop(eos.model, lat, pos, z, eos.components, eos.magnitudes))
    t["elasticity_ratio"] = round(t["elasticity_host_loop_ms"] / t["elasticity_run_ms"], 2)
    t["eos_ratio"] = round(t["eos_host_loop_ms"] / t["eos_run_ms"], 2)
    print(json.dumps({"case": name, "atoms": len(z), "elastic_copies": 25, "eos_copies": 11, **t, "reps": reps}), flush=True)


base = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])
grid = np.stack(np.meshgrid(*[np.arange(2)] * 3, indexing="ij"), -1).reshape(-1, 1, 3)
case("Cu conventional, 4 atoms", np.eye(3) * 3.61, base * 3.61, np.full(4, 29))
case("Cu 2x2x2, 32 atoms", np.eye(3) * 7.22, (grid + base[None]).reshape(-1, 3) * 3.61, np.full(32, 29))
a, c, u = 4.594, 2.959, 0.305
frac = np.array([[0, 0, 0], [0.5, 0.5, 0.5], [u, u, 0], [1 - u, 1 - u, 0], [0.5 + u, 0.5 - u, 0.5], [0.5 - u, 0.5 + u, 0.5]])
lat = np.diag([a, a, c])
case("TiO2 rutile, 6 atoms", lat, frac @ lat, np.array([22, 22, 8, 8, 8, 8]))
