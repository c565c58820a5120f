#!/usr/bin/env python3
"""Time per stage of the batched finite-displacement phonons (torch_m3gnet.phonons): displace, engine (VerletGraph.step of the
displaced batch), force constants, dynamical matrices and eigenvalues of a 20^3 mesh, for fcc Cu (4-atom conventional cell, a = 3.61
A) at 3x3x3 and 4x4x4 and rutile TiO2 (6-atom cell, a = 4.594 A, c = 2.959 A, u = 0.305) at 3x3x4.  Default model
(bench.default_model).  Every stage is timed with device events around `reps` repetitions (the engine: a fresh VerletGraph's first
step excluded, then `reps` steps at the same positions); the complex128 eigvalsh is timed once for comparison with the real embedding.
The eigensolvers of the mesh are timed side by side, alternating, as the minimum and the median of `reps` windows of 5 back-to-back
calls each after a warm-up: the real embedding (`_eigvalsh`), the library's Jacobi solver with eigenvalues only and with
eigenvectors (`linalg.eigh_batched`); then the derivative of the dynamical matrices and the group velocities of the same mesh.

    python tools/time_phonons.py [reps]
Prints one JSON line per case."""
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "torch-m3gnet_amd"):
    sys.path.insert(0, str(p))
import bench  # noqa: E402
from torch_m3gnet.data import MaterialGraphKey as K  # noqa: E402
from torch_m3gnet.data.atomic_masses import masses_of  # noqa: E402
from torch_m3gnet.data.md import VerletGraph  # noqa: E402
from torch_m3gnet.nn import Gradient  # noqa: E402
from torch_m3gnet.linalg import EIGH_MAX_N, eigh_batched  # noqa: E402
from torch_m3gnet.phonons import (PhononState, _eigvalsh, monkhorst_pack, ph_displace, ph_dynamical_matrices,  # noqa: E402
                                  ph_dynamical_matrix_gradients, ph_force_constants, ph_group_velocities)

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
dev = torch.device("cuda")
model = Gradient(bench.default_model(dev).model, pair_virial=True)


def timed(fn, n=reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / n, 4)


def timed_side_by_side(fns: dict, windows=reps, calls=5) -> dict:
    """{name: [min, median]} ms per call of each function: `windows` windows of `calls` back-to-back calls under device events, the
    functions alternating window by window, every one warmed first."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            samples[k].append(e0.elapsed_time(e1) / calls)
    return {k: [round(float(np.min(v)), 4), round(float(np.median(v)), 4)] for k, v in samples.items()}


def case(name, lat, pos, z, sc, mesh=20):
    st = PhononState([lat], [pos], [masses_of(z)], [sc], 0.01, device=dev)
    t = {"displace_ms": timed(lambda: ph_displace(st))}
    ns = int(st.super_sizes[0])
    copies = st.rows // ns
    vg = VerletGraph([st.supercell_lattice(0)] * copies, [st.supercell_numbers(0, z)] * copies, 5.0, 4.0, skin=0.5, device=dev)
    out = vg.step(model, st.pos)
    t["engine_ms"] = timed(lambda: vg.step(model, st.pos))
    f = out[K.FORCES]
    t["force_constants_ms"] = timed(lambda: ph_force_constants(st, f, True))
    q = torch.tensor(monkhorst_pack(mesh), device=dev)
    t["dynmat_ms"] = timed(lambda: ph_dynamical_matrices(st, 0, q))
    d = ph_dynamical_matrices(st, 0, q)
    t["eigh_real_embedding_ms"] = timed(lambda: _eigvalsh(d))
    t["eigh_complex128_ms"] = timed(lambda: torch.linalg.eigvalsh(d), n=1)
    assert d.shape[-1] <= EIGH_MAX_N
    w, v, info = eigh_batched(d)
    g = ph_dynamical_matrix_gradients(st, 0, q)
    t["min_median_ms"] = timed_side_by_side({
        "eigh_real_embedding": lambda: _eigvalsh(d),
        "eigh_jacobi_values": lambda: eigh_batched(d, eigenvectors=False),
        "eigh_jacobi_vectors": lambda: eigh_batched(d),
        "dynmat_gradient": lambda: ph_dynamical_matrix_gradients(st, 0, q),
        "group_velocities": lambda: ph_group_velocities(w, v, g)})
    t["jacobi_max_sweeps"] = int((info & 0xff).max())
    # both solvers against numpy.linalg.eigvalsh on the first 256 matrices, as a fraction of the largest eigenvalue
    ref = torch.tensor(np.linalg.eigvalsh(d[:256].cpu().numpy()), device=dev)
    t["jacobi_max_dev_from_numpy"] = float((w[:256] - ref).abs().max() / ref.abs().max())
    t["embedding_max_dev_from_numpy"] = float((_eigvalsh(d[:256]) - ref).abs().max() / ref.abs().max())
    print(json.dumps({"case": name, "unit_atoms": len(z), "supercell": list(sc), "supercell_atoms": ns, "displaced_rows": st.rows,
                      "engine_structures": copies, "qpoints": len(q), **t, "reps": reps}), flush=True)


base = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])
case("Cu conventional 3x3x3", np.eye(3) * 3.61, base * 3.61, np.full(4, 29), (3, 3, 3))
case("Cu conventional 4x4x4", np.eye(3) * 3.61, base * 3.61, np.full(4, 29), (4, 4, 4))
a, c, u = 4.594, 2.959, 0.305
frac = np.array([[0, 0, 0], [0.5, 0.5, 0.5], [u, u, 0], [1 - u, 1 - u, 0], [0.5 + u, 0.5 - u, 0.5], [0.5 - u, 0.5 + u, 0.5]])
lat = np.diag([a, a, c])
case("TiO2 rutile 3x3x4", lat, frac @ lat, np.array([22, 22, 8, 8, 8, 8]), (3, 3, 4))
