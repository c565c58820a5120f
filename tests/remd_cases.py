"""The synthetic replica-exchange cases of tests/test_gpu_remd.py and their reference runs (numpy: tests/md_reference.py and
tests/remd_reference.py), shared with tests/test_remd_cpu.py, which checks the chosen seeds without a GPU.

Three ladders -- R = 2 (odd attempts have no pair), 3 and 5 replicas of 257 (past a 256-row chunk), 1 and 3 atoms -- with synthetic
forces and energies drawn per (ladder, call), so a ladder sees the same inputs alone and in any batch.  The energies spread by about
0.1 eV, which makes Delta of order 1 at these temperatures.  A schedule is a list of ("step", call, finish_only) and ("exchange",
round) operations applied to every ladder."""
from __future__ import annotations

import numpy as np

import md_reference as mr
import remd_reference as rr

# (temperatures, atoms per replica, exchange seed, Langevin seeds of the replicas)
LADDERS = [
    ([300.0, 420.0], 257, 2 ** 63 + 11, [11, 2 ** 63 + 5]),
    ([200.0, 260.0, 350.0], 1, 7, [77, 12345, 2 ** 64 - 1]),
    ([300.0, 380.0, 470.0, 600.0, 800.0], 3, 2 ** 64 - 3, [3, 5, 8, 13, 21]),
]
PARAMS = dict(dt=1.0, friction=0.02)
ROUNDS = 12


def schedule(rounds: int = ROUNDS) -> list:
    """start a step, finish it at the next forces, exchange, start the next step with the same forces."""
    ops = []
    for r in range(rounds):
        ops += [("step", 2 * r, False), ("step", 2 * r + 1, True), ("exchange", r), ("step", 2 * r + 1, False)]
    return ops


def started_schedule() -> list:
    """Exchanges 1 and 4 are made while every replica is STARTED (no finish_only call before them)."""
    ops = []
    for r in range(6):
        if r in (1, 4):
            ops += [("step", 2 * r, False), ("exchange", r), ("step", 2 * r + 1, False)]
        else:
            ops += [("step", 2 * r, False), ("step", 2 * r + 1, True), ("exchange", r), ("step", 2 * r + 1, False)]
    return ops


def start(g: int):
    """Lattices, positions, masses and Maxwell-Boltzmann velocities of the replicas of ladder g."""
    from torch_m3gnet.dynamics import maxwell_boltzmann

    temps, n, _, seeds = LADDERS[g]
    rng = np.random.default_rng([5, g])
    lats, poss, ms, vs = [], [], [], []
    for t, sd in zip(temps, seeds):
        L = np.eye(3) * (12.0 * n) ** (1 / 3) + rng.normal(0, 0.05, (3, 3))
        lats.append(L)
        poss.append(rng.uniform(0, 1, (n, 3)) @ L)
        ms.append(rng.uniform(1.0, 200.0, n))
        vs.append(maxwell_boltzmann(ms[-1], t, sd % 2 ** 32) if n > 1 else rng.normal(0, 1e-3, (1, 3)))
    return lats, poss, ms, vs


def forces(g: int, call: int, nan_force=None) -> np.ndarray:
    """[R n, 3] float32 forces of ladder g at `call`; nan_force = {(g, call): row} makes one component NaN."""
    temps, n, _, _ = LADDERS[g]
    f = np.random.default_rng([17, g, call]).normal(0, 0.5, (len(temps) * n, 3)).astype(np.float32)
    if nan_force and (g, call) in nan_force:
        f[nan_force[g, call], 1] = np.nan
    return f


def energies(g: int, rnd: int, nan_energy=None) -> np.ndarray:
    """[R] float32 energies of ladder g at exchange `rnd`; nan_energy = {(g, rnd): replica} makes one NaN."""
    temps = LADDERS[g][0]
    e = np.random.default_rng([23, g, rnd]).normal(-1.0, 0.12, len(temps)).astype(np.float32)
    if nan_energy and (g, rnd) in nan_energy:
        e[nan_energy[g, rnd]] = np.nan
    return e


def reference(g: int, ops: list, nan_force=None, nan_energy=None) -> dict:
    """Ladder g through `ops`: {"refs": DynReference per replica, "ladder": LadderReference, "obs": [calls, R, 4] after every step
    operation, "scales": the velocity scales of every exchange}."""
    temps, n, seed, seeds = LADDERS[g]
    lats, poss, ms, vs = start(g)
    refs = [mr.DynReference(p, L, m, v, "nvt_langevin", temperature=t, seed=sd, **PARAMS)
            for p, L, m, v, t, sd in zip(poss, lats, ms, vs, temps, seeds)]
    lad = rr.LadderReference(temps, seed)
    obs, scales = [], []
    for op in ops:
        if op[0] == "step":
            f = forces(g, op[1], nan_force).astype(np.float64)
            for r, ref in enumerate(refs):
                ref.step(f[r * n:(r + 1) * n], np.zeros(6), finish_only=op[2])
            obs.append([ref.obs.copy() for ref in refs])
        else:
            scales.append(lad.exchange_dyn(energies(g, op[1], nan_energy).astype(np.float64), refs))
    return {"refs": refs, "ladder": lad, "obs": np.array(obs), "scales": scales}
