"""The synthetic swap Monte Carlo cases of tests/test_gpu_mc.py and their reference runs (numpy: tests/mc_reference.py, and
tests/md_reference.py for the runs over a dynamics state), shared with tests/test_mc_cpu.py, which checks the chosen seeds without a
GPU.

Eight structures of 2, 3, 64, 65, 257 and 300 atoms -- on either side of the 64-lane wave and of the 256-row chunk, a single-chunk and
two-chunk ones -- with two and three species in unequal counts, a site mask that leaves a species out, a single-species structure and
one with a single active row (both NO_PAIR), and seeds above 2^63.  Energies, forces and stresses are synthetic, drawn per
(structure, call), so a structure sees the same inputs alone and in any batch.  The energies spread by 0.03 eV, which makes
dE / (KB T) of order 1 at these temperatures: both verdicts occur."""
from __future__ import annotations

import numpy as np

import mc_reference as mcr
import md_reference as mr


def _species(counts: dict, seed: int) -> np.ndarray:
    z = np.concatenate([np.full(n, t) for t, n in counts.items()])
    return np.random.default_rng([41, seed]).permutation(z).astype(np.int64)


def _mask_65() -> np.ndarray:
    """Species 7 (and three rows of species 2) sit the run out."""
    z = STRUCTURES[3][0]
    m = z != 7
    m[np.flatnonzero(z == 2)[:3]] = False
    return m


# (species index per row (atom_types), temperature, seed, site mask or None)
STRUCTURES = [
    (np.array([4, 9], dtype=np.int64), 300.0, 2 ** 63 + 11, None),
    (np.array([3, 3, 28], dtype=np.int64), 450.0, 7, None),
    (_species({0: 10, 12: 20, 28: 34}, 2), 350.0, 2 ** 64 - 3, None),
    (_species({2: 25, 5: 28, 7: 12}, 3), 300.0, 12345, None),        # mask filled in below
    (_species({28: 100, 12: 157}, 4), 520.0, 2 ** 63 + 5, None),
    (_species({7: 50, 21: 100, 30: 150}, 5), 400.0, 99, None),
    (np.full(65, 28, dtype=np.int64), 300.0, 3, None),               # one species: NO_PAIR on the device
    (np.array([1, 2, 3], dtype=np.int64), 300.0, 5, np.array([False, True, False])),   # one active row: NO_PAIR at init
]
STRUCTURES[3] = STRUCTURES[3][:3] + (_mask_65(),)
ROUNDS = 200
UNTOUCHED = -7   # what the tests fill the history with


def mask(g: int) -> np.ndarray:
    z, _, _, m = STRUCTURES[g]
    return np.ones(len(z), dtype=bool) if m is None else m


def energies(g: int, call: int, bad=None) -> np.float32:
    """float32 energy of structure g at evaluation `call` (0: the starting configuration, r + 1: the trial of round r); bad =
    {(g, call): value} replaces it."""
    if bad and (g, call) in bad:
        return np.float32(bad[g, call])
    return np.random.default_rng([23, g, call]).normal(-1.0, 0.03, 1).astype(np.float32)[0]


def forces(g: int, call: int, nan_force=None) -> np.ndarray:
    """[n, 3] float32 forces of structure g at `call`; nan_force = {(g, call): row} makes one component NaN."""
    f = np.random.default_rng([17, g, call]).normal(0, 0.5, (len(STRUCTURES[g][0]), 3)).astype(np.float32)
    if nan_force and (g, call) in nan_force:
        f[nan_force[g, call], 1] = np.nan
    return f


def stresses(g: int, call: int) -> np.ndarray:
    return np.random.default_rng([19, g, call]).normal(0, 0.01, 6).astype(np.float32)


def reference(g: int, rounds: int = ROUNDS, bad=None, with_forces: bool = True) -> dict:
    """Structure g through `rounds` propose / decide rounds: {"mc": SwapReference, "types" [rounds, n] after every round, "e" [rounds]
    the current energy, "f" / "s": the current forces / stresses at the end, "verdicts": per round 1 / 0 / None}."""
    z, T, seed, _ = STRUCTURES[g]
    mc = mcr.SwapReference(z, T, seed, mask(g))
    e = energies(g, 0, bad)
    f, s = forces(g, 0), stresses(g, 0)
    types, es, verdicts = [], [], []
    for r in range(rounds):
        mc.propose(e)
        verdict, e = mc.decide(energies(g, r + 1, bad), e)
        if verdict and with_forces:
            f, s = forces(g, r + 1), stresses(g, r + 1)
        types.append(list(mc.types))
        es.append(e)
        verdicts.append(verdict)
    return {"mc": mc, "types": np.array(types), "e": np.array(es, dtype=np.float32), "f": f, "s": s, "verdicts": verdicts}


# ---- over a dynamics state ------------------------------------------------------------------------------------------------------------
DYN_STRUCTURES = [1, 3, 4]   # 3 atoms, 65 with the mask, 257 (two chunks)
DYN_PARAMS = dict(dt=1.0, friction=0.02)
DYN_ROUNDS = 12


def schedule(rounds: int = DYN_ROUNDS) -> list:
    """start a step, finish it at the next forces, one swap trial, start the next step with the same forces (the schedule of
    remd_cases.schedule)."""
    ops = []
    for r in range(rounds):
        ops += [("step", 2 * r, False), ("step", 2 * r + 1, True), ("swap", r), ("step", 2 * r + 1, False)]
    return ops


def started_schedule() -> list:
    """The proposals of rounds 1 and 4 are made while every structure is STARTED (no finish_only call before them)."""
    ops = []
    for r in range(6):
        if r in (1, 4):
            ops += [("step", 2 * r, False), ("swap", r), ("step", 2 * r + 1, False)]
        else:
            ops += [("step", 2 * r, False), ("step", 2 * r + 1, True), ("swap", r), ("step", 2 * r + 1, False)]
    return ops


def start(g: int):
    """Lattice, positions, masses (one per atom, all different) and Maxwell-Boltzmann velocities of structure g."""
    from torch_m3gnet.dynamics import maxwell_boltzmann

    z, T, seed, _ = STRUCTURES[g]
    n = len(z)
    rng = np.random.default_rng([5, g])
    L = np.eye(3) * (12.0 * n) ** (1 / 3) + rng.normal(0, 0.05, (3, 3))
    m = rng.uniform(1.0, 200.0, n)
    return L, rng.uniform(0, 1, (n, 3)) @ L, m, maxwell_boltzmann(m, T, seed % 2 ** 32)


def dyn_reference(g: int, ops: list, nan_force=None) -> dict:
    """Structure g through `ops`: {"dyn": DynReference, "mc": SwapReference, "e": current energy, "ke": [(before, after proposal,
    after verdict)] per swap, "mv": [(masses, velocities)] after every swap}."""
    z, T, seed, _ = STRUCTURES[g]
    L, x, m, v = start(g)
    dyn = mr.DynReference(x, L, m, v, "nvt_langevin", temperature=T, seed=seed, **DYN_PARAMS)
    mc = mcr.SwapReference(z, T, seed, mask(g))
    e = energies(g, 0)
    ke, mv = [], []
    for op in ops:
        if op[0] == "step":
            dyn.step(forces(g, op[1], nan_force).astype(np.float64), np.zeros(6), finish_only=op[2])
        else:
            k0 = dyn.kinetic_energy
            mc.propose_dyn(e, dyn)
            k1 = dyn.kinetic_energy
            _, e = mc.decide_dyn(energies(g, op[1] + 1), e, dyn)
            ke.append((k0, k1, dyn.kinetic_energy))
            mv.append((dyn.m.copy(), dyn.v.copy()))
    return {"dyn": dyn, "mc": mc, "e": e, "ke": ke, "mv": mv}
