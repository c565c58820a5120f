"""The inputs of tests/test_gpu_meta.py and tests/test_gpu_meta_guard.py: structures of 2, 7, 257 and 600 atoms (a part-filled
chunk, a one-row second chunk, several chunks) in triclinic cells with positions spread over -2 .. 3 cells, the batch of five
structures in groups of 1, 1, 1 and 2 walkers (the 600-atom structure twice), the restatement of the same batch, and the refusals of
m3g_meta_init.  The restatement's side runs on the CPU (tests/test_meta_cpu.py checks the construction there)."""
import ctypes as C
import functools

import numpy as np

import meta_reference as mr

SIZES = [2, 7, 257, 600]
BATCH = ((0, 0), (1, 0), (2, 0), (3, 0), (3, 1))     # (structure, variant of its positions) of every batch slot
GROUPS = (1, 1, 1, 2)                                # walkers per group over those slots
KIND_IDS = {"distance": mr.DISTANCE, "projection": mr.PROJECTION, "coordination": mr.COORDINATION}
POWER, R0, R_CUT = (3, 1), (2.5, 3.0), (4.0, 5.0)    # COORDINATION, per CV slot: p = 1 takes the branch without a multiplication
RAW_DIRECTIONS = np.array([[1.0, 2.5, -2.0], [0.3, 3.0, 4.0]])
DIRECTIONS = np.stack([n / np.linalg.norm(n) for n in RAW_DIRECTIONS])   # as metadynamics.projection normalises what it is given
SIGMA = np.array([0.4, 0.7])


@functools.lru_cache(maxsize=None)
def structure(idx: int, variant: int = 0):
    """(lattice, positions, weights, membership [2, n], forces float32, origins [2, 3]): everything but the positions and the forces
    depends on `idx` alone (the walkers of a group are copies that moved apart)."""
    n = SIZES[idx]
    rng = np.random.default_rng([11, idx])
    lattice = np.diag([12.0, 13.0, 14.0]) + rng.uniform(-1.0, 1.0, (3, 3))
    weights = rng.uniform(1.0, 100.0, n)
    membership = rng.choice(np.array([0, 0, 1, 2, 3], dtype=np.uint8), size=(2, n))
    membership[0, 0], membership[0, -1] = 1, 2      # both groups of both CVs hold an atom, and the two-atom structure is
    membership[1, 0], membership[1, -1] = 3, 3      # A - B under CV 0 and a pair counted from both sides under CV 1
    origins = rng.uniform(-1.0, 1.0, (2, 3))
    rng = np.random.default_rng([12, idx, variant])
    pos = rng.uniform(-2.0, 3.0, (n, 3)) @ lattice
    if n == 2:
        pos[1] = pos[0] + np.array([1.5, -2.0, 1.0]) + 2.0 * lattice[0] - lattice[2]   # a pair inside r_cut across the boundary
    forces = rng.normal(0.0, 1.0, (n, 3)).astype(np.float32)
    forces[0, 0] = -0.0
    return lattice, pos, weights, membership, forces, origins


def cvs_of(kinds, idx: int) -> list:
    membership = structure(idx)[3]
    return [mr.Cv(KIND_IDS[kind], membership[k], direction=DIRECTIONS[k], p=POWER[k], r0=R0[k], r_cut=R_CUT[k]) for k, kind in enumerate(kinds)]


@functools.lru_cache(maxsize=None)
def cv_values(kinds, idx: int, variant: int) -> np.ndarray:
    lattice, pos, weights, _, _, origins = structure(idx, variant)
    return mr.evaluate(cvs_of(kinds, idx), pos, lattice, weights, origins[:len(kinds)])["s"]


def restraints(kinds, slot: int, on: bool):
    """(centre [n_cv], kappa [n_cv], walls [n_cv,4]) of batch slot `slot`, set around the CV the slot starts at: the restraint pulls,
    even slots sit below their lower wall and above no upper one, odd slots the other way round."""
    n_cv = len(kinds)
    if not on:
        return np.zeros(n_cv), np.zeros(n_cv), np.zeros((n_cv, 4))
    s = cv_values(kinds, *BATCH[slot])
    centre, kappa = s + 0.3, np.array([1.5, 0.5])[:n_cv]
    lower, upper = (s + 0.1, s + 5.0) if slot % 2 == 0 else (s - 5.0, s - 0.2)
    walls = np.stack([lower, np.full(n_cv, 2.0), upper, np.full(n_cv, 0.75)], axis=1)
    return centre, kappa, walls


def reference_groups(kinds, slots, groups, on: bool, height: float, inv_kdt: float, max_hills: int, exp=np.exp) -> list:
    out, at = [], 0
    for R in groups:
        walkers = []
        for slot in slots[at:at + R]:
            lattice, _, weights, _, _, origins = structure(*BATCH[slot])
            centre, kappa, walls = restraints(kinds, slot, on)
            walkers.append(dict(lattice=lattice, weights=weights, origins=origins[:len(kinds)], centre=centre, kappa=kappa, walls=walls))
        out.append(mr.Group(cvs_of(kinds, BATCH[slots[at]][0]), walkers, SIGMA[:len(kinds)], height, inv_kdt, max_hills, exp=exp))
        at += R
    return out


def reference_call(refs, slots, groups, deposit: bool, positions=None):
    """One call of every group: (obs [S,8], forces_out, extras per slot)."""
    obs, f_out, extras, at = [], [], [], 0
    for ref, R in zip(refs, groups):
        mine = slots[at:at + R]
        pos = [structure(*BATCH[q])[1] if positions is None else positions[at + j] for j, q in enumerate(mine)]
        for o, f, x in ref.bias(pos, [structure(*BATCH[q])[4] for q in mine], deposit=deposit):
            obs.append(o)
            f_out.append(f)
            extras.append(x)
        at += R
    return np.stack(obs), np.concatenate(f_out), extras


# ---- the refusals of m3g_meta_init: (what to break, a piece of the reason) -------------------------------------------------------
def init_arguments():
    """Valid host arguments of m3g_meta_init for two structures of 3 and 2 atoms in one group each, CVs COORDINATION and PROJECTION."""
    return dict(n_cv=2, max_hills=4, kind=[mr.COORDINATION, mr.PROJECTION], power=[3, 0], r0=[2.0, 0.0], r_cut=[4.0, 0.0],
                direction=[[0.0, 0.0, 0.0], [0.0, 0.6, 0.8]], N=5, S=2, G=2, offsets=[0, 3, 5], group_offsets=[0, 1, 2],
                lattices=np.stack([np.eye(3) * 9.0, np.eye(3) * 10.0]), membership=np.array([[1, 2, 0, 3, 3], [1, 0, 2, 1, 0]], dtype=np.uint8),
                weights=np.ones(5), origins=np.zeros((2, 2, 3)), centres=np.zeros((2, 2)), kappas=np.ones((2, 2)),
                walls=np.zeros((2, 2, 4)), sigmas=np.ones((2, 2)), heights=np.ones(2), inv_kdt=np.ones(2))


def _set(key, value, index=None):
    def change(a):
        if index is None:
            a[key] = value
        else:
            a[key] = np.array(a[key], dtype=np.asarray(a[key]).dtype)
            a[key][index] = value
    return change


REFUSALS = [
    ("unknown kind", _set("kind", 7, 0), b"unknown kind"),
    ("n_cv 0", _set("n_cv", 0), b"n_cv must be"),
    ("n_cv 3", _set("n_cv", 3), b"n_cv must be"),
    ("empty A", _set("membership", 2, (0, 0)), b"empty group A"),
    ("empty B of coordination", _set("membership", 1, (0, slice(3, 5))), b"empty group B"),
    ("membership 4", _set("membership", 4, (1, 1)), b"membership"),
    ("total weight 0", _set("weights", 0.0, 0), b"total weight"),
    ("negative weight", _set("weights", -1.0, 2), b"weight of atom 2"),
    ("p 0", _set("power", 0, 0), b"power"),
    ("p 7", _set("power", 7, 0), b"power"),
    ("r0 0", _set("r0", 0.0, 0), b"r0"),
    ("r0 nan", _set("r0", np.nan, 0), b"r0"),
    ("r_cut 0", _set("r_cut", 0.0, 0), b"r_cut"),
    ("r_cut above half the cell", _set("r_cut", 4.6, 0), b"half the smallest perpendicular width"),
    ("direction not a unit vector", _set("direction", 0.7, (1, 1)), b"unit vector"),
    ("sigma 0", _set("sigmas", 0.0, (1, 0)), b"sigma"),
    ("sigma negative", _set("sigmas", -1.0, (0, 1)), b"sigma"),
    ("kappa negative", _set("kappas", -0.5, (1, 1)), b"kappa"),
    ("height negative", _set("heights", -1.0, 1), b"height"),
    ("inv_kdt negative", _set("inv_kdt", -1.0, 0), b"inv_kdt"),
    ("wall kappa negative", _set("walls", -1.0, (0, 0, 1)), b"wall"),
    ("offsets do not end at N", _set("offsets", [0, 3, 4]), b"offsets"),
    ("offsets do not increase", _set("offsets", [0, 5, 5]), b"offsets"),
    ("group offsets do not end at S", _set("group_offsets", [0, 1, 1]), b"group_offsets"),
    ("singular lattice", _set("lattices", 0.0, (1, 2, 2)), b"singular"),
    ("lattice not finite", _set("lattices", np.inf, (0, 0, 0)), b"not finite"),
    ("max_hills negative", _set("max_hills", -1), b"max_hills"),
]


def call_init(lib, _lib, a: dict, state, state_bytes: int) -> int:
    """m3g_meta_init over the host arguments `a`; `state`: a device pointer (never touched when a check refuses)."""
    p = _lib.M3GMetaParams(n_cv=a["n_cv"], reserved=0, max_hills=a["max_hills"])
    for k in range(2):
        p.kind[k], p.power[k], p.r0[k], p.r_cut[k] = int(a["kind"][k]), int(a["power"][k]), float(a["r0"][k]), float(a["r_cut"][k])
        for x in range(3):
            p.direction[k][x] = float(a["direction"][k][x])
    arrays = [np.ascontiguousarray(np.asarray(a[key], dtype=dtype)) for key, dtype in
              (("offsets", np.int64), ("group_offsets", np.int64), ("lattices", np.float64), ("membership", np.uint8), ("weights", np.float64),
               ("origins", np.float64), ("centres", np.float64), ("kappas", np.float64), ("walls", np.float64), ("sigmas", np.float64),
               ("heights", np.float64), ("inv_kdt", np.float64))]
    return lib.m3g_meta_init(C.byref(p), a["N"], a["S"], a["G"], *(x.ctypes.data for x in arrays), state, state_bytes, None)
