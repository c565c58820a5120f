"""Batched L-BFGS relaxation on the MI355X (torch_m3gnet.relax.LbfgsState, C ABI m3g_lbfgs_*): the kernels against the numpy
restatement (tests/lbfgs_reference.py), the launch count, bitwise reproducibility and independence of the batch, freezing, errors,
degenerate inputs, and relaxations under the LJ-fitted model through Relaxer(optimizer="lbfgs")."""
import ctypes as C

import numpy as np
import pytest
import torch

import lbfgs_reference as lr
from helpers import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = [1, 3, 32, 257, 1000, 10000]   # one part-filled chunk, a chunk boundary (256 + 1), many chunks
ITERS = 40
# Gate on X (atom rows and cell rows apart), pos and lattice, each relative to its largest entry.  The floor, measured on the CPU with
# these inputs (the restatement against itself with every sum of the two loops reversed; 40 iterations, every size, memory 5 and 100,
# profiles/relax_lbfgs.txt): at most 7.8e-14 absolute (relative 1.6e-15) with the cell fixed and 1.3e-13 absolute (relative 2.7e-15 on
# atom rows up to 49 A) with the cell relaxed.  30 floors = 8e-14 lie below 1e-12, so the gate is the FIRE test's 1e-12.
GATE = 1e-12


class Chain:
    """Physically consistent synthetic forces (or rho would be noise): a seeded anharmonic chain per structure,
    f = -(k_i u + c (2u - u_- - u_+) + u^3 / 2) with u = x - x0 (neighbours along the atom index, periodic within the structure),
    k_i in [1, 20], c = 3, a start displaced by N(0, 0.15); stresses a seeded linear restoring function of the deformation gradient F:
    -A (sym(F) - I - e0) in Voigt order.  With the cell relaxed the chain lives in the generalized coordinates -- x = X_atoms = pos F^-T,
    and the Cartesian forces are f F^-1, so that the generalized forces f F^-1 F are the chain's -- which keeps the field a gradient (a
    chain in pos would couple to F on one side only).  A is of the order of the atom count and e0 of 0.3 / atoms at most: the cell
    rows X = atoms * F then have the curvature and the distance to go of an atom row."""

    def __init__(self, sizes, seed=0):
        rng = np.random.default_rng(seed)
        self.sizes = list(sizes)
        self.offs = np.concatenate([[0], np.cumsum(sizes)])
        self.lats, self.x0, self.start, self.k, self.A, self.e0 = [], [], [], [], [], []
        for n in sizes:
            L = np.eye(3) * (12.0 * n) ** (1 / 3) + rng.normal(0, 0.05, (3, 3))
            x0 = rng.uniform(0, 1, (n, 3)) @ L
            self.lats.append(L)
            self.x0.append(x0)
            self.start.append(x0 + rng.normal(0, 0.15, (n, 3)))
            self.k.append(rng.uniform(1.0, 20.0, (n, 1)))
            self.A.append(n * rng.uniform(4.0, 8.0, 6))   # cell-row curvature 12 A / n of the order of alpha
            self.e0.append(rng.normal(0, 0.01, 6) * min(1.0, 30.0 / n))

    def forces_of(self, i, pos, F):
        u = np.linalg.solve(F, pos.T).T - self.x0[i]
        f = -(self.k[i] * u + 3.0 * (2 * u - np.roll(u, 1, axis=0) - np.roll(u, -1, axis=0)) + 0.5 * u ** 3) @ np.linalg.inv(F)
        e = 0.5 * (F + F.T) - np.eye(3)
        e6 = np.array([e[0, 0], e[1, 1], e[2, 2], e[1, 2], e[2, 0], e[0, 1]])
        return f.astype(np.float32), (-self.A[i] * (e6 - self.e0[i])).astype(np.float32)

    def forces(self, refs, only=None):
        """fp32 forces [N,3] / stresses [S,6] at the restatements' own positions: the SAME arrays go to both sides."""
        fs, ss = zip(*(self.forces_of(i, r.pos, r.F) for i, r in enumerate(refs) if only is None or i in only))
        return np.concatenate(fs), np.stack(ss)

    def references(self, relax_cell, fmax=1e-8, **params):
        return [lr.LbfgsReference(p, L, relax_cell, fmax, **params) for p, L in zip(self.start, self.lats)]


def _state(poss, lats, relax_cell, fmax=1e-8, **params):
    from torch_m3gnet.relax import LbfgsState

    pos = torch.tensor(np.concatenate(poss), dtype=torch.float64, device=DEV)
    lat = torch.tensor(np.stack(lats), dtype=torch.float64, device=DEV)
    return LbfgsState(pos, lat, np.concatenate([[0], np.cumsum([len(p) for p in poss])]), relax_cell=relax_cell, fmax=fmax, **params)


def _step(st, f, s, **kw):
    from torch_m3gnet.relax import lbfgs_step

    lbfgs_step(st, torch.tensor(f, device=DEV), torch.tensor(s, device=DEV), **kw)


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


_TRAJECTORIES = {}


def _trajectory(relax_cell, memory, only=None):
    """ITERS calls on the device and on the restatement over the same fp32 inputs; `only`: those structures of SIZES, as a batch of
    their own, with the inputs they had inside the whole batch (the restatement does not depend on the batch).  Computed once."""
    key = (relax_cell, memory, only)
    if key in _TRAJECTORIES:
        return _TRAJECTORIES[key]
    from torch_m3gnet import _lib

    chain = Chain(SIZES)
    refs = chain.references(relax_cell, memory=memory)
    pick = list(range(len(SIZES))) if only is None else list(only)
    st = _state([chain.start[i] for i in pick], [chain.lats[i] for i in pick], relax_cell, memory=memory)
    for k in range(ITERS):
        f, s = chain.forces(refs, only=None if only is None else set(only))
        _step(st, f, s)
        full_f, full_s = (f, s) if only is None else chain.forces(refs)
        for i, ref in enumerate(refs):
            a, b = chain.offs[i], chain.offs[i + 1]
            ref.step(full_f[a:b].astype(np.float64), full_s[i].astype(np.float64))
    torch.cuda.synchronize()
    _TRAJECTORIES[key] = (chain, refs, st, st.read(), st.pos.cpu().numpy(), st.lattice.cpu().numpy())
    return _TRAJECTORIES[key]


@pytest.mark.parametrize("memory", [5, 100])
@pytest.mark.parametrize("relax_cell", [False, True])
def test_lbfgs_kernels_match_restatement(relax_cell, memory):
    from torch_m3gnet import _lib

    chain, refs, st, out, pos, lat = _trajectory(relax_cell, memory)
    N = chain.offs[-1]
    for i, ref in enumerate(refs):
        a, b = chain.offs[i], chain.offs[i + 1]
        err = [_rel(out["x"][a:b], ref.X[: b - a]), _rel(pos[a:b], ref.pos), _rel(lat[i], ref.lattice)]
        if relax_cell:
            err.append(_rel(out["x"][N + 3 * i:N + 3 * i + 3], ref.X[b - a:]))
        print(f"relax_cell={relax_cell} memory={memory} n={b - a}: flags {out['flags'][i]} steps {out['n_steps'][i]} pairs {out['n_pairs'][i]} "
              f"clipped {ref.clipped} wrapped {ref.wrapped} rejected {ref.rejected} rel err X / pos / lattice / X cell " + " ".join(f"{e:.1e}" for e in err))
        assert out["flags"][i] == ref.flags and out["n_steps"][i] == ref.n_steps and out["n_pairs"][i] == ref.n_pairs, i
        assert max(err) < GATE, (i, err)
    assert any(ref.clipped for ref in refs)
    if memory == 5:
        assert all(ref.wrapped for ref in refs[2:]) and all(ref.n_pairs == 5 for ref in refs[2:])
    else:
        assert max(ref.n_pairs for ref in refs) > 30   # the history deepened
    assert not relax_cell or np.abs(lat - np.stack(chain.lats)).max() > 1e-4
    assert st.n_unconverged == sum(1 for ref in refs if not ref.flags & (lr.CONVERGED | lr.ERROR)) == len(SIZES) - 2
    # the 1- and 3-atom structures converged (fp32 forces far below fmax); two more calls, now with large forces on every atom, leave
    # them bitwise where they were while the others move  (last: the cached trajectory is final from here on)
    assert all(out["flags"][i] & _lib.LBFGS_CONVERGED and out["n_steps"][i] < ITERS for i in (0, 1)), (out["flags"], out["n_steps"])
    rng = np.random.default_rng(11)
    for _ in range(2):
        _step(st, rng.normal(0, 5.0, (N, 3)).astype(np.float32), rng.normal(0, 0.5, (len(SIZES), 6)).astype(np.float32))
    after, pos2, lat2 = st.read(), st.pos.cpu().numpy(), st.lattice.cpu().numpy()
    assert np.array_equal(pos2[:4], pos[:4]) and np.array_equal(lat2[:2], lat[:2]) and np.array_equal(after["x"][:4], out["x"][:4])
    assert np.array_equal(after["x"][N:N + 6], out["x"][N:N + 6])
    for key in ("flags", "n_steps", "n_pairs"):
        assert np.array_equal(after[key][:2], out[key][:2]), key
    assert np.array_equal(after["n_steps"][2:], out["n_steps"][2:] + 2) and not np.array_equal(pos2[4:], pos[4:])


def test_lbfgs_bitwise_reproducible_and_independent_of_the_batch():
    first = _trajectory(True, 5)
    _TRAJECTORIES.pop((True, 5, None))
    again = _trajectory(True, 5)
    for key in ("flags", "n_steps", "n_pairs", "x"):
        assert np.array_equal(first[3][key], again[3][key]), key
    assert np.array_equal(first[4], again[4]) and np.array_equal(first[5], again[5])
    # structure 2 (32 atoms) and 4 (1,000 atoms) alone, with the same inputs as inside the batch
    chain, _, _, batch, pos, lat = first
    N = chain.offs[-1]
    for i in (2, 4):
        a, b = chain.offs[i], chain.offs[i + 1]
        _, _, _, alone, pos1, lat1 = _trajectory(True, 5, only=(i,))
        assert np.array_equal(pos1, pos[a:b]) and np.array_equal(lat1[0], lat[i])
        assert np.array_equal(alone["x"][: b - a], batch["x"][a:b]) and np.array_equal(alone["x"][b - a:], batch["x"][N + 3 * i:N + 3 * i + 3])
        for key in ("flags", "n_steps", "n_pairs"):
            assert alone[key][0] == batch[key][i], key


def test_lbfgs_step_is_five_launches_whatever_memory_depth_and_batch():
    """The launch sequence of one m3g_lbfgs_step captured (not executed) on a side stream, its nodes counted: five kernels at memory 5
    and 100, at history depth 0 and 3, for one structure and for six; three with check_only."""
    from torch_m3gnet.relax import lbfgs_step

    hip = C.CDLL("libamdhip64.so")
    graph_nodes = hip.hipGraphGetNodes
    graph_nodes.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]

    def count(st, f, s, check_only=False):
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        graph, n = C.c_void_p(), C.c_size_t()
        with torch.cuda.stream(stream):
            assert hip.hipStreamBeginCapture(C.c_void_p(stream.cuda_stream), 2) == 0   # relaxed mode: this thread's other calls go on
            try:
                lbfgs_step(st, f, s, check_only=check_only)
            finally:
                assert hip.hipStreamEndCapture(C.c_void_p(stream.cuda_stream), C.byref(graph)) == 0
        assert graph_nodes(graph, None, C.byref(n)) == 0
        hip.hipGraphDestroy(graph)
        return n.value

    for sizes in ([40], SIZES):
        chain = Chain(sizes, seed=2)
        for memory in (5, 100):
            refs = chain.references(True, memory=memory)
            st = _state(chain.start, chain.lats, True, memory=memory)
            f, s = (torch.tensor(x, device=DEV) for x in chain.forces(refs))
            assert count(st, f, s) == 5 and count(st, f, s, check_only=True) == 3
            for _ in range(4):
                _step(st, *chain.forces(refs))
                for i, ref in enumerate(refs):
                    ref.step(*(x.astype(np.float64) for x in chain.forces_of(i, ref.pos, ref.F)))
            assert st.read()["n_pairs"].max() == 3
            f, s = (torch.tensor(x, device=DEV) for x in chain.forces(refs))
            assert count(st, f, s) == 5


def test_converged_structure_is_frozen_while_another_steps():
    from torch_m3gnet import _lib

    chain = Chain([32, 32], seed=4)
    refs = chain.references(True, fmax=1e-2)
    st = _state(chain.start, chain.lats, True, fmax=1e-2)
    snaps = []
    for k in range(12):
        f, s = chain.forces(refs)
        if k >= 4:   # structure 0: forces and stresses far below fmax from here on
            f[:32] *= 1e-6
            s[0] *= 1e-6
        _step(st, f, s)
        for i, ref in enumerate(refs):
            ref.step(f[32 * i:32 * i + 32].astype(np.float64), s[i].astype(np.float64))
        torch.cuda.synchronize()
        snaps.append((st.pos.clone(), st.lattice.clone(), st.read(), st.n_unconverged))
    p4, l4, r4, _ = snaps[4]
    assert r4["flags"][0] & _lib.LBFGS_CONVERGED and r4["n_steps"][0] == 4 and r4["n_pairs"][0] == 3
    for p, l, r, unconv in snaps[4:]:
        assert torch.equal(p[:32], p4[:32]) and torch.equal(l[0], l4[0])
        assert r["n_steps"][0] == 4 and r["n_pairs"][0] == 3 and np.array_equal(r["x"][:32], r4["x"][:32]) and np.array_equal(r["x"][64:67], r4["x"][64:67])
        assert unconv == 1   # the pinned count
    assert snaps[-1][2]["n_steps"][1] == 12 and not torch.equal(snaps[-1][0][32:], p4[32:])


def test_non_finite_inputs_flag_those_structures_only():
    from torch_m3gnet import _lib

    chain = Chain([3, 32, 1000], seed=5)
    refs = chain.references(True)
    st = _state(chain.start, chain.lats, True)
    pos, lat = st.pos, st.lattice
    for k in range(10):
        f, s = chain.forces(refs)
        if k == 4:
            f[3 + 7, 1] = np.nan
        if k == 6:
            s[2, 3] = np.inf
        if k in (4, 6):
            before = (pos.clone(), lat.clone())
        _step(st, f, s)
        for i, ref in enumerate(refs):
            ref.step(f[chain.offs[i]:chain.offs[i + 1]].astype(np.float64), s[i].astype(np.float64))
        if k == 4:
            torch.cuda.synchronize()
            assert torch.equal(pos[3:35], before[0][3:35]) and torch.equal(lat[1], before[1][1])
        if k == 6:
            torch.cuda.synchronize()
            assert torch.equal(pos[35:], before[0][35:]) and torch.equal(lat[2], before[1][2])
    r = st.read()
    assert [bool(x & _lib.LBFGS_ERROR) for x in r["flags"]] == [False, True, True]
    assert list(r["n_steps"][1:]) == [4, 6] and r["n_steps"][0] == refs[0].n_steps
    assert torch.isfinite(pos).all() and torch.isfinite(lat).all()
    assert st.n_unconverged == (0 if refs[0].converged else 1)


def test_equal_forces_twice_store_no_pair():
    chain = Chain([3, 300], seed=6)
    refs = chain.references(False, fmax=1e-8)
    st = _state(chain.start, chain.lats, False, fmax=1e-8)
    f, s = chain.forces(refs)
    for k in range(3):   # the same arrays three times: y = 0 at the second and third call
        _step(st, f, s)
        for i, ref in enumerate(refs):
            ref.step(f[chain.offs[i]:chain.offs[i + 1]].astype(np.float64))
    out = st.read()
    pos = st.pos.cpu().numpy()
    assert list(out["n_pairs"]) == [0, 0] == [ref.n_pairs for ref in refs] and list(out["n_steps"]) == [3, 3]
    assert [ref.rejected for ref in refs] == [2, 2]
    for i, ref in enumerate(refs):
        a, b = chain.offs[i], chain.offs[i + 1]
        assert out["flags"][i] == ref.flags and _rel(out["x"][a:b], ref.X) < GATE and _rel(pos[a:b], ref.pos) < GATE
    assert np.isfinite(pos).all()
    # ... and a fresh pair after it is stored again
    f2, s2 = chain.forces(refs)
    _step(st, f2, s2)
    assert list(st.read()["n_pairs"]) == [1, 1]


def test_one_huge_force_moves_that_atom_by_maxstep():
    chain = Chain([5, 300], seed=7)
    refs = chain.references(False)
    st = _state(chain.start, chain.lats, False)
    f, s = chain.forces(refs)
    f[2] = [3e6, -4e6, 0.0]
    f[5 + 260] = [0.0, 0.0, -7e5]   # (in the second chunk of the second structure)
    before = st.pos.cpu().numpy()
    _step(st, f, s)
    moved = np.linalg.norm(st.pos.cpu().numpy() - before, axis=1)
    for at, (a, b) in ((2, (0, 5)), (265, (5, 305))):
        assert abs(moved[at] - 0.2) < 1e-12 * 0.2 and moved[a:b].argmax() == at - a
        others = np.delete(moved[a:b], at - a)
        assert 0 < others.max() < 1e-3


# ---- physics under the LJ-fitted model ---------------------------------------------------------------------------------------------
FCC_BASE = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])


def _model():
    from torch_m3gnet.model.build import build_model_from_npz

    return build_model_from_npz(GOLDEN / "model_fitted_lj.npz").to(DEV)


def _fcc(a, n=2):
    grid = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1).reshape(-1, 1, 3)
    return (grid + FCC_BASE[None]).reshape(-1, 3) * a, np.eye(3) * n * a


def test_fixed_cell_relaxation_returns_to_perfect_fcc_in_fewer_steps_than_fire():
    from torch_m3gnet.relax import Relaxer

    model = _model()
    pos0, lat = _fcc(3.45)
    pos = pos0 + np.random.default_rng(7).normal(0, 0.05, pos0.shape)
    args = ([lat], [pos], [np.full(32, 29)])
    (res,) = Relaxer(model, relax_cell=False, optimizer="lbfgs").relax(*args, fmax=0.002, steps=500)
    assert res["converged"] and not res["error"] and 0 < res["n_steps"] < 500
    assert np.sqrt((res["forces"] ** 2).sum(1).max()) < 0.01
    assert np.array_equal(res["lattice"], lat)
    shift = (pos - pos0).mean(0)   # every s and y sums to zero over the atoms when the forces do
    assert np.abs(res["positions"] - (pos0 + shift)).max() < 1e-3
    (fire,) = Relaxer(model, relax_cell=False, optimizer="fire").relax(*args, fmax=0.002, steps=500)
    print(f"fixed cell, fmax 0.002: L-BFGS {res['n_steps']} steps, FIRE {fire['n_steps']} steps")
    assert fire["converged"] and res["n_steps"] < fire["n_steps"]


def test_variable_cell_relaxation_reaches_the_models_lattice_constant():
    from torch_m3gnet.data import MaterialGraphKey as K
    from torch_m3gnet.data.md import VerletGraph
    from torch_m3gnet.nn import Gradient
    from torch_m3gnet.relax import Relaxer

    model = _model()
    pv = Gradient(model.model, pair_virial=True)
    z = np.full(32, 29)
    grid_a = np.linspace(3.48, 3.53, 11)
    e = []
    for a in grid_a:
        p, L = _fcc(a)
        vg = VerletGraph([L], [z], 5.0, 4.0, skin=0.5, device=DEV)
        e.append(float(vg.step(pv, torch.tensor(p, device=DEV))[K.TOTAL_ENERGY][0]) / 32)
    c2, c1, _ = np.polyfit(grid_a, e, 2)
    a0 = -c1 / (2 * c2)
    assert 3.48 < a0 < 3.53 and c2 > 0
    pos, lat = _fcc(3.46)
    pos = pos + np.random.default_rng(8).normal(0, 0.03, pos.shape)
    (res,) = Relaxer(model, relax_cell=True, optimizer="lbfgs").relax([lat], [pos], [z], fmax=0.01, steps=500)
    print(f"variable cell, fmax 0.01: L-BFGS {res['n_steps']} steps")
    assert res["converged"] and not res["error"], res["n_steps"]
    L = res["lattice"]
    assert np.abs(L - np.diag(np.diag(L))).max() < 2e-3   # stays cubic
    assert np.abs(np.diag(L) / 2 - a0).max() < 2e-3, (np.diag(L) / 2, a0)


def test_out_of_range_species_raises():
    from torch_m3gnet.relax import Relaxer

    pos, lat = _fcc(3.5)
    z = np.full(32, 29)
    z[3] = 200
    with pytest.raises((IndexError, ValueError)):
        Relaxer(_model(), optimizer="lbfgs").relax([lat], [pos], [z], steps=3)
