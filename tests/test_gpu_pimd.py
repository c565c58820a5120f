"""Path-integral MD on the MI355X (torch_m3gnet.path_integral PimdState / pimd_step, C ABI m3g_pimd_*): the kernels against the numpy
restatement (tests/pimd_reference.py) under synthetic forces, bitwise reproducibility and independence of the batch, a non-finite
force on one bead, and graph capture."""
import functools

import numpy as np
import pytest
import torch

import pimd_reference as pr
from test_gpu_dynamics import SEEDS, TEMPS, _forces, _rel

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = [1, 3, 32, 257, 1000]   # one atom, one chunk, a chunk boundary (256 rows + 1), several chunks
SIZES_64 = [1, 3, 257]
# no internal mode; only the k = P/2 mode; odd P; both kinds of mode; odd and one short of a bucket; the edge of the second register
# bucket; the largest
CASES = [(P, SIZES) for P in (1, 2, 3, 4, 7, 16)] + [(64, SIZES_64)]
PARAMS = dict(dt=0.5, centroid_friction=0.02, pile_lambda=0.5)
ITERS = 30


@functools.lru_cache(maxsize=None)
def _rings(sizes, P):
    """Per ring: masses [n], bead positions and velocities [P,n,3] (the beads spread about one configuration, velocities at P T).
    Two correct fp64 implementations differ by the rounding of the stored bead positions, eps |x|, which the next transform sees as
    eps |x| / spread of an internal mode and the springs turn into velocity: about calls * eps * |x| / spread = 30 * 1.1e-16 * 10 /
    0.25 = 1.3e-13 at the end, whatever P and T.  Hence atoms within 10 A of the origin and a spread of 0.25 A for the 1e-12 gate."""
    rng = np.random.default_rng([len(sizes), P])
    out = []
    for n, t in zip(sizes, TEMPS):
        m = rng.uniform(1.0, 200.0, n)
        x = rng.uniform(0, 10.0, (1, n, 3)) + rng.normal(0, 0.25, (P, n, 3))
        v = rng.normal(0, 1.0, (P, n, 3)) * np.sqrt(pr.KB * P * t * pr.KAPPA / m)[None, :, None]
        out.append((m, x, v))
    return out


def _bead_sizes(sizes, P):
    return [n for n in sizes for _ in range(P)]


def _state(thermostat, sizes, P, only=None):
    """The batch's state, or with `only` = g that of its ring g alone."""
    from torch_m3gnet.path_integral import PimdState

    rings, temps, seeds = _rings(tuple(sizes), P), TEMPS[:len(sizes)], SEEDS[:len(sizes)]
    if only is not None:
        rings, temps, seeds, sizes = [rings[only]], [temps[only]], [seeds[only]], [sizes[only]]
    pos = torch.tensor(np.concatenate([x.reshape(-1, 3) for _, x, _ in rings]), dtype=torch.float64, device=DEV)
    vel = torch.tensor(np.concatenate([v.reshape(-1, 3) for _, _, v in rings]), dtype=torch.float64, device=DEV)
    masses = np.concatenate([np.tile(m, P) for m, _, _ in rings])
    offsets = np.concatenate([[0], np.cumsum(_bead_sizes(sizes, P))])
    return PimdState(pos, offsets, masses, vel, temps, seeds, P, thermostat=thermostat, **PARAMS)


def _run(st, sizes, P, iters, nan_at=None, rows=None, snapshot_after=None):
    from torch_m3gnet.path_integral import pimd_step

    obs, snap = [], None
    for k in range(iters):
        f, _ = _forces(_bead_sizes(sizes, P), k, P, nan_at)
        if rows is not None:   # one ring's rows of the batch's inputs
            f = np.ascontiguousarray(f[rows[0]:rows[1]])
        pimd_step(st, torch.tensor(f, device=DEV), finish_only=(k == iters - 1))
        obs.append(st.obs.clone())
        if k == snapshot_after:
            snap = (st.pos.clone(), st.state.clone())
    torch.cuda.synchronize()
    return torch.stack(obs).cpu().numpy(), snap


def _references(thermostat, sizes, P, iters, nan_at=None):
    refs = [pr.PimdReference(x, m, v, t, seed=sd, thermostat=thermostat, **PARAMS)
            for (m, x, v), t, sd in zip(_rings(tuple(sizes), P), TEMPS, SEEDS)]
    offs = P * np.concatenate([[0], np.cumsum(sizes)])
    obs = []
    for k in range(iters):
        f, _ = _forces(_bead_sizes(sizes, P), k, P, nan_at)
        row = []
        for g, ref in enumerate(refs):
            ref.step(f[offs[g]:offs[g + 1]].astype(np.float64).reshape(P, -1, 3), finish_only=(k == iters - 1))
            row.append(ref.obs)
        obs.append(row)
    return refs, np.array(obs)


def _compare(st, obs, refs, ref_obs, sizes, P):
    out = st.read()
    offs = P * np.concatenate([[0], np.cumsum(sizes)])
    pos = st.pos.cpu().numpy()
    worst = (0.0, "")
    for g, ref in enumerate(refs):
        a, b = offs[g], offs[g + 1]
        assert out["flags"][g] == ref.flags and out["n_steps"][g] == ref.n_steps, (g, out["flags"][g], ref.flags, out["n_steps"][g], ref.n_steps)
        errs = {"pos": _rel(pos[a:b], ref.pos.reshape(-1, 3)), "v": _rel(out["v"][a:b], ref.v.reshape(-1, 3), 1e-4),
                "heat": _rel(out["heat"][g:g + 1], np.array([ref.heat]), 1e-6)}
        if not ref.flags & pr.ERROR:
            errs.update({f"obs{j}": _rel(obs[:, g, j], ref_obs[:, g, j], 1e-6) for j in range(6)})
            assert not obs[:, g, 6:].any()
        for key, err in errs.items():
            assert err < 1e-12, (g, key, err)
        worst = max(worst, *((err, f"{key} of ring {g}") for key, err in errs.items()))
    return worst


@pytest.mark.parametrize("thermostat", ["none", "pile_l"])
@pytest.mark.parametrize("P,sizes", CASES)
def test_pimd_kernel_matches_restatement(P, sizes, thermostat):
    st = _state(thermostat, sizes, P)
    obs, _ = _run(st, sizes, P, ITERS)
    refs, ref_obs = _references(thermostat, sizes, P, ITERS)
    worst = _compare(st, obs, refs, ref_obs, sizes, P)
    print(f"P = {P}, {thermostat}: largest relative difference from the restatement {worst[0]:.1e} ({worst[1]})")
    assert all(ref.n_steps == ITERS - 1 for ref in refs)
    heat = st.read()["heat"]
    assert (heat != 0.0).all() if thermostat == "pile_l" else not heat.any()
    if P > 1:
        assert (obs[-1, :, 2] > 0).all()   # the springs hold energy


@pytest.mark.parametrize("P,sizes", [(7, SIZES), (64, SIZES_64)])
def test_pimd_kernel_bitwise_reproducible_and_independent_of_the_batch(P, sizes):
    runs = []
    for _ in range(2):
        st = _state("pile_l", sizes, P)
        runs.append((st, _run(st, sizes, P, 20)[0]))
    (s0, o0), (s1, o1) = runs
    r0, r1 = s0.read(), s1.read()
    assert np.array_equal(o0, o1) and torch.equal(s0.pos, s1.pos) and all(np.array_equal(r0[key], r1[key]) for key in r0)
    offs = P * np.concatenate([[0], np.cumsum(sizes)])
    for g in range(len(sizes)):
        a, b = offs[g], offs[g + 1]
        alone = _state("pile_l", sizes, P, only=g)
        obs, _ = _run(alone, sizes, P, 20, rows=(a, b))
        r = alone.read()
        assert torch.equal(alone.pos, s0.pos[a:b]) and np.array_equal(r["v"], r0["v"][a:b]) and np.array_equal(obs[:, 0], o0[:, g])
        assert r["flags"][0] == r0["flags"][g] and r["n_steps"][0] == r0["n_steps"][g] and r["heat"][0] == r0["heat"][g]


def test_non_finite_force_on_one_bead_freezes_that_ring_only():
    from torch_m3gnet import _lib

    P, iters = 3, 16
    offs = P * np.concatenate([[0], np.cumsum(SIZES)])
    a, b = offs[2], offs[3]
    nan_at = (6, a + 32 + 20)   # call 6: an atom of bead 1 of ring 2
    st = _state("pile_l", SIZES, P)
    obs, snap = _run(st, SIZES, P, iters, nan_at=nan_at, snapshot_after=5)
    refs, ref_obs = _references("pile_l", SIZES, P, iters, nan_at=nan_at)
    _compare(st, obs, refs, ref_obs, SIZES, P)
    r = st.read()
    assert [bool(x & _lib.DYN_ERROR) for x in r["flags"]] == [False, False, True, False, False]
    assert list(r["n_steps"]) == [iters - 1] * 2 + [6] + [iters - 1] * 2
    assert np.array_equal(obs[6:, 2], np.repeat(obs[5:6, 2], iters - 6, axis=0))   # its observables stay those of call 5
    # bitwise where it stood after call 5: every bead's positions and velocities, and the heat
    pos5, state5 = snap
    frozen = _state("pile_l", SIZES, P)
    frozen.state.copy_(state5)
    r5 = frozen.read()
    assert torch.equal(st.pos[a:b], pos5[a:b]) and np.array_equal(r["v"][a:b], r5["v"][a:b]) and r["heat"][2] == r5["heat"][2]
    assert not torch.equal(st.pos[:a], pos5[:a]) and not torch.equal(st.pos[b:], pos5[b:])
    assert torch.isfinite(st.pos).all() and np.isfinite(r["v"]).all()


def test_pimd_step_capture_replays_bitwise():
    from torch_m3gnet.path_integral import pimd_step

    sizes, P = [3, 32, 300], 5
    f, _ = _forces(_bead_sizes(sizes, P), 0, 3)
    forces = torch.tensor(f, device=DEV)
    for thermostat in ("none", "pile_l"):
        eager, graphed = _state(thermostat, sizes, P), _state(thermostat, sizes, P)
        for _ in range(10):
            pimd_step(eager, forces)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            pimd_step(graphed, forces)
        for _ in range(10):
            g.replay()
        torch.cuda.synchronize()
        assert torch.equal(eager.pos, graphed.pos) and torch.equal(eager.obs, graphed.obs)
        re, rg = eager.read(), graphed.read()
        assert all(np.array_equal(re[key], rg[key]) for key in re) and re["n_steps"][0] == 10 and not (re["flags"] & 2).any()
