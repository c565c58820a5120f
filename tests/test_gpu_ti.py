"""Thermodynamic integration to an Einstein crystal on the MI355X (torch_m3gnet.free_energy TiState / ti_path / ti_step, C ABI
m3g_ti_*): the kernels against the numpy restatement (tests/ti_reference.py) under synthetic forces and energies across a change of
path, bitwise reproducibility and independence of the batch, a non-finite force or energy on one structure, and graph capture."""
import functools

import numpy as np
import pytest
import torch

import ti_reference as tr
from test_gpu_dynamics import SEEDS, TEMPS, _forces, _rel

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = [2, 3, 32, 257, 1000]   # the smallest legal structure, one chunk, a chunk boundary (256 rows + 1), several chunks
ITERS, SWAP = 30, 15            # calls in all; the call before which the second path starts (a step is under way then)
# per structure (lambda_b, lambda_e): both directions, fixed coupling, part of the range; then (n_switch, n_discard)
PATH_A = (np.array([1.0, 0.0, 0.3, 1.0, 0.2]), np.array([0.0, 1.0, 0.3, 0.5, 0.9]), 10, 3)
PATH_B = (np.array([0.0, 1.0, 0.8, 0.5, 0.9]), np.array([1.0, 0.0, 0.8, 1.0, 0.2]), 8, 0)


@functools.lru_cache(maxsize=None)
def _systems(sizes):
    """Per structure: masses, springs [n] (atom 0 of the larger ones untied), sites, positions and velocities [n,3].
    Two correct fp64 implementations differ by the rounding of the stored positions, eps |x|, which u = x - r0 turns into eps |x| / |u|
    of the spring force, the spring energy and the per-atom sums: about calls * eps * |x| / spread = 30 * 1.1e-16 * 8.7 / 0.2 = 1.4e-13
    at the end.  Hence sites within 5 A of the origin along every axis and a spread of 0.2 A for the 1e-12 gate.  The synthetic
    energies are negative, so dH/dlambda = E - U_s and the work along a monotonic path never cancel."""
    rng = np.random.default_rng([len(sizes), 41])
    out = []
    for n, t in zip(sizes, TEMPS):
        m = rng.uniform(1.0, 200.0, n)
        k = rng.uniform(0.5, 8.0, n)
        if n > 2:
            k[0] = 0.0
        r0 = rng.uniform(0.0, 5.0, (n, 3))
        x = r0 + rng.normal(0, 0.2, (n, 3))
        v = rng.normal(0, 1.0, (n, 3)) * np.sqrt(tr.KB * t * tr.KAPPA / m)[:, None]
        out.append((m, k, r0, x, v))
    return out


def _inputs(sizes, k, seed, nan_at=None, nan_energy_at=None):
    """forces [N,3] and energies [S] float32 of call k."""
    f, _ = _forces(sizes, k, seed, nan_at)
    e = (-(1.0 + np.abs(np.random.default_rng([seed, k, 99]).normal(size=len(sizes)))) * np.array(sizes)).astype(np.float32)
    if nan_energy_at is not None and k == nan_energy_at[0]:
        e[nan_energy_at[1]] = np.nan
    return f, e


def _state(schedule, friction, sizes, only=None):
    """The batch's state, or with `only` = g that of its structure g alone."""
    from torch_m3gnet.free_energy import TiState

    systems, temps, seeds = _systems(tuple(sizes)), TEMPS[:len(sizes)], SEEDS[:len(sizes)]
    if only is not None:
        systems, temps, seeds, sizes = [systems[only]], [temps[only]], [seeds[only]], [sizes[only]]
    cat = lambda j: np.concatenate([s[j] for s in systems])   # noqa: E731
    f64 = dict(dtype=torch.float64, device=DEV)
    return TiState(torch.tensor(cat(3), **f64), np.concatenate([[0], np.cumsum(sizes)]), cat(0), cat(1), torch.tensor(cat(4), **f64),
                   torch.tensor(cat(2), **f64), temps, seeds, schedule=schedule, dt=1.0, friction=friction)


def _pick(path, only, n_structs):
    lb, le, n_switch, n_discard = path
    rows = slice(0, n_structs) if only is None else slice(only, only + 1)
    return lb[rows], le[rows], n_switch, n_discard


def _run(st, sizes, iters, only=None, snapshot_after=None, **bad):
    """`iters` calls, PATH_A from the start and PATH_B from call SWAP on; `only`: structure g's share of the batch's inputs."""
    from torch_m3gnet.free_energy import ti_path, ti_step

    offs = np.concatenate([[0], np.cumsum(sizes)])
    obs, snap = [], None
    ti_path(st, *_pick(PATH_A, only, len(sizes)))
    for k in range(iters):
        if k == SWAP:
            ti_path(st, *_pick(PATH_B, only, len(sizes)))
        f, e = _inputs(sizes, k, 5, **bad)
        if only is not None:
            f, e = np.ascontiguousarray(f[offs[only]:offs[only + 1]]), e[only:only + 1]
        ti_step(st, torch.tensor(f, device=DEV), torch.tensor(e, device=DEV), finish_only=(k == iters - 1))
        obs.append(st.obs.clone())
        if k == snapshot_after:
            snap = (st.pos.clone(), st.state.clone())
    torch.cuda.synchronize()
    return torch.stack(obs).cpu().numpy(), snap


def _references(schedule, friction, sizes, iters, **bad):
    refs = [tr.TiReference(x, m, k, v, r0, t, seed=sd, schedule=schedule, dt=1.0, friction=friction)
            for (m, k, r0, x, v), t, sd in zip(_systems(tuple(sizes)), TEMPS, SEEDS)]
    offs = np.concatenate([[0], np.cumsum(sizes)])
    obs = []
    for k in range(iters):
        for path in ((PATH_A,) if k == 0 else (PATH_B,) if k == SWAP else ()):
            for g, ref in enumerate(refs):
                ref.path(path[0][g], path[1][g], path[2], path[3])
        f, e = _inputs(sizes, k, 5, **bad)
        row = []
        for g, ref in enumerate(refs):
            ref.step(f[offs[g]:offs[g + 1]].astype(np.float64), float(e[g]), finish_only=(k == iters - 1))
            row.append(ref.obs)
        obs.append(row)
    return refs, np.array(obs)


def _compare(st, obs, refs, ref_obs, sizes):
    out = st.read()
    offs = np.concatenate([[0], np.cumsum(sizes)])
    pos = st.pos.cpu().numpy()
    worst = (0.0, "")
    for g, ref in enumerate(refs):
        a, b = offs[g], offs[g + 1]
        assert out["flags"][g] == ref.flags and out["n_steps"][g] == ref.n_steps and out["count"][g] == ref.count, (g, out["flags"][g], ref.flags)
        one = lambda key, x: _rel(out[key][g:g + 1], np.array([x]), 1e-6)   # noqa: E731
        errs = {"pos": _rel(pos[a:b], ref.pos), "v": _rel(out["v"][a:b], ref.v, 1e-4), "work": one("work", ref.work),
                "mean": one("mean", ref.mean), "m2": one("m2", ref.m2), "msd_sum": _rel(out["msd_sum"][a:b], ref.msd_sum, 1e-6)}
        if not ref.flags & tr.ERROR:
            errs.update({f"obs{j}": _rel(obs[:, g, j], ref_obs[:, g, j], 1e-6) for j in range(6)})
            assert not obs[:, g, 6:].any()
        for key, err in errs.items():
            assert err < 1e-12, (g, key, err)
        worst = max(worst, *((err, f"{key} of structure {g}") for key, err in errs.items()))
    return worst


@pytest.mark.parametrize("friction", [0.0, 0.02])
@pytest.mark.parametrize("schedule", ["linear", "smooth"])
def test_ti_kernel_matches_restatement(schedule, friction):
    st = _state(schedule, friction, SIZES)
    obs, _ = _run(st, SIZES, ITERS)
    refs, ref_obs = _references(schedule, friction, SIZES, ITERS)
    worst = _compare(st, obs, refs, ref_obs, SIZES)
    print(f"{schedule}, friction {friction}: largest relative difference from the restatement {worst[0]:.1e} ({worst[1]})")
    out = st.read()
    assert all(ref.n_steps == ITERS - 1 for ref in refs) and list(out["count"]) == [ITERS - SWAP] * len(SIZES)
    assert (out["work"][[0, 1, 3, 4]] != 0.0).all() and out["work"][2] == 0.0 and (out["msd_sum"] > 0).all()
    lam = obs[:, :, 4]
    assert np.array_equal(lam[0], PATH_A[0]) and np.array_equal(lam[SWAP - 1], PATH_A[1]) and np.array_equal(lam[SWAP], PATH_B[0])
    assert np.array_equal(lam[-1], PATH_B[1])


@pytest.mark.parametrize("friction", [0.0, 0.02])
def test_ti_centre_of_mass_momentum_only_decays(friction):
    """sum_i m_i v_i changes by no force and no noise: after k steps it is c1^k times what it was (the synthetic starts carry some)."""
    st = _state("smooth", friction, SIZES)
    systems = _systems(tuple(SIZES))
    _run(st, SIZES, ITERS)
    v = st.read()["v"]
    offs = np.concatenate([[0], np.cumsum(SIZES)])
    for g, (m, _, _, _, v0) in enumerate(systems):
        p0, p1 = (m[:, None] * v0).sum(0), (m[:, None] * v[offs[g]:offs[g + 1]]).sum(0)
        scale = np.abs(m[:, None] * v0).sum()
        assert np.abs(p1 - np.exp(-friction * (ITERS - 1)) * p0).max() < 1e-12 * scale, (g, p0, p1)


def test_ti_kernel_bitwise_reproducible_and_independent_of_the_batch():
    runs = []
    for _ in range(2):
        st = _state("smooth", 0.02, SIZES)
        runs.append((st, _run(st, SIZES, 20)[0]))
    (s0, o0), (s1, o1) = runs
    r0, r1 = s0.read(), s1.read()
    assert np.array_equal(o0, o1) and torch.equal(s0.pos, s1.pos) and all(np.array_equal(r0[key], r1[key]) for key in r0)
    offs = np.concatenate([[0], np.cumsum(SIZES)])
    for g in range(len(SIZES)):
        a, b = offs[g], offs[g + 1]
        alone = _state("smooth", 0.02, SIZES, only=g)
        obs, _ = _run(alone, SIZES, 20, only=g)
        r = alone.read()
        assert torch.equal(alone.pos, s0.pos[a:b]) and np.array_equal(obs[:, 0], o0[:, g])
        assert np.array_equal(r["v"], r0["v"][a:b]) and np.array_equal(r["msd_sum"], r0["msd_sum"][a:b])
        assert all(r[key][0] == r0[key][g] for key in ("flags", "n_steps", "work", "count", "mean", "m2"))


@pytest.mark.parametrize("what", ["force", "energy"])
def test_non_finite_force_or_energy_freezes_that_structure_only(what):
    from torch_m3gnet import _lib

    iters = 20
    offs = np.concatenate([[0], np.cumsum(SIZES)])
    a, b = offs[2], offs[3]
    bad = dict(nan_at=(6, a + 20)) if what == "force" else dict(nan_energy_at=(6, 2))   # call 6: structure 2
    st = _state("smooth", 0.02, SIZES)
    obs, snap = _run(st, SIZES, iters, snapshot_after=5, **bad)
    refs, ref_obs = _references("smooth", 0.02, SIZES, iters, **bad)
    _compare(st, obs, refs, ref_obs, SIZES)
    r = st.read()
    assert [bool(x & _lib.DYN_ERROR) for x in r["flags"]] == [False, False, True, False, False]
    assert list(r["n_steps"]) == [iters - 1] * 2 + [6] + [iters - 1] * 2
    assert np.array_equal(obs[6:, 2], np.repeat(obs[5:6, 2], iters - 6, axis=0))   # its observables stay those of call 5
    # bitwise where it stood after call 5, through the change of path at call 15 too
    pos5, state5 = snap
    frozen = _state("smooth", 0.02, SIZES)
    frozen.state.copy_(state5)
    r5 = frozen.read()
    assert torch.equal(st.pos[a:b], pos5[a:b]) and np.array_equal(r["v"][a:b], r5["v"][a:b]) and np.array_equal(r["msd_sum"][a:b], r5["msd_sum"][a:b])
    assert all(r[key][2] == r5[key][2] for key in ("work", "count", "mean", "m2")) and r["count"][2] == 3
    assert not torch.equal(st.pos[:a], pos5[:a]) and not torch.equal(st.pos[b:], pos5[b:])
    assert torch.isfinite(st.pos).all() and np.isfinite(r["v"]).all()


def test_ti_step_capture_replays_bitwise():
    from torch_m3gnet.free_energy import ti_path, ti_step

    sizes = [2, 32, 300]
    f, e = _inputs(sizes, 0, 3)
    forces, energies = torch.tensor(f, device=DEV), torch.tensor(e, device=DEV)
    for friction in (0.0, 0.02):
        eager, graphed = _state("smooth", friction, sizes), _state("smooth", friction, sizes)
        for st in (eager, graphed):
            ti_path(st, [1.0, 0.0, 0.5], [0.0, 1.0, 0.5], 6, 2)
        for _ in range(10):
            ti_step(eager, forces, energies)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            ti_step(graphed, forces, energies)
        for _ in range(10):
            g.replay()
        torch.cuda.synchronize()
        assert torch.equal(eager.pos, graphed.pos) and torch.equal(eager.obs, graphed.obs)
        re, rg = eager.read(), graphed.read()
        assert all(np.array_equal(re[key], rg[key]) for key in re) and re["n_steps"][0] == 10 and not (re["flags"] & 2).any()
        assert list(re["count"]) == [8] * 3 and re["work"][0] != 0.0
