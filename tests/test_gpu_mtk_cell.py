"""Flexible-cell MTK NPT on the MI355X (torch_m3gnet.dynamics MtkCellState / mtk_cell_step, C ABI m3g_mtk_*): the kernels against the
numpy restatement (tests/mtk_cell_reference.py), the second trip of the wave's loop over chunks, bitwise reproducibility and
independence of the batch, freezing on a non-finite force and on a cell rate past the series' range, graph capture, guard bands
round the state, and runs under the LJ-fitted model: a sheared cell swinging back through cubic, an orthorhombic cell keeping its
axes, the conserved quantity against the isotropic family's, and no stale neighbour list over a change of shape."""
import functools

import numpy as np
import pytest
import torch

import mtk_cell_reference as mr
from test_gpu_dynamics import _batch, _fcc, _fitted_model, _forces, _rel
from test_gpu_nhc import PARAMS, TEMPS

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = [2, 3, 40, 257, 769]   # one chunk, a chunk boundary (256 rows + 1), three chunks + 1
MASKS = ["full", "orthorhombic"]
CASES = [(mask, fc, chain) for mask in MASKS for fc in (False, True) for chain in ((1, 1), (3, 2))]


def _state(mask, fix_com, sizes, chain=(3, 1), only=None, temps=None):
    """The batch's state, or with `only` = i that of its structure i alone."""
    from torch_m3gnet.dynamics import MtkCellState

    lats, poss, ms, vs = _batch(sizes, 0)
    temps = (TEMPS * 2)[:len(sizes)] if temps is None else temps
    if only is not None:
        lats, poss, ms, vs, temps, sizes = [lats[only]], [poss[only]], [ms[only]], [vs[only]], [temps[only]], [sizes[only]]
    pos = torch.tensor(np.concatenate(poss), dtype=torch.float64, device=DEV)
    lat = torch.tensor(np.stack(lats), dtype=torch.float64, device=DEV)
    vel = torch.tensor(np.concatenate(vs), dtype=torch.float64, device=DEV)
    return MtkCellState(pos, lat, np.concatenate([[0], np.cumsum(sizes)]), np.concatenate(ms), vel, temps, cell_mask=mask, fix_com=fix_com,
                        chain_length=chain[0], chain_substeps=chain[1], **PARAMS)


def _inputs(sizes, k, nan_at=None, stress_at=None):
    """The forces and stresses of call k; `nan_at` = (call, atom) a NaN force, `stress_at` = (call, structure) a stress of 10 eV/A^3:
    finite, and some ten thousand times what keeps the cell rate within the series' range."""
    f, s = _forces(sizes, k, 0, nan_at)
    if stress_at is not None and k == stress_at[0]:
        s[stress_at[1], 5] = 10.0
    return f, s


def _run(st, sizes, iters, rows=None, snapshot_after=None, **bad):
    from torch_m3gnet.dynamics import mtk_cell_step

    obs, snap = [], None
    for k in range(iters):
        f, s = _inputs(sizes, k, **bad)
        if rows is not None:   # one structure's rows of the batch's inputs
            (a, b), i = rows
            f, s = np.ascontiguousarray(f[a:b]), np.ascontiguousarray(s[i:i + 1])
        mtk_cell_step(st, torch.tensor(f, device=DEV), torch.tensor(s, device=DEV), finish_only=(k == iters - 1))
        obs.append(st.obs.clone())
        if k == snapshot_after:
            snap = (st.pos.clone(), st.lattice.clone(), st.state.clone())
    torch.cuda.synchronize()
    return torch.stack(obs).cpu().numpy(), snap


def _references(mask, fix_com, sizes, iters, chain=(3, 1), **bad):
    lats, poss, ms, vs = _batch(sizes, 0)
    refs = [mr.MtkCellReference(p, L, m, v, mask, temperature=t, fix_com=fix_com, chain_length=chain[0], chain_substeps=chain[1], **PARAMS)
            for p, L, m, v, t in zip(poss, lats, ms, vs, TEMPS * 2)]
    offs = np.concatenate([[0], np.cumsum(sizes)])
    obs = []
    for k in range(iters):
        f, s = _inputs(sizes, k, **bad)
        row = []
        for i, ref in enumerate(refs):
            ref.step(f[offs[i]:offs[i + 1]].astype(np.float64), s[i].astype(np.float64), finish_only=(k == iters - 1))
            row.append(ref.obs)
        obs.append(row)
    return refs, np.array(obs)


def _compare(st, obs, refs, ref_obs, sizes):
    """Every gate is 1e-12; returns the largest relative difference met."""
    worst = []

    def rel(a, b, floor=1e-300):
        worst.append(_rel(a, b, floor))
        return worst[-1]

    out = st.read()
    offs = np.concatenate([[0], np.cumsum(sizes)])
    pos, lat = st.pos.cpu().numpy(), st.lattice.cpu().numpy()
    M = st.chain_length
    for i, ref in enumerate(refs):
        a, b = offs[i], offs[i + 1]
        assert out["flags"][i] == ref.flags and out["n_steps"][i] == ref.n_steps, (i, out["flags"][i], ref.flags, out["n_steps"][i], ref.n_steps)
        assert rel(pos[a:b], ref.pos) < 1e-12, (i, rel(pos[a:b], ref.pos))
        assert rel(out["v"][a:b], ref.v, 1e-4) < 1e-12, (i, rel(out["v"][a:b], ref.v, 1e-4))
        assert rel(lat[i], ref.lattice) < 1e-12, (i, rel(lat[i], ref.lattice))
        chain = ref.chain_row()
        assert out["chain"][i].shape == (4 * M + 6,) and rel(out["chain"][i], chain) < 1e-12, (i, out["chain"][i], chain)
        assert rel(out["chain"][i][4 * M:], chain[4 * M:]) < 1e-12, (i, out["chain"][i], chain)   # vg on its own scale
        called = np.isfinite(ref_obs[:, i, 0])   # (a structure flagged at its first call has no row yet)
        for j in range(12):
            if j != 5:
                assert rel(obs[called, i, j], ref_obs[called, i, j]) < 1e-12, (i, j, rel(obs[called, i, j], ref_obs[called, i, j]))
        assert not obs[called, i, 5].any()
    return max(worst)


def _cell_strain(st, sizes):
    """lattice0^-1 lattice of every structure: what the run multiplied the cells by."""
    return np.stack([np.linalg.solve(L0, L) for L0, L in zip(_batch(sizes, 0)[0], st.lattice.cpu().numpy())])


@pytest.mark.parametrize("mask,fix_com,chain", CASES)
def test_mtk_kernel_matches_restatement(mask, fix_com, chain):
    iters = 40
    st = _state(mask, fix_com, SIZES, chain)
    obs, _ = _run(st, SIZES, iters)
    refs, ref_obs = _references(mask, fix_com, SIZES, iters, chain)
    worst = _compare(st, obs, refs, ref_obs, SIZES)
    print(f"{mask}, fix_com {fix_com}, chain {chain}: largest relative difference from the restatement {worst:.1e} (gate 1e-12)")
    assert all(ref.n_steps == iters - 1 and not ref.flags & mr.ERROR for ref in refs)
    assert max(ref.max_rate for ref in refs) < 0.02 and any(abs(ref.lam - 1.0) > 1e-6 for ref in refs)   # far from the rate limit
    assert torch.equal(st.lattice32, st.lattice.to(torch.float32))
    strain = _cell_strain(st, SIZES)
    off = np.abs(strain[:, [0, 0, 1, 1, 2, 2], [1, 2, 0, 2, 0, 1]]).max(1)
    assert (np.abs(np.diagonal(strain, axis1=1, axis2=2) - 1.0).max(1) > 1e-6).all()
    if mask == "full":
        assert (off > 1e-6).all(), off   # the shape moved
    else:
        assert (off < 1e-12).all(), off


def test_mtk_kernel_second_trip_of_the_lane_strided_chunk_loop():
    """16,641 atoms are 65 chunks + 1 atom: lanes 0 and 1 of the structure's wave read a second chunk partial each."""
    sizes, iters = [3, 16641], 10
    st = _state("full", True, sizes)
    obs, _ = _run(st, sizes, iters)
    refs, ref_obs = _references("full", True, sizes, iters)
    worst = _compare(st, obs, refs, ref_obs, sizes)
    print(f"16,641 atoms: largest relative difference from the restatement {worst:.1e} (gate 1e-12)")
    assert all(ref.n_steps == iters - 1 for ref in refs)


@pytest.mark.parametrize("mask", MASKS)
def test_mtk_kernel_bitwise_reproducible_and_independent_of_the_batch(mask):
    runs = []
    for _ in range(2):
        st = _state(mask, True, SIZES)
        runs.append((st, _run(st, SIZES, 25)[0]))
    (s0, o0), (s1, o1) = runs
    assert np.array_equal(o0, o1) and torch.equal(s0.pos, s1.pos) and torch.equal(s0.lattice, s1.lattice)
    assert torch.equal(s0.lattice32, s1.lattice32)
    r0, r1 = s0.read(), s1.read()
    assert np.array_equal(r0["v"], r1["v"]) and np.array_equal(r0["chain"], r1["chain"])
    offs = np.concatenate([[0], np.cumsum(SIZES)])
    for i in (0, 3, 4):
        a, b = offs[i], offs[i + 1]
        alone = _state(mask, True, SIZES, only=i)
        obs, _ = _run(alone, SIZES, 25, rows=((a, b), i))
        r = alone.read()
        assert torch.equal(alone.pos, s0.pos[a:b]) and torch.equal(alone.lattice[0], s0.lattice[i])
        assert np.array_equal(r["v"], r0["v"][a:b]) and np.array_equal(obs[:, 0], o0[:, i]) and np.array_equal(r["chain"][0], r0["chain"][i])
        assert r["flags"][0] == r0["flags"][i] and r["n_steps"][0] == r0["n_steps"][i]


def test_bad_force_and_over_rate_stress_freeze_those_structures_only():
    from torch_m3gnet import _lib

    iters = 20
    bad = dict(nan_at=(6, 2 + 3 + 20), stress_at=(9, 3))   # call 6: an atom of structure 2; call 9: structure 3's stress
    offs = np.concatenate([[0], np.cumsum(SIZES)])
    st = _state("full", True, SIZES)
    obs, snap = _run(st, SIZES, iters, snapshot_after=5, **bad)
    refs, ref_obs = _references("full", True, SIZES, iters, **bad)
    _compare(st, obs, refs, ref_obs, SIZES)
    r = st.read()
    assert [bool(x & _lib.DYN_ERROR) for x in r["flags"]] == [False, False, True, True, False]
    assert list(r["n_steps"]) == [iters - 1] * 2 + [6, 9, iters - 1]
    assert np.array_equal(obs[6:, 2], np.repeat(obs[5:6, 2], iters - 6, axis=0))   # their observables stay those of the call before
    assert np.array_equal(obs[9:, 3], np.repeat(obs[8:9, 3], iters - 9, axis=0))
    # structure 2 bitwise where it stood after call 5: positions, cell, velocities and chain
    pos5, lat5, state5 = snap
    frozen = _state("full", True, SIZES)
    frozen.state.copy_(state5)
    r5 = frozen.read()
    a, b = offs[2], offs[3]
    assert torch.equal(st.pos[a:b], pos5[a:b]) and torch.equal(st.lattice[2], lat5[2])
    assert np.array_equal(r["v"][a:b], r5["v"][a:b]) and np.array_equal(r["chain"][2], r5["chain"][2])
    assert torch.isfinite(st.pos).all() and np.isfinite(r["v"]).all() and np.isfinite(r["chain"]).all()
    # the others: bitwise those of an undisturbed run; structure 3 up to the call before its verdict
    clean = _state("full", True, SIZES)
    clean_obs, _ = _run(clean, SIZES, iters)
    rc = clean.read()
    for i in (0, 1, 4):
        a, b = offs[i], offs[i + 1]
        assert torch.equal(st.pos[a:b], clean.pos[a:b]) and torch.equal(st.lattice[i], clean.lattice[i])
        assert np.array_equal(r["v"][a:b], rc["v"][a:b]) and np.array_equal(r["chain"][i], rc["chain"][i])
        assert np.array_equal(obs[:, i], clean_obs[:, i])
    assert np.array_equal(obs[:9, 3], clean_obs[:9, 3]) and not np.array_equal(obs[9:, 3], clean_obs[9:, 3])


def test_mtk_step_capture_replays_bitwise():
    from torch_m3gnet.dynamics import mtk_cell_step

    sizes = [3, 32, 1000]
    f, s = _forces(sizes, 0, 3)
    forces, stresses = torch.tensor(f, device=DEV), torch.tensor(s, device=DEV)
    for mask in MASKS:
        eager, graphed = _state(mask, True, sizes), _state(mask, True, sizes)
        for _ in range(10):
            mtk_cell_step(eager, forces, stresses)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            mtk_cell_step(graphed, forces, stresses)
        for _ in range(10):
            g.replay()
        torch.cuda.synchronize()
        assert torch.equal(eager.pos, graphed.pos) and torch.equal(eager.lattice, graphed.lattice) and torch.equal(eager.obs, graphed.obs)
        assert torch.equal(eager.lattice32, graphed.lattice32)
        re, rg = eager.read(), graphed.read()
        assert np.array_equal(re["v"], rg["v"]) and np.array_equal(re["chain"], rg["chain"]) and np.array_equal(re["n_steps"], rg["n_steps"])
        assert re["n_steps"][0] == 10 and not (re["flags"] & 2).any()


@pytest.mark.parametrize("mask", MASKS)
def test_mtk_state_on_exact_size_buffer(mask, monkeypatch):
    from test_gpu_guard_bands import _driver_on_guarded_states
    from torch_m3gnet import dynamics

    sizes = [2, 40, 257]

    def run():
        st = _state(mask, True, sizes)
        obs, _ = _run(st, sizes, 10)
        return dict(st.read(), obs=obs, pos=st.pos, lattice=st.lattice, lattice32=st.lattice32)

    _driver_on_guarded_states(monkeypatch, f"mtk cell {mask}", {"dynamics": dynamics}, run)


# ---- physics under the LJ-fitted model ---------------------------------------------------------------------------------------------
STEPS, SHEAR = 800, 0.002
Z32 = np.full(32, 29)


def _drift(log):
    return float(np.abs(log["conserved"] - log["conserved"][0]).max())


@functools.lru_cache(maxsize=None)
def _a0():
    """The model's lattice constant: the parabola fit of tests/test_gpu_nhc.py's test_npt_mtk_oscillates_about_the_models_lattice_constant."""
    from torch_m3gnet.data import MaterialGraphKey as K
    from torch_m3gnet.data.md import VerletGraph
    from torch_m3gnet.nn import Gradient

    pv = Gradient(_fitted_model().model, pair_virial=True)
    grid_a = np.linspace(3.48, 3.53, 11)
    e = []
    for a in grid_a:
        p, L = _fcc(a, 2)
        vg = VerletGraph([L], [Z32], 5.0, 4.0, skin=0.5, device=DEV)
        e.append(float(vg.step(pv, torch.tensor(p, device=DEV))[K.TOTAL_ENERGY][0]) / 32)
    c2, c1, _ = np.polyfit(grid_a, e, 2)
    a0 = -c1 / (2 * c2)
    assert 3.48 < a0 < 3.53 and c2 > 0
    return a0


def _md(ensemble, **kw):
    """10 K, taut 1000, taup 3000, 0 GPa, 1 fs: the settings of the isotropic family's test, for the reasons its docstring gives."""
    from torch_m3gnet.dynamics import MolecularDynamics

    return MolecularDynamics(_fitted_model(), ensemble=ensemble, timestep=1.0, temperature=10.0, taut=1000.0, pressure=0.0, taup=3000.0, **kw)


@functools.lru_cache(maxsize=None)
def _isotropic_yardstick():
    """The isotropic family's run from a0 + 0.01 A: conserved per atom-step."""
    pos, lat = _fcc(_a0() + 0.01, 2)
    (res,) = _md("npt_mtk").run([lat], [pos], [Z32], STEPS, loginterval=1)
    assert not res["error"] and res["n_steps"] == STEPS
    return _drift(res["log"]) / (32 * STEPS)


@functools.lru_cache(maxsize=None)
def _sheared_run():
    """(a): the cubic cell at a0 times I + eps, eps_xy = eps_yx = 0.002, which moves the fourth shell 0.010 A, inside its 0.047 A
    distance to the cutoff."""
    pos, lat = _fcc(_a0(), 2)
    strain = np.eye(3)
    strain[0, 1] = strain[1, 0] = SHEAR
    (res,) = _md("npt_mtk_cell", cell_mask="full").run([lat @ strain], [pos @ strain], [Z32], STEPS, loginterval=1)
    return res


def test_sheared_cell_swings_back_through_cubic_and_conserves():
    """Gates: at least 4 sign changes of the symmetric shear strain (about 13 expected: C44 = 163 and B = 304 GPa from
    profiles/elastic.txt and the 71 fs isotropic period give a shear period of about 119 fs), its mean over the last 300 steps below
    0.3 of the starting strain, <a> of the last fifth within 3e-3 A of a0, `conserved` per atom-step at most 3 times that of the
    isotropic family's run from a0 + 0.01 A (the project's drift margin).  Measured on the MI355X (profiles/mtk_cell.txt): 16 sign
    changes, period 98.7 fs, mean of the last 300 steps 1.53e-5, <a> 2.0e-4 A from a0, 9.85e-10 eV per atom-step against 1.63e-9
    (0.61 x)."""
    a0, res = _a0(), _sheared_run()
    assert not res["error"] and res["n_steps"] == STEPS
    log = res["log"]
    assert log["lattice"].shape == (STEPS + 1, 3, 3) and log["pressure_tensor"].shape == (STEPS + 1, 6)
    assert np.allclose(log["p"], log["pressure_tensor"][:, :3].mean(1), rtol=1e-12, atol=1e-14)
    assert np.allclose(np.abs(np.linalg.det(log["lattice"])), log["v"], rtol=1e-12)
    assert np.array_equal(log["lattice"][-1], res["lattice"])
    f = log["lattice"] / (2.0 * a0)   # the deformation gradient against the cubic cell
    shear = 0.5 * (f[:, 0, 1] + f[:, 1, 0])
    assert shear[0] == pytest.approx(SHEAR, rel=1e-9)
    crossings = np.nonzero(np.diff(np.sign(shear)) != 0)[0]
    period = 2.0 * np.diff(crossings).mean() if len(crossings) > 1 else float("nan")
    a = log["v"] ** (1 / 3) / 2
    a_mean = a[-STEPS // 5:].mean()
    d_cell, d_iso = _drift(log) / (32 * STEPS), _isotropic_yardstick()
    print(f"a0 = {a0:.5f} A; shear strain from {SHEAR} in [{shear.min():.5f}, {shear.max():.5f}], {len(crossings)} sign changes, period "
          f"{period:.1f} fs, mean of the last 300 steps {shear[-300:].mean():.2e}; <a> of the last fifth {a_mean:.5f} A; conserved within "
          f"{d_cell:.2e} eV per atom-step against {d_iso:.2e} of npt_mtk ({d_cell / d_iso:.2f} x)")
    assert len(crossings) >= 4
    assert abs(shear[-300:].mean()) < 0.3 * SHEAR
    assert abs(a_mean - a0) < 3e-3, (a_mean, a0)
    assert d_cell <= 3.0 * d_iso, (d_cell, d_iso)


def test_orthorhombic_cell_keeps_its_axes_and_conserves():
    """(b): from diag(a0 + 0.01, a0, a0) * 2.  Measured on the MI355X: lengths / 2 of 3.50728, 3.49917, 3.49926 A at the end,
    9.06e-10 eV per atom-step against 1.63e-9 (0.56 x)."""
    a0 = _a0()
    pos, lat = _fcc(a0, 2)
    stretch = np.diag([(a0 + 0.01) / a0, 1.0, 1.0])
    (res,) = _md("npt_mtk_cell", cell_mask="orthorhombic").run([lat @ stretch], [pos @ stretch], [Z32], STEPS, loginterval=1)
    assert not res["error"] and res["n_steps"] == STEPS
    lats = res["log"]["lattice"]
    assert (lats - lats * np.eye(3) == 0.0).all()   # off-diagonals exactly 0 throughout
    lengths = np.diag(res["lattice"])
    d_cell, d_iso = _drift(res["log"]) / (32 * STEPS), _isotropic_yardstick()
    print(f"orthorhombic: lengths / 2 = {lengths / 2} A against a0 = {a0:.5f}; conserved within {d_cell:.2e} eV per atom-step against "
          f"{d_iso:.2e} of npt_mtk ({d_cell / d_iso:.2f} x)")
    assert min(abs(lengths[0] - lengths[1]), abs(lengths[1] - lengths[2]), abs(lengths[0] - lengths[2])) > 1e-7
    assert np.ptp(np.diagonal(lats, axis1=1, axis2=2)[:, 0]) > 1e-3   # and they moved
    assert d_cell <= 3.0 * d_iso, (d_cell, d_iso)


def test_final_energy_and_forces_match_a_fresh_evaluation_in_the_final_cell():
    """No stale neighbour list was carried over the change of shape: a fresh graph at the final positions and cell agrees (energy
    to 1e-5 relative, forces to 1e-4 of max |F|; measured on the MI355X: both equal bit for bit)."""
    from types import SimpleNamespace

    from torch_m3gnet.data import MaterialGraphKey as K
    from torch_m3gnet.data.graph_gpu import batch_from_structures

    res = _sheared_run()
    s = SimpleNamespace(lattice=SimpleNamespace(matrix=res["lattice"]), cart_coords=res["positions"], atomic_numbers=Z32)
    g = _fitted_model()(batch_from_structures([s], 5.0, 4.0))
    e, f = float(g[K.TOTAL_ENERGY][0]), g[K.FORCES].double().cpu().numpy()
    e_err, f_err = abs(e - res["total_energy"]) / abs(e), np.abs(f - res["forces"]).max() / np.abs(f).max()
    print(f"fresh evaluation in the final cell: E rel err {e_err:.2e}, F err {f_err:.2e} of max |F|")
    assert np.abs(res["lattice"] - np.diag(np.diag(res["lattice"]))).max() > 1e-6
    assert e_err < 1e-5 and f_err < 1e-4
