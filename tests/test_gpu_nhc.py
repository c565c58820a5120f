"""Nose-Hoover chain NVT and MTK NPT on the MI355X (torch_m3gnet.dynamics NhcState / nhc_step, C ABI m3g_nhc_*): the kernels against
the numpy restatement (tests/nhc_reference.py), bitwise reproducibility and independence of the batch, non-finite forces, graph
capture, and runs under the LJ-fitted model: the conserved quantity, the approach to the target temperature and the lattice constant
at zero pressure."""
import functools

import numpy as np
import pytest
import torch

import nhc_reference as nr
from helpers import CASE_MODEL, GOLDEN
from test_gpu_dynamics import _batch, _fcc, _fitted_model, _forces, _rel

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = [2, 3, 32, 257, 10000]   # one chunk, a chunk boundary (256 rows + 1), many chunks
TEMPS = [50.0, 900.0, 300.0, 20.0, 600.0]
PARAMS = dict(dt=1.0, taut=20.0, pressure=1e-3, taup=100.0)
CASES = [(e, fc, m, nc) for e in ("nvt_nose_hoover", "npt_mtk") for fc in (False, True) for m in (1, 3) for nc in (1, 2)]


def _state(ensemble, fix_com, sizes, chain=(3, 1), temps=None, only=None):
    """The batch's state, or with `only` = i that of its structure i alone."""
    from torch_m3gnet.dynamics import NhcState

    lats, poss, ms, vs = _batch(sizes, 0)
    temps = TEMPS[:len(sizes)] if temps is None else temps
    if only is not None:
        lats, poss, ms, vs, temps, sizes = [lats[only]], [poss[only]], [ms[only]], [vs[only]], [temps[only]], [sizes[only]]
    pos = torch.tensor(np.concatenate(poss), dtype=torch.float64, device=DEV)
    lat = torch.tensor(np.stack(lats), dtype=torch.float64, device=DEV)
    vel = torch.tensor(np.concatenate(vs), dtype=torch.float64, device=DEV)
    return NhcState(pos, lat, np.concatenate([[0], np.cumsum(sizes)]), np.concatenate(ms), vel, temps, ensemble=ensemble, fix_com=fix_com,
                    chain_length=chain[0], chain_substeps=chain[1], **PARAMS)


def _run(st, sizes, iters, nan_at=None, rows=None, snapshot_after=None):
    from torch_m3gnet.dynamics import nhc_step

    obs, snap = [], None
    for k in range(iters):
        f, s = _forces(sizes, k, 0, nan_at)
        if rows is not None:   # one structure's rows of the batch's inputs
            (a, b), i = rows
            f, s = np.ascontiguousarray(f[a:b]), np.ascontiguousarray(s[i:i + 1])
        nhc_step(st, torch.tensor(f, device=DEV), torch.tensor(s, device=DEV), finish_only=(k == iters - 1))
        obs.append(st.obs.clone())
        if k == snapshot_after:
            snap = (st.pos.clone(), st.lattice.clone(), st.state.clone())
    torch.cuda.synchronize()
    return torch.stack(obs).cpu().numpy(), snap


def _references(ensemble, fix_com, sizes, iters, chain=(3, 1), nan_at=None):
    lats, poss, ms, vs = _batch(sizes, 0)
    refs = [nr.NhcReference(p, L, m, v, ensemble, temperature=t, fix_com=fix_com, chain_length=chain[0], chain_substeps=chain[1], **PARAMS)
            for p, L, m, v, t in zip(poss, lats, ms, vs, TEMPS)]
    offs = np.concatenate([[0], np.cumsum(sizes)])
    obs, lam_off_one = [], False
    for k in range(iters):
        f, s = _forces(sizes, k, 0, nan_at)
        row = []
        for i, ref in enumerate(refs):
            ref.step(f[offs[i]:offs[i + 1]].astype(np.float64), s[i].astype(np.float64), finish_only=(k == iters - 1))
            row.append(ref.obs)
            lam_off_one = lam_off_one or abs(ref.lam - 1.0) > 1e-6
        obs.append(row)
    return refs, np.array(obs), lam_off_one


def _compare(st, obs, refs, ref_obs, sizes):
    out = st.read()
    offs = np.concatenate([[0], np.cumsum(sizes)])
    pos, lat = st.pos.cpu().numpy(), st.lattice.cpu().numpy()
    M = st.chain_length
    for i, ref in enumerate(refs):
        a, b = offs[i], offs[i + 1]
        assert out["flags"][i] == ref.flags and out["n_steps"][i] == ref.n_steps, (i, out["flags"][i], ref.flags, out["n_steps"][i], ref.n_steps)
        assert _rel(pos[a:b], ref.pos) < 1e-12, (i, _rel(pos[a:b], ref.pos))
        assert _rel(out["v"][a:b], ref.v, 1e-4) < 1e-12, (i, _rel(out["v"][a:b], ref.v, 1e-4))
        assert _rel(lat[i], ref.lattice) < 1e-12, i
        chain = np.concatenate([ref.xi, ref.vxi, ref.xib, ref.vxib, [ref.veps]])
        assert out["chain"][i].shape == (4 * M + 1,) and _rel(out["chain"][i], chain) < 1e-12, (i, out["chain"][i], chain)
        if not ref.flags & nr.ERROR:
            for j in range(5):
                assert _rel(obs[:, i, j], ref_obs[:, i, j]) < 1e-12, (i, j, _rel(obs[:, i, j], ref_obs[:, i, j]))
            assert not obs[:, i, 5].any()


@pytest.mark.parametrize("ensemble,fix_com,chain_length,chain_substeps", CASES)
def test_nhc_kernel_matches_restatement(ensemble, fix_com, chain_length, chain_substeps):
    iters, chain = 40, (chain_length, chain_substeps)
    st = _state(ensemble, fix_com, SIZES, chain)
    obs, _ = _run(st, SIZES, iters)
    refs, ref_obs, lam_off_one = _references(ensemble, fix_com, SIZES, iters, chain)
    _compare(st, obs, refs, ref_obs, SIZES)
    assert all(ref.n_steps == iters - 1 for ref in refs) and lam_off_one
    moved = np.abs(st.lattice.cpu().numpy() - np.stack(_batch(SIZES)[0])).max()
    if ensemble == "npt_mtk":
        assert moved > 1e-6
        assert torch.equal(st.lattice32, st.lattice.to(torch.float32))
    else:
        assert moved == 0.0


@pytest.mark.parametrize("ensemble", ["nvt_nose_hoover", "npt_mtk"])
def test_nhc_kernel_bitwise_reproducible_and_independent_of_the_batch(ensemble):
    runs = []
    for _ in range(2):
        st = _state(ensemble, True, SIZES)
        runs.append((st, _run(st, SIZES, 25)[0]))
    (s0, o0), (s1, o1) = runs
    assert np.array_equal(o0, o1) and torch.equal(s0.pos, s1.pos) and torch.equal(s0.lattice, s1.lattice)
    r0, r1 = s0.read(), s1.read()
    assert np.array_equal(r0["v"], r1["v"]) and np.array_equal(r0["chain"], r1["chain"])
    offs = np.concatenate([[0], np.cumsum(SIZES)])
    for i in (0, 3, 4):
        a, b = offs[i], offs[i + 1]
        alone = _state(ensemble, True, SIZES, only=i)
        obs, _ = _run(alone, SIZES, 25, rows=((a, b), i))
        r = alone.read()
        assert torch.equal(alone.pos, s0.pos[a:b]) and torch.equal(alone.lattice[0], s0.lattice[i])
        assert np.array_equal(r["v"], r0["v"][a:b]) and np.array_equal(obs[:, 0], o0[:, i]) and np.array_equal(r["chain"][0], r0["chain"][i])
        assert r["flags"][0] == r0["flags"][i] and r["n_steps"][0] == r0["n_steps"][i]


@pytest.mark.parametrize("ensemble", ["nvt_nose_hoover", "npt_mtk"])
def test_non_finite_force_freezes_that_structure_only(ensemble):
    from torch_m3gnet import _lib

    iters, nan_at = 20, (6, 2 + 3 + 20)   # call 6: an atom of structure 2
    st = _state(ensemble, True, SIZES)
    obs, snap = _run(st, SIZES, iters, nan_at=nan_at, snapshot_after=5)
    refs, ref_obs, _ = _references(ensemble, True, SIZES, iters, nan_at=nan_at)
    _compare(st, obs, refs, ref_obs, SIZES)
    r = st.read()
    assert [bool(x & _lib.DYN_ERROR) for x in r["flags"]] == [False, False, True, False, False]
    assert list(r["n_steps"]) == [iters - 1] * 2 + [6] + [iters - 1] * 2
    assert np.array_equal(obs[6:, 2], np.repeat(obs[5:6, 2], iters - 6, axis=0))   # its observables stay those of call 5
    # bitwise where it stood after call 5: positions, cell, velocities and chain
    pos5, lat5, state5 = snap
    frozen = _state(ensemble, True, SIZES)
    frozen.state.copy_(state5)
    r5 = frozen.read()
    assert torch.equal(st.pos[5:37], pos5[5:37]) and torch.equal(st.lattice[2], lat5[2])
    assert np.array_equal(r["v"][5:37], r5["v"][5:37]) and np.array_equal(r["chain"][2], r5["chain"][2])
    assert not torch.equal(st.pos[37:], pos5[37:])
    assert torch.isfinite(st.pos).all() and np.isfinite(r["v"]).all()


def test_nhc_step_capture_replays_bitwise():
    from torch_m3gnet.dynamics import nhc_step

    sizes = [3, 32, 1000]
    f, s = _forces(sizes, 0, 3)
    forces, stresses = torch.tensor(f, device=DEV), torch.tensor(s, device=DEV)
    for ensemble in ("nvt_nose_hoover", "npt_mtk"):
        eager, graphed = _state(ensemble, True, sizes), _state(ensemble, True, sizes)
        for _ in range(10):
            nhc_step(eager, forces, stresses)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            nhc_step(graphed, forces, stresses)
        for _ in range(10):
            g.replay()
        torch.cuda.synchronize()
        assert torch.equal(eager.pos, graphed.pos) and torch.equal(eager.lattice, graphed.lattice) and torch.equal(eager.obs, graphed.obs)
        re, rg = eager.read(), graphed.read()
        assert np.array_equal(re["v"], rg["v"]) and np.array_equal(re["chain"], rg["chain"]) and np.array_equal(re["n_steps"], rg["n_steps"])
        assert re["n_steps"][0] == 10


# ---- physics under the LJ-fitted model ---------------------------------------------------------------------------------------------
def _drift(log):
    h = log["conserved"] if "conserved" in log else log["e_pot"] + log["ke"]
    return float(np.abs(h - h[0]).max())


@functools.lru_cache(maxsize=None)
def _nve_setup_runs():
    """The 108-atom setup of tests/test_gpu_dynamics.py's NVE test (cutoffs 4.76 / 4.38 in gaps of the fcc shells, 50 K start) for
    300 fs: NVE at dt = 1, nvt_nose_hoover (taut = 50 fs) at dt = 1 and 2.  Run once, shared by the tests below.  The thermostat's
    target is the 50 K of the start: the kinetic share settles near 31 K in NVE, so the thermostat has work to do, and the amplitudes
    stay those of the NVE test.  They have to: the reference model's energy jumps where a pair crosses a cutoff, and from a start
    of twice the velocities NVE itself loses 0.64 eV in these 300 fs, at 1 fs and at 2 fs alike; a 100 K target with taut = 50 fs
    heats the cell to 118 K and the conserved quantity then moves by 1.1e-2 eV whatever the timestep (0.5, 1 and 2 fs)."""
    from oracle import m3gnet_oracle as orc
    from torch_m3gnet.dynamics import MolecularDynamics
    from torch_m3gnet.model.build import build_model

    rc, r3 = 4.76, 4.38
    params, cfg, elemental = orc.load_model_npz(GOLDEN / f"{CASE_MODEL['cu32fit']}.npz")
    model = build_model(rc, r3, cfg.l_max, cfg.n_max, cfg.num_types, cfg.embedding_dim, cfg.num_blocks, elemental_energies=elemental,
                        energy_scale=cfg.energy_scale, length_scale=cfg.length_scale)
    model.load_state_dict({k: v for k, v in params.items()})
    model = model.to(DEV)
    pos0, lat = _fcc(3.61, 3)
    mass = 63.546
    rng = np.random.default_rng(9)
    pos = pos0 + rng.normal(0, 0.01, pos0.shape)
    vel = rng.normal(0, np.sqrt(nr.KB * 50.0 / mass * nr.KAPPA), pos0.shape)
    vel -= vel.mean(0)

    def run(ensemble, dt, steps, **kw):
        md = MolecularDynamics(model, ensemble=ensemble, timestep=dt, skin=0.3, **kw)
        (res,) = md.run([lat], [pos], [np.full(108, 29)], steps, velocities=[vel], loginterval=1)
        assert not res["error"] and res["n_steps"] == steps
        return res["log"]

    nhc = dict(temperature=50.0, taut=50.0)
    return run("nve", 1.0, 300), run("nvt_nose_hoover", 1.0, 300, **nhc), run("nvt_nose_hoover", 2.0, 150, **nhc)


def test_nose_hoover_under_the_fitted_model_conserves_and_heats_towards_the_target():
    """Measured on the MI355X (profiles/nose_hoover.txt): NVE within 6.4e-5 eV; Nose-Hoover within 9.3e-5 eV at 1 fs (1.45 x NVE) and
    3.5e-4 eV at 2 fs (ratio 3.75; 2.9e-5 eV at 0.5 fs); T over the last 100 fs 53.4 K against 31.2 K in NVE."""
    nve, nh1, nh2 = _nve_setup_runs()
    assert set(nh1) == set(nve) | {"conserved"}   # the log keys of the other ensembles are unchanged
    d_nve, d1, d2 = _drift(nve), _drift(nh1), _drift(nh2)
    t_nve, t_nh = nve["t"][-100:].mean(), nh1["t"][-100:].mean()
    print(f"300 fs from 50 K: NVE drift {d_nve:.2e} eV; Nose-Hoover (50 K) conserved within {d1:.2e} eV at dt = 1 fs ({d1 / d_nve:.2f} x NVE), "
          f"{d2:.2e} eV at 2 fs (ratio {d2 / d1:.2f}); T over the last 100 fs {t_nh:.1f} K against {t_nve:.1f} K in NVE")
    assert 2.0 < d2 / d1 < 8.0, (d1, d2)
    assert d1 <= 3.0 * d_nve, (d1, d_nve)
    target = 50.0 * (3 * 108 - 3) / (3 * 108)
    assert nh1["t"][0] == pytest.approx(nve["t"][0], rel=1e-12)
    assert t_nve < target and abs(t_nh - target) < 0.5 * abs(t_nve - target), (t_nh, t_nve)


def test_nose_hoover_replica_batch_holds_each_target():
    """2,000 steps of 2 fs; taut = 50 fs, at which the restatement on the LJ cell of tests/test_nhc_cpu.py meets the same gate on the
    CPU (test_restatement_nvt_mean_temperature).  T is 2 KE / (3 n kB): its canonical mean is t0 g / (3 n)."""
    from torch_m3gnet.dynamics import MolecularDynamics

    pos, lat = _fcc(3.61, 3)
    temps = [300.0, 200.0]
    md = MolecularDynamics(_fitted_model(), ensemble="nvt_nose_hoover", timestep=2.0, temperature=temps, taut=50.0, seed=5)
    res = md.run([lat] * 2, [pos] * 2, [np.full(108, 29)] * 2, 2000, loginterval=1)
    for r, t0 in zip(res, temps):
        assert not r["error"] and r["n_steps"] == 2000
        t_mean, want = r["log"]["t"][-1500:].mean(), t0 * (3 * 108 - 3) / (3 * 108)
        print(f"target {t0} K: mean T of the last 1,500 steps {t_mean:.2f} K against {want:.2f} K")
        assert abs(t_mean / want - 1.0) < 0.05, (t0, t_mean)
    assert not np.array_equal(res[0]["positions"], res[1]["positions"])


def test_nose_hoover_accepts_trajectory_observables():
    from torch_m3gnet.dynamics import MolecularDynamics
    from torch_m3gnet.trajectory import TrajectoryObservables

    pos, lat = _fcc(3.61, 2)
    md = MolecularDynamics(_fitted_model(), ensemble="nvt_nose_hoover", timestep=2.0, temperature=100.0, taut=50.0)
    (res,) = md.run([lat], [pos], [np.full(32, 29)], 20, observables=TrajectoryObservables(rdf_bins=50, n_lags=8))
    assert not res["error"] and "observables" in res and "conserved" in res["log"]


def test_npt_mtk_oscillates_about_the_models_lattice_constant():
    """The 32-atom cell from a0 + 0.01 A at 10 K and zero pressure.  The amplitudes have to stay small enough that no pair crosses a
    cutoff, because the reference model's energy jumps there: the fourth fcc shell lies 0.047 A inside the 5 A two-body cutoff at a0
    and 0.033 A inside at a0 + 0.01 A, where the cell starts and to where it swings back every period.  The kinetic share of the 10 K
    start settles near 5 K.  With taut = 100 fs the thermostat rings (T between 6 and 11 K) and one pair crossed the cutoff and back
    at steps 564 and 570, two jumps of 4.3e-3 eV in a quantity otherwise constant to 1.8e-5 eV, at 1 fs and at 0.5 fs alike; so
    taut = 1000 fs here, longer than the run, under which the lattice keeps the amplitudes of 5 - 6 K.  The barostat mass is
    proportional to kT, so at 10 K taup = 3000 fs gives a cell period of 71 fs.  800 steps of 1 fs; the last fifth spans two periods.
    The drift gate is per atom-step against the Nose-Hoover run at 1 fs of the test above."""
    from torch_m3gnet.data import MaterialGraphKey as K
    from torch_m3gnet.data.md import VerletGraph
    from torch_m3gnet.dynamics import MolecularDynamics
    from torch_m3gnet.nn import Gradient

    model = _fitted_model()
    pv = Gradient(model.model, pair_virial=True)
    z = np.full(32, 29)
    grid_a = np.linspace(3.48, 3.53, 11)   # the parabola fit of test_npt_berendsen_reaches_the_models_lattice_constant
    e = []
    for a in grid_a:
        p, L = _fcc(a, 2)
        vg = VerletGraph([L], [z], 5.0, 4.0, skin=0.5, device=DEV)
        e.append(float(vg.step(pv, torch.tensor(p, device=DEV))[K.TOTAL_ENERGY][0]) / 32)
    c2, c1, _ = np.polyfit(grid_a, e, 2)
    a0 = -c1 / (2 * c2)
    assert 3.48 < a0 < 3.53 and c2 > 0
    pos, lat = _fcc(a0 + 0.01, 2)
    steps = 800
    md = MolecularDynamics(model, ensemble="npt_mtk", timestep=1.0, temperature=10.0, taut=1000.0, pressure=0.0, taup=3000.0)
    (res,) = md.run([lat], [pos], [z], steps, loginterval=1)
    assert not res["error"] and res["n_steps"] == steps
    L = res["lattice"]
    assert np.abs(L - np.diag(np.diag(L))).max() < 1e-9 * np.abs(L).max()   # stays cubic
    assert np.ptp(np.diag(L)) < 1e-9 * L[0, 0]
    a = res["log"]["v"] ** (1 / 3) / 2
    a_mean = a[-steps // 5:].mean()
    d_npt, d_nvt = _drift(res["log"]) / (32 * steps), _drift(_nve_setup_runs()[1]) / (108 * 300)
    print(f"a0 = {a0:.5f} A; a in [{a.min():.5f}, {a.max():.5f}], mean of the last fifth {a_mean:.5f} A; conserved within {d_npt:.2e} eV "
          f"per atom-step against {d_nvt:.2e} of the Nose-Hoover run ({d_npt / d_nvt:.2f} x)")
    assert a.min() < a0 < a.max()
    assert abs(a_mean - a0) < 3e-3, (a_mean, a0)
    assert d_npt <= 3.0 * d_nvt, (d_npt, d_nvt)
