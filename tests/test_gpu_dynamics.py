"""Batched molecular dynamics on the MI355X (torch_m3gnet.dynamics, C ABI m3g_dyn_*): the kernel against the numpy restatement
(tests/md_reference.py) in all four ensembles, bitwise reproducibility and independence of the batch, non-finite forces, graph
capture, and NVE / Langevin / Berendsen NVT / NPT runs under the LJ-fitted model."""
import numpy as np
import pytest
import torch

import md_reference as mr
from helpers import CASE_MODEL, GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = [1, 3, 32, 1000, 10000]
TEMPS = [50.0, 900.0, 300.0, 20.0, 600.0]
SEEDS = [11, 2 ** 63 + 5, 77, 12345, 2 ** 64 - 1]
FCC_BASE = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])
PARAMS = dict(dt=1.0, taut=20.0, friction=0.02, pressure=1e-3, taup=100.0, compressibility=1.0)
CASES = [("nve", False), ("nve", True), ("nvt_berendsen", False), ("nvt_berendsen", True), ("nvt_langevin", False),
         ("npt_berendsen", False), ("npt_berendsen", True)]


def _batch(sizes, seed=0):
    """Lattices, positions, masses and starting velocities (Maxwell-Boltzmann at a temperature far from the targets: a lambda clamp)."""
    from torch_m3gnet.dynamics import maxwell_boltzmann

    rng = np.random.default_rng(seed)
    lats, poss, ms, vs = [], [], [], []
    for j, n in enumerate(sizes):
        L = np.eye(3) * (12.0 * n) ** (1 / 3) + rng.normal(0, 0.05, (3, 3))
        lats.append(L)
        poss.append(rng.uniform(0, 1, (n, 3)) @ L)
        ms.append(rng.uniform(1.0, 200.0, n))
        vs.append(maxwell_boltzmann(ms[-1], 100.0 + 50 * j, seed + j) if n > 1 else rng.normal(0, 1e-3, (1, 3)))
    return lats, poss, ms, vs


def _forces(sizes, k, seed, nan_at=None):
    rng = np.random.default_rng([seed, k])
    n = sum(sizes)
    f = rng.normal(0, 0.5, (n, 3)).astype(np.float32)
    st = rng.normal(0, 1e-3, (len(sizes), 6)).astype(np.float32)
    if nan_at is not None and k == nan_at[0]:
        f[nan_at[1], 1] = np.nan
    return f, st


def _state(ensemble, fix_com, sizes, seed=0, temps=None, seeds=None):
    from torch_m3gnet.dynamics import DynState

    lats, poss, ms, vs = _batch(sizes, seed)
    pos = torch.tensor(np.concatenate(poss), dtype=torch.float64, device=DEV)
    lat = torch.tensor(np.stack(lats), dtype=torch.float64, device=DEV)
    vel = torch.tensor(np.concatenate(vs), dtype=torch.float64, device=DEV)
    return DynState(pos, lat, np.concatenate([[0], np.cumsum(sizes)]), np.concatenate(ms), vel, TEMPS if temps is None else temps,
                    SEEDS if seeds is None else seeds, ensemble=ensemble, fix_com=fix_com, **PARAMS)


def _run(st, sizes, iters, seed=0, nan_at=None, rows=None):
    from torch_m3gnet.dynamics import dyn_step

    obs = []
    for k in range(iters):
        f, s = _forces(sizes, k, seed, nan_at)
        if rows is not None:   # one structure's rows of the batch's inputs
            (a, b), i = rows
            f, s = np.ascontiguousarray(f[a:b]), np.ascontiguousarray(s[i:i + 1])
        dyn_step(st, torch.tensor(f, device=DEV), torch.tensor(s, device=DEV), finish_only=(k == iters - 1))
        obs.append(st.obs.clone())
    torch.cuda.synchronize()
    return torch.stack(obs).cpu().numpy()


def _rel(a, b, floor=1e-300):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), floor))


def _references(ensemble, fix_com, sizes, iters, seed=0, nan_at=None):
    lats, poss, ms, vs = _batch(sizes, seed)
    refs = [mr.DynReference(p, L, m, v, ensemble, temperature=t, seed=sd, fix_com=fix_com, **PARAMS)
            for p, L, m, v, t, sd in zip(poss, lats, ms, vs, TEMPS, SEEDS)]
    offs = np.concatenate([[0], np.cumsum(sizes)])
    obs, clamped = [], False
    for k in range(iters):
        f, s = _forces(sizes, k, seed, nan_at)
        row = []
        for i, ref in enumerate(refs):
            ref.step(f[offs[i]:offs[i + 1]].astype(np.float64), s[i].astype(np.float64), finish_only=(k == iters - 1))
            row.append(ref.obs)
            clamped = clamped or (ref.lam in (0.9, 1.1) and k < iters - 1)
        obs.append(row)
    return refs, np.array(obs), clamped


def _compare(st, obs, refs, ref_obs, sizes):
    out = st.read()
    offs = np.concatenate([[0], np.cumsum(sizes)])
    pos, lat = st.pos.cpu().numpy(), st.lattice.cpu().numpy()
    for i, ref in enumerate(refs):
        a, b = offs[i], offs[i + 1]
        assert out["flags"][i] == ref.flags and out["n_steps"][i] == ref.n_steps, (i, out["flags"][i], ref.flags, out["n_steps"][i], ref.n_steps)
        assert _rel(pos[a:b], ref.pos) < 1e-12, (i, _rel(pos[a:b], ref.pos))
        assert _rel(out["v"][a:b], ref.v, 1e-4) < 1e-12, (i, _rel(out["v"][a:b], ref.v, 1e-4))
        assert _rel(lat[i], ref.lattice) < 1e-12, i
        if not ref.flags & mr.ERROR:
            for j in range(4):
                assert _rel(obs[:, i, j], ref_obs[:, i, j]) < 1e-12, (i, j)


@pytest.mark.parametrize("ensemble,fix_com", CASES)
def test_dyn_kernel_matches_restatement(ensemble, fix_com):
    iters = 40
    st = _state(ensemble, fix_com, SIZES)
    obs = _run(st, SIZES, iters)
    refs, ref_obs, clamped = _references(ensemble, fix_com, SIZES, iters)
    _compare(st, obs, refs, ref_obs, SIZES)
    assert all(ref.n_steps == iters - 1 for ref in refs)
    if ensemble in ("nvt_berendsen", "npt_berendsen"):
        assert clamped
    if ensemble == "npt_berendsen":
        assert np.abs(st.lattice.cpu().numpy() - np.stack(_batch(SIZES)[0])).max() > 1e-6


@pytest.mark.parametrize("ensemble", ["nvt_langevin", "npt_berendsen"])
def test_dyn_kernel_bitwise_reproducible_and_independent_of_the_batch(ensemble):
    fix_com = ensemble != "nvt_langevin"
    runs = []
    for _ in range(2):
        st = _state(ensemble, fix_com, SIZES)
        runs.append((st, _run(st, SIZES, 25)))
    (s0, o0), (s1, o1) = runs
    assert np.array_equal(o0, o1) and torch.equal(s0.pos, s1.pos) and torch.equal(s0.lattice, s1.lattice)
    r0 = s0.read()
    assert np.array_equal(r0["v"], s1.read()["v"])
    offs = np.concatenate([[0], np.cumsum(SIZES)])
    lats, poss, ms, vs = _batch(SIZES)
    from torch_m3gnet.dynamics import DynState

    for i in (2, 3):
        a, b = offs[i], offs[i + 1]
        pos = torch.tensor(poss[i], dtype=torch.float64, device=DEV)
        lat = torch.tensor(lats[i][None], dtype=torch.float64, device=DEV)
        alone = DynState(pos, lat, [0, b - a], ms[i], torch.tensor(vs[i], device=DEV), [TEMPS[i]], [SEEDS[i]], ensemble=ensemble,
                         fix_com=fix_com, **PARAMS)
        obs = _run(alone, SIZES, 25, rows=((a, b), i))
        r = alone.read()
        assert torch.equal(pos, s0.pos[a:b]) and torch.equal(lat[0], s0.lattice[i])
        assert np.array_equal(r["v"], r0["v"][a:b]) and np.array_equal(obs[:, 0], o0[:, i])
        assert r["flags"][0] == r0["flags"][i] and r["n_steps"][0] == r0["n_steps"][i]


def test_non_finite_force_freezes_that_structure_only():
    from torch_m3gnet import _lib

    iters, nan_at = 20, (6, 3 + 1 + 20)   # call 6: an atom of structure 2
    st = _state("nvt_langevin", False, SIZES)
    obs = _run(st, SIZES, iters, nan_at=nan_at)
    refs, ref_obs, _ = _references("nvt_langevin", False, SIZES, iters, nan_at=nan_at)
    _compare(st, obs, refs, ref_obs, SIZES)
    r = st.read()
    assert [bool(x & _lib.DYN_ERROR) for x in r["flags"]] == [False, False, True, False, False]
    assert list(r["n_steps"]) == [iters - 1] * 2 + [6] + [iters - 1] * 2
    assert np.array_equal(obs[6:, 2], np.repeat(obs[5:6, 2], iters - 6, axis=0))   # its observables stay those of call 5
    assert torch.isfinite(st.pos).all() and np.isfinite(r["v"]).all()


def test_dyn_step_capture_replays_bitwise():
    from torch_m3gnet.dynamics import dyn_step

    sizes = [3, 32, 1000]
    f, s = _forces(sizes, 0, 3)
    forces, stresses = torch.tensor(f, device=DEV), torch.tensor(s, device=DEV)
    for ensemble in ("nvt_langevin", "npt_berendsen"):
        eager = _state(ensemble, False, sizes, temps=TEMPS[:3], seeds=SEEDS[:3])
        graphed = _state(ensemble, False, sizes, temps=TEMPS[:3], seeds=SEEDS[:3])
        for _ in range(10):
            dyn_step(eager, forces, stresses)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            dyn_step(graphed, forces, stresses)
        for _ in range(10):
            g.replay()
        torch.cuda.synchronize()
        assert torch.equal(eager.pos, graphed.pos) and torch.equal(eager.lattice, graphed.lattice) and torch.equal(eager.obs, graphed.obs)
        re, rg = eager.read(), graphed.read()
        assert np.array_equal(re["v"], rg["v"]) and np.array_equal(re["n_steps"], rg["n_steps"]) and re["n_steps"][0] == 10


# ---- physics under the LJ-fitted model ---------------------------------------------------------------------------------------------
def _fitted_model():
    from torch_m3gnet.model.build import build_model_from_npz

    return build_model_from_npz(GOLDEN / "model_fitted_lj.npz").to(DEV)


def _fcc(a, n):
    grid = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1).reshape(-1, 1, 3)
    return (grid + FCC_BASE[None]).reshape(-1, 3) * a, np.eye(3) * n * a


def _total_energy(res):
    return res["log"]["e_pot"] + res["log"]["ke"]


def test_nve_under_the_fitted_model_conserves_energy():
    """The 108-atom setup of tests/test_gpu_md.py's NVE test through MolecularDynamics (cutoffs 4.76 / 4.38: in a gap of the fcc
    shells, since the reference model's energy jumps where a pair crosses the two-body cutoff)."""
    from oracle import m3gnet_oracle as orc
    from torch_m3gnet.dynamics import MolecularDynamics
    from torch_m3gnet.model.build import build_model

    rc, r3 = 4.76, 4.38
    params, cfg, elemental = orc.load_model_npz(GOLDEN / f"{CASE_MODEL['cu32fit']}.npz")
    model = build_model(rc, r3, cfg.l_max, cfg.n_max, cfg.num_types, cfg.embedding_dim, cfg.num_blocks, elemental_energies=elemental,
                        energy_scale=cfg.energy_scale, length_scale=cfg.length_scale)
    model.load_state_dict({k: v for k, v in params.items()})
    pos0, lat = _fcc(3.61, 3)
    mass = 63.546
    rng = np.random.default_rng(9)
    pos = pos0 + rng.normal(0, 0.01, pos0.shape)
    vel = rng.normal(0, np.sqrt(mr.KB * 50.0 / mass * mr.KAPPA), pos0.shape)
    vel -= vel.mean(0)

    def drift(dt, steps):
        md = MolecularDynamics(model.to(DEV), ensemble="nve", timestep=dt, skin=0.3)
        (res,) = md.run([lat], [pos], [np.full(108, 29)], steps, velocities=[vel], loginterval=1)
        assert not res["error"] and res["n_steps"] == steps
        e = _total_energy(res)
        return np.abs(e - e[0]).max(), np.ptp(res["log"]["e_pot"])

    d1, swing = drift(1.0, 300)
    d2, _ = drift(2.0, 150)
    print(f"NVE 300 fs: potential swing {swing:.3f} eV; total energy within {d1:.1e} eV at dt = 1 fs, {d2:.1e} eV at 2 fs")
    assert swing > 0.2 and d1 < 3e-4, (d1, swing)
    assert 2.0 < d2 / d1 < 8.0, (d1, d2)


def test_langevin_replica_batch_reaches_each_target():
    from torch_m3gnet.dynamics import MolecularDynamics

    pos, lat = _fcc(3.61, 3)
    temps = [100.0, 200.0, 300.0, 400.0]
    md = MolecularDynamics(_fitted_model(), ensemble="nvt_langevin", timestep=2.0, temperature=temps, friction=0.02, seed=5)
    res = md.run([lat] * 4, [pos] * 4, [np.full(108, 29)] * 4, 2000, loginterval=1)
    for r, t0 in zip(res, temps):
        assert not r["error"] and r["n_steps"] == 2000
        t_mean = r["log"]["t"][-1500:].mean()
        assert abs(t_mean / t0 - 1.0) < 0.05, (t0, t_mean)
    assert not np.array_equal(res[0]["positions"], res[1]["positions"])


def test_berendsen_nvt_cools_a_hot_start():
    from torch_m3gnet.dynamics import MolecularDynamics, maxwell_boltzmann

    pos, lat = _fcc(3.61, 3)
    vel = maxwell_boltzmann(np.full(108, 63.546), 600.0, 1)
    md = MolecularDynamics(_fitted_model(), ensemble="nvt_berendsen", timestep=2.0, temperature=300.0, taut=50.0)
    (res,) = md.run([lat], [pos], [np.full(108, 29)], 1000, velocities=[vel], loginterval=1)
    t = res["log"]["t"]
    assert t[0] == pytest.approx(600.0, rel=1e-6)
    assert abs(t[-500:].mean() / 300.0 - 1.0) < 0.05, t[-500:].mean()


def test_npt_berendsen_reaches_the_models_lattice_constant():
    from torch_m3gnet.data import MaterialGraphKey as K
    from torch_m3gnet.data.md import VerletGraph
    from torch_m3gnet.dynamics import MolecularDynamics
    from torch_m3gnet.nn import Gradient

    model = _fitted_model()
    pv = Gradient(model.model, pair_virial=True)
    z = np.full(32, 29)
    grid_a = np.linspace(3.48, 3.53, 11)
    e = []
    for a in grid_a:
        p, L = _fcc(a, 2)
        vg = VerletGraph([L], [z], 5.0, 4.0, skin=0.5, device=DEV)
        e.append(float(vg.step(pv, torch.tensor(p, device=DEV))[K.TOTAL_ENERGY][0]) / 32)
    c2, c1, _ = np.polyfit(grid_a, e, 2)
    a0 = -c1 / (2 * c2)
    assert 3.48 < a0 < 3.53 and c2 > 0
    pos, lat = _fcc(3.46, 2)
    md = MolecularDynamics(model, ensemble="npt_berendsen", timestep=2.0, temperature=10.0, taut=20.0, pressure=0.0, taup=100.0,
                           compressibility=0.01)
    (res,) = md.run([lat], [pos], [z], 500, loginterval=1)
    assert not res["error"]
    L = res["lattice"]
    assert np.abs(L - np.diag(np.diag(L))).max() < 1e-9 * np.abs(L).max()   # stays cubic
    assert np.ptp(np.diag(L)) < 1e-9 * L[0, 0]
    a_mean = (res["log"]["v"][-100:] ** (1 / 3)).mean() / 2
    assert abs(a_mean - a0) < 3e-3, (a_mean, a0)


def test_out_of_range_species_raises():
    from torch_m3gnet.dynamics import MolecularDynamics

    pos, lat = _fcc(3.5, 2)
    z = np.full(32, 29)
    z[3] = 200
    md = MolecularDynamics(_fitted_model(), ensemble="nve", temperature=10.0)
    with pytest.raises(ValueError):
        md.run([lat], [pos], [z], 3)
    with pytest.raises((IndexError, ValueError)):
        md.run([lat], [pos], [z], 3, masses=[np.full(32, 63.546)])
