"""Batched FIRE relaxation on the MI355X (torch_m3gnet.relax, C ABI m3g_fire_*): the kernel against the numpy restatement
(tests/fire_reference.py), bitwise reproducibility and independence of the batch, freezing, errors, and relaxations under the
LJ-fitted model with the cell fixed and relaxed."""
import numpy as np
import pytest
import torch

import fire_reference as fr
from helpers import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = [1, 3, 32, 1000, 10000]
FCC_BASE = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])


def _batch(sizes, seed=0):
    rng = np.random.default_rng(seed)
    lats, poss = [], []
    for n in sizes:
        L = np.eye(3) * (12.0 * n) ** (1 / 3) + rng.normal(0, 0.05, (3, 3))
        lats.append(L)
        poss.append(rng.uniform(0, 1, (n, 3)) @ L)
    return lats, poss


def _forces(sizes, k, seed):
    """Seeded forces / stresses of iteration k: a fixed direction per run (P > 0 streaks, so dt grows), sign flips at some
    iterations (P < 0), one large force (maxstep clips even the 1-atom structure)."""
    rng = np.random.default_rng(seed)
    n = sum(sizes)
    base = rng.normal(0, 1, (n, 3))
    sbase = rng.normal(0, 1e-3, (len(sizes), 6))
    r = np.random.default_rng([seed, k])
    sign = -1.0 if k in (9, 21, 22, 33) else 1.0
    scale = 100.0 if k == 14 else 1.0
    f = (scale * sign * (base + 0.3 * r.normal(0, 1, (n, 3)))).astype(np.float32)
    st = (sign * (sbase + 3e-4 * r.normal(0, 1, sbase.shape))).astype(np.float32)
    return f, st


def _run_kernel(sizes, relax_cell, iters, seed=0, fmax=1e-8, forces=None):
    from torch_m3gnet.relax import FireState, fire_step

    lats, poss = _batch(sizes, seed)
    pos = torch.tensor(np.concatenate(poss), dtype=torch.float64, device=DEV)
    lat = torch.tensor(np.stack(lats), dtype=torch.float64, device=DEV)
    st = FireState(pos, lat, np.concatenate([[0], np.cumsum(sizes)]), relax_cell=relax_cell, fmax=fmax)
    for k in range(iters):
        f, s = forces(k) if forces else _forces(sizes, k, seed)
        fire_step(st, torch.tensor(f, device=DEV), torch.tensor(s, device=DEV))
    torch.cuda.synchronize()
    return st, st.read()


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize("relax_cell", [False, True])
def test_fire_kernel_matches_restatement(relax_cell):
    sizes, iters = SIZES, 40
    st, out = _run_kernel(sizes, relax_cell, iters)
    lats, poss = _batch(sizes)
    refs = [fr.FireReference(p, L, relax_cell, 1e-8) for p, L in zip(poss, lats)]
    offs = np.concatenate([[0], np.cumsum(sizes)])
    for k in range(iters):
        f, s = _forces(sizes, k, 0)
        for i, ref in enumerate(refs):
            ref.step(f[offs[i]:offs[i + 1]].astype(np.float64), s[i].astype(np.float64))
    pos, lat = st.pos.cpu().numpy(), st.lattice.cpu().numpy()
    N = offs[-1]
    for i, ref in enumerate(refs):
        a, b = offs[i], offs[i + 1]
        assert out["flags"][i] == ref.flags and out["n_steps"][i] == ref.n_steps == iters, i
        assert out["dt"][i] == ref.dt and out["a"][i] == ref.a and out["n"][i] == ref.n, (i, out["dt"][i], ref.dt, out["n"][i], ref.n)
        x, v = out["x"][a:b], out["v"][a:b]
        if relax_cell:
            x = np.concatenate([x, out["x"][N + 3 * i:N + 3 * i + 3]])
            v = np.concatenate([v, out["v"][N + 3 * i:N + 3 * i + 3]])
        assert _rel(x, ref.X) < 1e-12 and _rel(v, ref.v) < 1e-12, i
        assert _rel(pos[a:b], ref.pos) < 1e-12 and _rel(lat[i], ref.lattice) < 1e-12, i
    # the run took both branches and clipped
    assert {ref.n for ref in refs} != {0} and min(ref.dt for ref in refs) < 0.1
    assert not relax_cell or np.abs(lat - np.stack(lats)).max() > 1e-6


def test_fire_kernel_bitwise_reproducible_and_independent_of_the_batch():
    runs = [_run_kernel(SIZES, True, 25) for _ in range(2)]
    for key in ("flags", "n_steps", "dt", "a", "n", "x", "v"):
        assert np.array_equal(runs[0][1][key], runs[1][1][key]), key
    assert torch.equal(runs[0][0].pos, runs[1][0].pos) and torch.equal(runs[0][0].lattice, runs[1][0].lattice)
    # structure 2 (32 atoms) and 3 (1,000 atoms) alone, with the same inputs as inside the batch
    offs = np.concatenate([[0], np.cumsum(SIZES)])
    N = offs[-1]
    lats, poss = _batch(SIZES)
    for i in (2, 3):
        a, b = offs[i], offs[i + 1]

        def forces(k, i=i, a=a, b=b):
            f, s = _forces(SIZES, k, 0)
            return np.ascontiguousarray(f[a:b]), np.ascontiguousarray(s[i:i + 1])

        from torch_m3gnet.relax import FireState, fire_step

        pos = torch.tensor(poss[i], dtype=torch.float64, device=DEV)
        lat = torch.tensor(lats[i][None], dtype=torch.float64, device=DEV)
        st = FireState(pos, lat, [0, b - a], relax_cell=True, fmax=1e-8)
        for k in range(25):
            f, s = forces(k)
            fire_step(st, torch.tensor(f, device=DEV), torch.tensor(s, device=DEV))
        alone = st.read()
        batch = runs[0][1]
        assert torch.equal(pos, runs[0][0].pos[a:b]) and torch.equal(lat[0], runs[0][0].lattice[i])
        assert np.array_equal(alone["x"][: b - a], batch["x"][a:b]) and np.array_equal(alone["x"][b - a:], batch["x"][N + 3 * i:N + 3 * i + 3])
        assert np.array_equal(alone["v"][: b - a], batch["v"][a:b])
        for key in ("dt", "a", "n", "flags", "n_steps"):
            assert alone[key][0] == batch[key][i], key


def test_converged_structure_is_frozen_while_another_steps():
    from torch_m3gnet import _lib
    from torch_m3gnet.relax import FireState, fire_step

    sizes = [32, 32]
    lats, poss = _batch(sizes, seed=4)
    pos = torch.tensor(np.concatenate(poss), dtype=torch.float64, device=DEV)
    lat = torch.tensor(np.stack(lats), dtype=torch.float64, device=DEV)
    st = FireState(pos, lat, [0, 32, 64], relax_cell=True, fmax=1e-2)
    snaps = []
    for k in range(20):
        f, s = _forces(sizes, k, 4)
        if k >= 6:   # structure 0: forces and stresses far below fmax from here on
            f[:32] *= 1e-4
            s[0] *= 1e-4
        fire_step(st, torch.tensor(f, device=DEV), torch.tensor(s, device=DEV))
        torch.cuda.synchronize()
        snaps.append((pos.clone(), lat.clone(), st.read(), st.n_unconverged))
    p6, l6, r6, _ = snaps[6]
    assert r6["flags"][0] & _lib.FIRE_CONVERGED and r6["n_steps"][0] == 6
    for p, l, r, unconv in snaps[6:]:
        assert torch.equal(p[:32], p6[:32]) and torch.equal(l[0], l6[0])
        assert r["n_steps"][0] == 6 and r["dt"][0] == r6["dt"][0] and np.array_equal(r["x"][:32], r6["x"][:32])
        assert unconv == 1
    assert snaps[-1][2]["n_steps"][1] == 20 and not torch.equal(snaps[-1][0][32:], p6[32:])


def test_non_finite_force_flags_that_structure_only():
    from torch_m3gnet import _lib
    from torch_m3gnet.relax import FireState, fire_step

    sizes = [3, 32, 1000]
    lats, poss = _batch(sizes, seed=5)
    pos = torch.tensor(np.concatenate(poss), dtype=torch.float64, device=DEV)
    lat = torch.tensor(np.stack(lats), dtype=torch.float64, device=DEV)
    st = FireState(pos, lat, [0, 3, 35, 1035], relax_cell=True, fmax=1e-8)
    for k in range(10):
        f, s = _forces(sizes, k, 5)
        if k == 4:
            f[3 + 7, 1] = np.nan
        if k == 6:
            s[2, 3] = np.inf
        if k in (4, 6):
            before = (pos.clone(), lat.clone())
        fire_step(st, torch.tensor(f, device=DEV), torch.tensor(s, device=DEV))
        if k == 4:
            torch.cuda.synchronize()
            assert torch.equal(pos[3:35], before[0][3:35]) and torch.equal(lat[1], before[1][1])
        if k == 6:
            torch.cuda.synchronize()
            assert torch.equal(pos[35:], before[0][35:]) and torch.equal(lat[2], before[1][2])
    r = st.read()
    assert [bool(x & _lib.FIRE_ERROR) for x in r["flags"]] == [False, True, True]
    assert list(r["n_steps"]) == [10, 4, 6]
    assert torch.isfinite(pos).all() and torch.isfinite(lat).all() and st.n_unconverged == 1


# ---- physics under the LJ-fitted model ---------------------------------------------------------------------------------------------
def _model():
    from torch_m3gnet.model.build import build_model_from_npz

    return build_model_from_npz(GOLDEN / "model_fitted_lj.npz").to(DEV)


def _fcc(a, n=2):
    grid = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1).reshape(-1, 1, 3)
    return (grid + FCC_BASE[None]).reshape(-1, 3) * a, np.eye(3) * n * a


def test_fixed_cell_relaxation_returns_to_perfect_fcc():
    from torch_m3gnet.relax import Relaxer

    pos0, lat = _fcc(3.45)
    pos = pos0 + np.random.default_rng(7).normal(0, 0.05, pos0.shape)
    (res,) = Relaxer(_model(), relax_cell=False).relax([lat], [pos], [np.full(32, 29)], fmax=0.002, steps=500)
    assert res["converged"] and not res["error"] and 0 < res["n_steps"] < 500
    assert np.sqrt((res["forces"] ** 2).sum(1).max()) < 0.01
    assert np.array_equal(res["lattice"], lat)
    shift = (pos - pos0).mean(0)   # FIRE conserves sum v when sum f = 0
    assert np.abs(res["positions"] - (pos0 + shift)).max() < 1e-3


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
    (res,) = Relaxer(model, relax_cell=True).relax([lat], [pos], [z], fmax=0.01, steps=500)
    assert res["converged"] and not res["error"], res["n_steps"]
    L = res["lattice"]
    assert np.abs(L - np.diag(np.diag(L))).max() < 2e-3   # stays cubic
    assert np.abs(np.diag(L) / 2 - a0).max() < 2e-3, (np.diag(L) / 2, a0)


def test_batch_relaxation_equals_relaxing_each_alone():
    from torch_m3gnet.relax import Relaxer

    rng = np.random.default_rng(9)
    p32, l32 = _fcc(3.46)
    p108, l108 = _fcc(3.55, 3)
    z = np.load(GOLDEN / "case_mixfit_doc.npz")
    first = z["in_batch"] == 0
    cells = [(l32, p32 + rng.normal(0, 0.04, p32.shape), np.full(32, 29)),
             (l108, p108 + rng.normal(0, 0.04, p108.shape), np.full(108, 29)),
             (z["in_lattice"][0].astype(np.float64), z["in_pos"][first].astype(np.float64), z["in_atom_types"][first] + 1)]
    relaxer = Relaxer(_model(), relax_cell=True)
    kw = dict(fmax=0.05, steps=150)
    together = relaxer.relax(*zip(*cells), **kw)
    for c, t in zip(cells, together):
        (alone,) = relaxer.relax([c[0]], [c[1]], [c[2]], **kw)
        assert alone["converged"] == t["converged"] and alone["error"] == t["error"] is False
        assert abs(alone["total_energy"] - t["total_energy"]) / len(c[2]) < 1e-5
        assert np.abs(alone["positions"] - t["positions"]).max() < 1e-4
    assert together[0]["converged"] and together[1]["converged"]


def test_out_of_range_species_raises():
    from torch_m3gnet.relax import Relaxer

    pos, lat = _fcc(3.5)
    z = np.full(32, 29)
    z[3] = 200
    with pytest.raises((IndexError, ValueError)):
        Relaxer(_model()).relax([lat], [pos], [z], steps=3)
