"""Batched finite-displacement phonons on the MI355X (torch_m3gnet.phonons, C ABI m3g_ph_*): the three launches against the numpy
restatement (tests/phonon_reference.py) -- displaced positions bit for bit, force constants of synthetic forces, dynamical matrices
and frequencies over random q -- bitwise independence of the batch, non-finite forces, and fcc Cu under the LJ-fitted model."""
import numpy as np
import pytest
import torch

import phonon_reference as pr
from helpers import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda"
FCC_BASE = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])


def _structures():
    """(lattice, positions, masses, supercell): 1 to 30 unit atoms, triclinic cells, several supercells."""
    rng = np.random.default_rng(3)
    out = [(np.eye(3) * 3.6, FCC_BASE * 3.6, np.full(4, 63.546), (3, 3, 3)),
           (np.array([[2.9, 0.0, 0.0], [0.4, 3.1, 0.0], [-0.3, 0.5, 3.3]]), np.array([[0.1, 0.2, 0.3]]), np.array([12.0]), (3, 4, 2)),
           (np.array([[4.6, 0.0, 0.0], [0.0, 4.6, 0.0], [0.0, 0.0, 2.96]]), rng.uniform(0, 3, (6, 3)), rng.uniform(10, 50, 6), (2, 2, 3))]
    lat30 = np.array([[9.0, 0.3, 0.0], [0.0, 8.5, 0.4], [0.2, 0.0, 7.0]])
    out.append((lat30, rng.uniform(0, 1, (30, 3)) @ lat30, rng.uniform(1, 200, 30), (1, 2, 1)))
    return out


def _state(structs, delta=0.01):
    from torch_m3gnet.phonons import PhononState

    return PhononState([s[0] for s in structs], [s[1] for s in structs], [s[2] for s in structs], [s[3] for s in structs], delta,
                       device=DEV)


def _forces(st, seed):
    return torch.tensor(np.random.default_rng(seed).normal(0, 1, (st.rows, 3)).astype(np.float32), device=DEV)


def test_displaced_positions_are_bitwise_the_restatement():
    from torch_m3gnet.phonons import ph_displace

    structs = _structures()
    st = _state(structs, delta=0.0137)
    pos = ph_displace(st).cpu().numpy()
    ref = np.concatenate([pr.displaced(L, p, n, 0.0137) for L, p, _, n in structs])
    assert np.array_equal(pos, ref)


@pytest.mark.parametrize("asr", [True, False])
def test_force_constants_match_the_restatement(asr):
    from torch_m3gnet.phonons import ph_force_constants

    structs = _structures()
    st = _state(structs)
    f = _forces(st, 1)
    ph_force_constants(st, f, asr)
    phi, sums, bad = st.phi.cpu().numpy(), st.sums.cpu().numpy(), st.nonfinite.cpu().numpy()
    fh = f.cpu().numpy()
    assert (bad == 0).all()
    for s, (_, p, _, n) in enumerate(structs):
        nu = len(p)
        rp, rs = pr.force_constants(fh[st.row_offsets[s]:st.row_offsets[s + 1]], nu, 0.01, asr)
        got = phi[st.pair_offsets[s]:st.pair_offsets[s + 1]].reshape(rp.shape)
        off = np.ones(rp.shape[:2], bool)
        off[np.arange(nu), np.arange(nu)] = not asr
        assert np.array_equal(got[off], rp[off])   # every entry but the ASR self terms: bit for bit
        assert np.abs(got - rp).max() <= 1e-12 * np.abs(rp).max()
        assert np.abs(sums[st.unit_offsets[s]:st.unit_offsets[s + 1]].reshape(nu, 3, 3) - rs).max() <= 1e-12 * np.abs(rp).max()
        if asr:
            assert np.abs(got.sum(axis=1)).max() <= 1e-12 * np.abs(rp).max() * got.shape[1]


def test_dynamical_matrices_and_frequencies_match_the_restatement():
    from torch_m3gnet.phonons import _eigvalsh, ph_dynamical_matrices, ph_force_constants

    structs = _structures()
    st = _state(structs)
    ph_force_constants(st, _forces(st, 2), True)
    phi = st.phi.cpu().numpy()
    rng = np.random.default_rng(5)
    qs = np.concatenate([np.zeros((1, 3)), [[0.5, 0, 0], [0.5, 0.5, 0.5], [0, -0.5, 0.5], [1.0, 0.25, -1.5]], rng.uniform(-1, 1, (6, 3))])
    for s, (L, p, m, n) in enumerate(structs):
        nu = len(p)
        table = pr.image_table(L, p, n)
        rphi = phi[st.pair_offsets[s]:st.pair_offsets[s + 1]].reshape(nu, -1, 3, 3)
        d = ph_dynamical_matrices(st, s, qs)
        lam = _eigvalsh(d).cpu().numpy()
        d = d.cpu().numpy()
        refs = [pr.dynamical_matrix(rphi, table, m, q) for q in qs]
        scale = max(np.abs(r).max() for r in refs)   # (D(0) is zero up to rounding with the sum rule: scaled by the whole set)
        for i, (q, ref) in enumerate(zip(qs, refs)):
            assert np.abs(d[i] - ref).max() <= 1e-12 * scale, (s, q)
            rl = np.linalg.eigvalsh(ref)
            assert np.abs(lam[i] - rl).max() <= 1e-10 * scale, (s, q)


def test_batch_independence_of_every_launch():
    from torch_m3gnet.phonons import ph_displace, ph_dynamical_matrices, ph_force_constants

    structs = _structures()
    q = np.random.default_rng(7).uniform(-0.5, 0.5, (9, 3))
    st = _state(structs)
    f = _forces(st, 3)
    pos = ph_displace(st).clone()
    ph_force_constants(st, f, True)
    for s in (0, 2, 3):
        alone = _state([structs[s]])
        a, b = int(st.row_offsets[s]), int(st.row_offsets[s + 1])
        assert torch.equal(ph_displace(alone), pos[a:b])
        ph_force_constants(alone, f[a:b].contiguous(), True)
        assert torch.equal(alone.phi, st.phi[int(st.pair_offsets[s]):int(st.pair_offsets[s + 1])])
        assert torch.equal(alone.sums, st.sums[int(st.unit_offsets[s]):int(st.unit_offsets[s + 1])])
        d = ph_dynamical_matrices(st, s, q)
        assert torch.equal(ph_dynamical_matrices(alone, 0, q), d) and torch.equal(ph_dynamical_matrices(st, s, q[3:5]), d[3:5])


def test_non_finite_force_flags_that_structure_only():
    from torch_m3gnet.phonons import ph_dynamical_matrices, ph_force_constants

    structs = _structures()
    st = _state(structs)
    f = _forces(st, 4)
    ph_force_constants(st, f, True)
    clean = st.phi.clone()
    bad = f.clone()
    bad[int(st.row_offsets[2]) + 17, 1] = float("nan")
    bad[int(st.row_offsets[2]) + 40, 2] = float("inf")
    ph_force_constants(st, bad, True)
    assert st.nonfinite.cpu().tolist() == [0, 0, 2, 0]
    a, b = int(st.pair_offsets[2]), int(st.pair_offsets[3])
    assert torch.isnan(st.phi[a:b]).all() and torch.isnan(st.sums[int(st.unit_offsets[2]):int(st.unit_offsets[3])]).all()
    assert torch.equal(st.phi[:a], clean[:a]) and torch.equal(st.phi[b:], clean[b:])
    assert torch.isnan(ph_dynamical_matrices(st, 2, [[0.1, 0.2, 0.3]])).all()


# ---- fcc Cu under the LJ-fitted model -----------------------------------------------------------------------------------------------
def _model():
    from torch_m3gnet.model.build import build_model_from_npz

    return build_model_from_npz(GOLDEN / "model_fitted_lj.npz").to(DEV)


@pytest.fixture(scope="module")
def cu():
    """The model's own lattice constant (a fit of E(a) of the 32-atom cell, as in test_gpu_relax.py) and its phonons (4-atom
    conventional cell, 3 x 3 x 3)."""
    from torch_m3gnet.data import MaterialGraphKey as K
    from torch_m3gnet.data.md import VerletGraph
    from torch_m3gnet.nn import Gradient
    from torch_m3gnet.phonons import Phonons

    model = _model()
    pv = Gradient(model.model, pair_virial=True)
    grid = np.stack(np.meshgrid(*[np.arange(2)] * 3, indexing="ij"), -1).reshape(-1, 1, 3)
    e = []
    grid_a = np.linspace(3.48, 3.53, 11)
    for a in grid_a:
        vg = VerletGraph([np.eye(3) * 2 * a], [np.full(32, 29)], 5.0, 4.0, skin=0.5, device=DEV)
        e.append(float(vg.step(pv, torch.tensor((grid + FCC_BASE[None]).reshape(-1, 3) * a, device=DEV))[K.TOTAL_ENERGY][0]))
    c2, c1, _ = np.polyfit(grid_a, e, 2)
    a0 = -c1 / (2 * c2)
    ph = Phonons(model)
    (res,) = ph.run([np.eye(3) * a0], [FCC_BASE * a0], [np.full(4, 29)], (3, 3, 3))
    return model, ph, a0, res


CONV_PATH = [(0, 0, 0), (0, 1, 0), (0.5, 1, 0), (0.75, 0.75, 0), (0, 0, 0), (0.5, 0.5, 0.5)]   # Gamma X W K Gamma L (conventional)


def test_fitted_cu_matches_the_restatement_on_single_evaluations(cu):
    from torch_m3gnet.data import MaterialGraphKey as K
    from torch_m3gnet.data.md import VerletGraph

    model, ph, a0, res = cu
    assert not res.error and res.residual_fmax < 1e-3, res.residual_fmax
    lat, pos = np.eye(3) * a0, FCC_BASE * a0
    ls, _ = pr.supercell(lat, pos, (3, 3, 3))
    rows = pr.displaced(lat, pos, (3, 3, 3), 0.01)
    f = []
    for c in range(25):   # every displaced supercell evaluated on its own
        vg = VerletGraph([ls], [np.full(108, 29)], 5.0, 4.0, skin=0.5, device=DEV)
        f.append(vg.step(ph.model, torch.tensor(rows[108 * c:108 * (c + 1)], device=DEV))[K.FORCES].cpu().numpy())
    phi, sums = pr.force_constants(np.concatenate(f), 4, 0.01, True)
    table = pr.image_table(lat, pos, (3, 3, 3))
    bands = res.band_structure(CONV_PATH, npts=9)
    worst = 0.0
    for q, got in zip(bands["q"], bands["frequencies"]):
        ref = pr.frequencies(pr.dynamical_matrix(phi, table, res.masses, q))
        err = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))   # 1e-3 THz below 1 THz, 1e-3 relative above
        worst = max(worst, float(err.max()))
    print(f"fitted Cu: worst band deviation from the single-evaluation restatement {worst:.2e} (THz or relative)")
    assert worst < 1e-3
    assert np.abs(res.force_constants - phi).max() < 1e-3 * np.abs(phi).max()


def test_fitted_cu_acoustic_modes_symmetry_and_stability(cu):
    model, ph, a0, res = cu
    print(f"fitted Cu: a0 {a0:.4f} A, raw ASR violation {res.asr_violation:.3e} eV/A^2, residual fmax {res.residual_fmax:.2e} eV/A")
    g = res.frequencies([[0, 0, 0]])[0]
    assert np.abs(g[:3]).max() < 1e-3, g
    # Gamma of the conventional cell: the acoustic triplet, then the primitive X modes of the three X points (TA 6-fold, LA 3-fold)
    assert np.ptp(g[3:9]) < 1e-3 and np.ptp(g[9:]) < 1e-3 and g[9] - g[8] > 0.1, g
    x = res.frequencies([[0.5, 0, 0], [0, 0.5, 0], [0, 0, 0.5]])
    assert np.abs(x - x[0]).max() < 1e-3, x   # the three cubic axes
    bands = res.band_structure(CONV_PATH, npts=21)
    assert bands["frequencies"].min() > -0.05, bands["frequencies"].min()
    assert 3.0 < bands["frequencies"].max() < 15.0


def test_fitted_cu_bitwise_alone_and_in_a_batch_and_split(cu):
    from torch_m3gnet.phonons import Phonons

    model, ph, a0, res = cu
    other = (np.eye(3) * 3.6, FCC_BASE * 3.6 + np.random.default_rng(1).normal(0, 0.02, (4, 3)), np.full(4, 29), (2, 2, 3))
    cu_args = (np.eye(3) * a0, FCC_BASE * a0, np.full(4, 29), (3, 3, 3))
    batch = ph.run(*zip(other, cu_args))
    q = np.random.default_rng(2).uniform(-0.5, 0.5, (20, 3))
    f = res.frequencies(q)
    r = batch[1]
    assert np.array_equal(r.force_constants, res.force_constants) and np.array_equal(r.asr_correction, res.asr_correction)
    assert r.residual_fmax == res.residual_fmax and np.array_equal(r.frequencies(q), f)
    (alone,) = ph.run(*zip(other))
    assert np.array_equal(alone.force_constants, batch[0].force_constants)
    # max_qpoints splits the q-points of one launch: every dynamical matrix is computed on its own
    assert np.allclose(Phonons(model, max_qpoints=7).run(*zip(cu_args))[0].frequencies(q), f, rtol=0, atol=1e-12 * np.abs(f).max())
    # max_atoms splits a structure's supercells over several engine batches: the engine's own rounding changes with its batch, so the
    # force constants agree to the fp32 forces' rounding, not bit for bit
    small = Phonons(model, max_atoms=300).run(*zip(cu_args, other))
    scale = np.abs(res.force_constants).max()
    dev = max(np.abs(small[0].force_constants - res.force_constants).max(), np.abs(small[1].force_constants - batch[0].force_constants).max())
    print(f"fitted Cu: max_atoms=300 against one batch per structure: max |dPhi| {dev:.2e} eV/A^2 ({dev / scale:.1e} of max |Phi|)")
    assert dev < 1e-5 * scale
    assert np.abs(small[0].frequencies(q) - f).max() < 1e-4


def test_fitted_cu_dos_and_thermal_properties(cu):
    from torch_m3gnet.phonons import KB_EV

    model, ph, a0, res = cu
    d = res.dos(mesh=(8, 8, 8), sigma=0.1)
    assert abs(np.trapezoid(d["dos"], d["frequency_points"]) - 12.0) < 1e-2
    t = res.thermal_properties([0.0, 300.0, 3000.0], mesh=(8, 8, 8))
    assert t["n_excluded"] == 3   # the acoustic modes at Gamma
    assert t["heat_capacity"][0] == 0.0 and t["free_energy"][0] > 0 and t["free_energy"][2] < t["free_energy"][1] < t["free_energy"][0]
    n_modes = 12 - 3 / 512
    assert abs(t["heat_capacity"][2] / (n_modes * KB_EV) - 1) < 5e-3
