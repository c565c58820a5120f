"""The batched Hermitian eigensolver, phonon eigenvectors and group velocities on the MI355X (torch_m3gnet.linalg, torch_m3gnet.phonons;
C ABI m3g_eigh_batched, m3g_ph_dynmat_gradient, m3g_ph_group_velocities): the solver against numpy.linalg.eigh, bitwise independence
of the batch, non-finite input, gradient and velocities against the numpy restatement (tests/phonon_modes_reference.py), and fcc Cu
under the LJ-fitted model.  Eigenvectors are compared on invariants only: residuals, orthonormality, projectors onto degenerate sets,
per-set traces of v and the per-set eigenvalues of W."""
import copy

import numpy as np
import pytest
import torch

import phonon_modes_reference as pm
import phonon_reference as pr
from helpers import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda"
FCC_BASE = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])


# ---- the eigensolver ----------------------------------------------------------------------------------------------------------------
def _unitary(rng, n):
    return np.linalg.qr(rng.normal(size=(n, n)) + 1j * rng.normal(size=(n, n)))[0]


def _matrices(n, seed):
    """{kind: Hermitian [n, n] complex128}"""
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(n, n)) + 1j * rng.normal(size=(n, n))
    rand = 0.5 * (a + a.conj().T)
    q = _unitary(rng, n)
    herm = lambda m: 0.5 * (m + m.conj().T)
    tiny = rng.normal(size=(n, n)) + 1j * rng.normal(size=(n, n))
    out = {"random": rand,
           "threefold": herm(q @ np.diag((np.arange(n) // 3 + 1.0)) @ q.conj().T),
           "diagonal": np.diag(rng.normal(size=n)).astype(np.complex128),
           "zero": np.zeros((n, n), dtype=np.complex128),
           "nearly_diagonal": np.diag(np.arange(1.0, n + 1)) + 1e-9 * herm(tiny - np.diag(np.diag(tiny))),
           "three_zeros": herm(q @ np.diag(np.where(np.arange(n) < 3, 0.0, 1.0 + np.arange(n))) @ q.conj().T),
           "real_symmetric": rand.real.astype(np.complex128)}
    out["scaled_1e8"] = 1e8 * out["threefold"]
    out["scaled_1e-8"] = 1e-8 * out["random"]
    return out


def _check_solution(h, w, v, info, tag):
    """(eigenvalue error, residual, orthonormality error) in the units of the bound, asserted."""
    from torch_m3gnet import _lib

    n = h.shape[0]
    norm = np.linalg.norm(h, 2)
    assert info & ~_lib.EIGH_SWEEPS_MASK == 0 and (info & _lib.EIGH_SWEEPS_MASK) <= 20, (tag, hex(info))
    assert (np.diff(w) >= 0).all(), tag
    de = np.abs(w - np.linalg.eigvalsh(h)).max()
    res = np.abs(h @ v - v * w[None]).max()
    orth = np.abs(v.conj().T @ v - np.eye(n)).max()
    assert de <= 1e-12 * norm and res <= 1e-12 * norm and orth <= 1e-12, (tag, de, res, orth, norm)
    return (de / norm if norm else de), (res / norm if norm else res), orth


@pytest.mark.parametrize("n", [1, 2, 3, 5, 6, 12, 18, 36, "max"])
def test_eigh_matches_numpy(n):
    from torch_m3gnet import _lib
    from torch_m3gnet.linalg import EIGH_MAX_N, eigh_batched

    n = EIGH_MAX_N if n == "max" else n
    mats = _matrices(n, 100 + n)
    a = torch.tensor(np.stack(list(mats.values())), device=DEV)
    w, v, info = eigh_batched(a)
    w0, v0, info0 = eigh_batched(a, eigenvectors=False)
    assert v0 is None and torch.equal(w0, w) and torch.equal(info0, info)   # the same eigenvalue bits without eigenvectors
    w, v, info = w.cpu().numpy(), v.cpu().numpy(), info.cpu().numpy()
    worst = np.zeros(3)
    for i, (kind, h) in enumerate(mats.items()):
        worst = np.maximum(worst, _check_solution(h, w[i], v[i], int(info[i]), (n, kind)))
    # a float64 (real symmetric) input is the same problem
    wr, vr, _ = eigh_batched(torch.tensor(mats["real_symmetric"].real.copy(), device=DEV))
    assert np.array_equal(wr.cpu().numpy(), w[list(mats).index("real_symmetric")])
    sweeps = int((info & _lib.EIGH_SWEEPS_MASK).max())
    print(f"eigh n = {n}: eigenvalues {worst[0]:.2e} |H|_2, residual {worst[1]:.2e} |H|_2, |V^H V - I| {worst[2]:.2e}, sweeps <= {sweeps}")


@pytest.mark.parametrize("n", [6, 12, 36])
def test_eigh_is_bitwise_independent_of_the_batch(n):
    from torch_m3gnet.linalg import eigh_batched

    rng = np.random.default_rng(n)
    a = rng.normal(size=(257, n, n)) + 1j * rng.normal(size=(257, n, n))
    a = 0.5 * (a + a.conj().transpose(0, 2, 1))
    probe = a[100].copy()
    a[0] = a[256] = probe
    batch = torch.tensor(a, device=DEV)
    w, v, info = eigh_batched(batch)
    w1, v1, i1 = eigh_batched(batch[100:101].clone())
    for k in (0, 100, 256):
        assert torch.equal(w[k], w1[0]) and torch.equal(v[k], v1[0]) and torch.equal(info[k], i1[0]), k
    w3, v3, i3 = eigh_batched(batch[99:102].clone())
    assert torch.equal(w3, w[99:102]) and torch.equal(v3, v[99:102]) and torch.equal(i3, info[99:102])
    assert not torch.equal(w[1], w[0])


def test_eigh_non_finite_input_flags_that_matrix_only():
    from torch_m3gnet import _lib
    from torch_m3gnet.linalg import eigh_batched

    rng = np.random.default_rng(9)
    a = rng.normal(size=(6, 7, 7)) + 1j * rng.normal(size=(6, 7, 7))
    a = 0.5 * (a + a.conj().transpose(0, 2, 1))
    clean = torch.tensor(a, device=DEV)
    w, v, info = eigh_batched(clean)
    bad = a.copy()
    bad[1, 2, 5] = np.nan            # upper triangle
    bad[3, 4, 4] = np.inf            # diagonal
    bad[4, 5, 2] = np.nan            # lower triangle: not read
    bad[4, 3, 3] = complex(bad[4, 3, 3].real, np.inf)   # imaginary part of the diagonal: not read
    wb, vb, ib = eigh_batched(torch.tensor(bad, device=DEV))
    ib = ib.cpu().numpy()
    for k in (1, 3):
        assert ib[k] & _lib.EIGH_NONFINITE and torch.isnan(wb[k]).all() and torch.isnan(torch.view_as_real(vb[k])).all(), k
    for k in (0, 2, 4, 5):
        assert ib[k] == int(info[k]) and torch.equal(wb[k], w[k]) and torch.equal(vb[k], v[k]), k
    w2, v2, i2 = eigh_batched(clean)   # the next call on the same stream
    assert torch.equal(w2, w) and torch.equal(v2, v) and torch.equal(i2, info)


# ---- gradient and velocities against the restatement --------------------------------------------------------------------------------
def _structures():
    """(lattice, positions, masses, supercell): 1 to 30 unit atoms, triclinic cells, several supercells (those of test_gpu_phonons.py)."""
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


QS = np.concatenate([np.zeros((1, 3)), [[0.5, 0, 0], [0.5, 0.5, 0.5], [0, -0.5, 0.5]], np.random.default_rng(5).uniform(-1, 1, (4, 3))])
DIRECTION = (1.0, 2.0, 3.0)
# Velocities of non-degenerate modes against the restatement.  Both sides apply the same formula to eigenvectors of the same matrix
# (equal to 1e-12), so they differ by the eigenvectors' own rounding, eps |D| / gap, times |dD| THZ^2 / (2 f).  Measured over the
# q-points above, as a fraction of the structure's largest velocity: 3.8e-15 (4 atoms), 4.2e-16 (1), 1.2e-14 (6), 1.7e-14 (30 atoms,
# the wide-matrix route; its random spectrum has the closest levels); asserted at 10 x the largest.
VELOCITY_BOUND = 1.7e-13


@pytest.fixture(scope="module")
def synthetic():
    from torch_m3gnet.phonons import ph_force_constants

    structs = _structures()
    st = _state(structs)
    ph_force_constants(st, _forces(st, 2), True)
    return structs, st, st.phi.cpu().numpy()


@pytest.mark.parametrize("s", [0, 1, 2, 3])
def test_gradient_and_velocities_match_the_restatement(synthetic, s):
    from torch_m3gnet import _lib
    from torch_m3gnet.linalg import EIGH_MAX_N
    from torch_m3gnet.phonons import _eigh, ph_dynamical_matrices, ph_dynamical_matrix_gradients, ph_group_velocities

    structs, st, phi = synthetic
    L, p, m, n = structs[s]
    nu = len(p)
    assert (3 * nu > EIGH_MAX_N) == (s == 3) and 3 * nu <= _lib.PH_GV_MAX_N   # the 30-atom structure takes the wide-matrix route
    table = pr.image_table(L, p, n)
    rphi = phi[st.pair_offsets[s]:st.pair_offsets[s + 1]].reshape(nu, -1, 3, 3)
    d = ph_dynamical_matrices(st, s, QS)
    g = ph_dynamical_matrix_gradients(st, s, QS)
    w, e = _eigh(d)
    v = ph_group_velocities(w, e, g, DIRECTION, 1e-4, 1e-3).cpu().numpy()
    g, w, e = g.cpu().numpy(), w.cpu().numpy(), e.cpu().numpy()
    refs = [pm.dynamical_matrix_gradient(rphi, table, m, q, L) for q in QS]
    scale = max(np.abs(r).max() for r in refs)
    assert g.shape == (len(QS), 3, 3 * nu, 3 * nu)
    worst_g = max(np.abs(g[i] - refs[i]).max() for i in range(len(QS))) / scale
    assert worst_g <= 1e-12, (s, worst_g)
    assert np.abs(g - g.conj().transpose(0, 1, 3, 2)).max() == 0.0            # Hermitian as written
    worst_v, vmax, compared = 0.0, 0.0, 0
    for i, q in enumerate(QS):
        dq = pr.dynamical_matrix(rphi, table, m, q)
        f, rv, sets, w_ref = pm.group_velocities(dq, refs[i], DIRECTION, 1e-4, 1e-3)
        got_f = np.sign(w[i]) * np.sqrt(np.abs(w[i])) * pm.THZ
        assert pm.degenerate_sets(got_f, 1e-4) == sets, (s, q)
        assert (v[i][f < 1e-3 - 1e-9] == 0.0).all()                            # below the cutoff: exactly 0
        vmax = max(vmax, np.abs(rv).max())
        for (b, c), wr in zip(sets, w_ref):
            if c - b == 1:
                worst_v = max(worst_v, np.abs(v[i, b] - rv[b]).max())
                compared += 1
            else:   # a degenerate set: the trace of v, the eigenvalues of W (= 2 f n.v / THZ^2) and the projector
                assert np.abs(v[i, b:c].sum(0) - rv[b:c].sum(0)).max() <= 1e-8 * max(np.abs(rv).max(), 1e-30), (s, q, b, c)
                nd = np.asarray(DIRECTION) / np.linalg.norm(DIRECTION)
                if f[b] >= 1e-3:
                    got_w = np.sort(2 * got_f[b:c] * (v[i, b:c] @ nd) / pm.THZ ** 2)
                    assert np.abs(got_w - wr).max() <= 1e-8 * np.abs(refs[i]).max(), (s, q, b, c)
                er = np.linalg.eigh(dq)[1]
                assert np.abs(e[i][:, b:c] @ e[i][:, b:c].conj().T - er[:, b:c] @ er[:, b:c].conj().T).max() <= 1e-8
    print(f"structure {s} ({nu} atoms): gradient {worst_g:.2e} of its largest entry, velocities of {compared} non-degenerate modes "
          f"{worst_v / vmax:.2e} of the largest velocity")
    assert compared > 3 * nu and worst_v <= VELOCITY_BOUND * vmax


def test_degenerate_sets_are_rotated_like_the_restatement():
    """Spectra with threefold and sixfold levels, random Hermitian derivatives: the per-set traces of v and the per-set eigenvalues of
    W match the restatement, one mode at a time where W has distinct eigenvalues; a set above M3G_PH_GV_MAX_SET is NaN, alone."""
    from torch_m3gnet import _lib
    from torch_m3gnet.linalg import eigh_batched
    from torch_m3gnet.phonons import ph_group_velocities

    rng = np.random.default_rng(11)
    n, nq = 18, 4
    lam = np.array([0.01, 0.01, 0.01, 0.04, 0.05, 0.05, 0.05, 0.05, 0.05, 0.05, 0.09, 0.1, 0.1, 0.12, 0.2, 0.2, 0.2, 0.3])
    d = np.stack([(lambda u: 0.5 * ((u * lam) @ u.conj().T + ((u * lam) @ u.conj().T).conj().T))(_unitary(rng, n)) for _ in range(nq)])
    g = rng.normal(size=(nq, 3, n, n)) + 1j * rng.normal(size=(nq, 3, n, n))
    g = 0.5 * (g + g.conj().transpose(0, 1, 3, 2))
    w, e, _ = eigh_batched(torch.tensor(d, device=DEV))
    v = ph_group_velocities(w, e, torch.tensor(g, device=DEV), DIRECTION, 1e-4, 1e-3).cpu().numpy()
    nd = np.asarray(DIRECTION) / np.linalg.norm(DIRECTION)
    for i in range(nq):
        f, rv, sets, w_ref = pm.group_velocities(d[i], g[i], DIRECTION, 1e-4, 1e-3)
        assert [c - b for b, c in sets] == [3, 1, 6, 1, 2, 1, 3, 1]
        scale = np.abs(rv).max()
        for (b, c), wr in zip(sets, w_ref):
            assert np.abs(v[i, b:c].sum(0) - rv[b:c].sum(0)).max() <= 1e-9 * scale
            assert np.abs(np.sort(2 * f[b:c] * (v[i, b:c] @ nd) / pm.THZ ** 2) - wr).max() <= 1e-9 * np.abs(g[i]).max()
            assert np.abs(v[i, b:c] - rv[b:c]).max() <= 1e-7 * scale      # W of a random derivative has distinct eigenvalues
    # one level of 17 modes: above the set capacity -> NaN for that set only
    big = np.concatenate([[0.02], np.full(_lib.PH_GV_MAX_SET + 1, 0.05)])
    wb, eb, _ = eigh_batched(torch.tensor(np.diag(big).astype(np.complex128)[None], device=DEV))
    gb = rng.normal(size=(1, 3, len(big), len(big))) + 0j
    vb = ph_group_velocities(wb, eb, torch.tensor(gb + gb.transpose(0, 1, 3, 2), device=DEV), DIRECTION, 1e-4, 1e-3).cpu().numpy()
    assert np.isfinite(vb[0, 0]).all() and np.isnan(vb[0, 1:]).all()


def test_gradient_and_velocities_are_bitwise_independent_of_the_batch(synthetic):
    from torch_m3gnet.phonons import _eigh, ph_dynamical_matrices, ph_dynamical_matrix_gradients, ph_force_constants, ph_group_velocities

    structs, st, _ = synthetic
    f = _forces(st, 2)
    q = np.random.default_rng(7).uniform(-0.5, 0.5, (9, 3))
    q[4] = (0.5, 0.0, 0.0)
    for s in (0, 3):
        alone = _state([structs[s]])
        ph_force_constants(alone, f[int(st.row_offsets[s]):int(st.row_offsets[s + 1])].contiguous(), True)
        g = ph_dynamical_matrix_gradients(st, s, q)
        assert torch.equal(ph_dynamical_matrix_gradients(alone, 0, q), g) and torch.equal(ph_dynamical_matrix_gradients(st, s, q[3:5]), g[3:5])
        w, e = _eigh(ph_dynamical_matrices(st, s, q))
        v = ph_group_velocities(w, e, g, DIRECTION)
        v1 = ph_group_velocities(w[3:5].contiguous(), e[3:5].contiguous(), g[3:5].contiguous(), DIRECTION)
        assert torch.equal(v1, v[3:5]) and torch.isfinite(v).all()
    # a flagged q (NaN eigenvalues) gets NaN, its neighbours are untouched
    wn = w.clone()
    wn[2] = float("nan")
    vn = ph_group_velocities(wn, e, g, DIRECTION)
    assert torch.isnan(vn[2]).all() and torch.equal(vn[:2], v[:2]) and torch.equal(vn[3:], v[3:])


# ---- fcc Cu under the LJ-fitted model -----------------------------------------------------------------------------------------------
A0 = 3.5025   # the model's lattice constant
CONV_PATH = [(0, 0, 0), (0, 1, 0), (0.5, 1, 0), (0.75, 0.75, 0), (0, 0, 0), (0.5, 0.5, 0.5)]   # Gamma X W K Gamma L (conventional)


@pytest.fixture(scope="module")
def cu():
    from torch_m3gnet.model.build import build_model_from_npz
    from torch_m3gnet.phonons import Phonons

    model = build_model_from_npz(GOLDEN / "model_fitted_lj.npz").to(DEV)
    args = ([np.eye(3) * A0], [FCC_BASE * A0], [np.full(4, 29)], (3, 3, 3))
    (res,) = Phonons(model).run(*args)
    (jac,) = Phonons(model, eigensolver="jacobi").run(*args)
    return res, jac


def _eigenvalues(f):
    return np.sign(f) * (f / pm.THZ) ** 2


def test_fitted_cu_jacobi_frequencies_equal_the_default(cu):
    res, jac = cu
    assert res.eigensolver == "embedding" and jac.eigensolver == "jacobi" and np.array_equal(res.force_constants, jac.force_constants)
    a, b = res.band_structure(CONV_PATH, npts=9)["frequencies"], jac.band_structure(CONV_PATH, npts=9)["frequencies"]
    la, lb = _eigenvalues(a), _eigenvalues(b)
    err = np.abs(la - lb).max() / np.abs(la).max()
    print(f"fitted Cu: jacobi against embedding eigenvalues along the path {err:.2e} of the largest")
    assert err <= 1e-10


def test_fitted_cu_modes_are_eigenpairs(cu):
    from torch_m3gnet.phonons import ph_dynamical_matrices

    res, _ = cu
    q = res.band_structure(CONV_PATH, npts=5)["q"]
    m = res.modes(q)
    f, e = m["frequencies"], m["eigenvectors"]
    assert f.shape == (len(q), 12) and e.shape == (len(q), 12, 12)
    d = ph_dynamical_matrices(res._state, res._s, q).cpu().numpy()
    lam = _eigenvalues(f)
    worst_r = worst_o = 0.0
    for i in range(len(q)):
        norm = np.linalg.norm(d[i], 2)
        worst_r = max(worst_r, np.abs(d[i] @ e[i] - e[i] * lam[i][None]).max() / norm)
        worst_o = max(worst_o, np.abs(e[i].conj().T @ e[i] - np.eye(12)).max())
    print(f"fitted Cu: modes residual {worst_r:.2e} |D|_2, |V^H V - I| {worst_o:.2e}")
    assert worst_r <= 1e-12 and worst_o <= 1e-12
    assert np.abs(_eigenvalues(f) - _eigenvalues(res.frequencies(q))).max() <= 1e-10 * np.abs(lam).max()


# Central differences of `frequencies` at h = 1e-4 1/A away from crossings (neighbouring levels more than 0.05 THz away).  What is
# seen is the O(h^2) term of the difference quotient, as in tests/test_phonon_modes_cpu.py (5.2e-6 of the largest velocity there for
# the LJ crystal's conventional cell).  The fp32 forces enter both sides through the same force constants and cancel; the rounding
# of the two eigenvalue solves behind the quotient, eps |D| THZ^2 / (2 f h) ~ 1e-16 x 0.5 x 244 / (2 x 3 x 1e-4) ~ 2e-11 THz A, is far
# below.  Measured: 1.08e-5 of the largest velocity; asserted at 10 x.
CU_FD_BOUND = 1.08e-4


def test_fitted_cu_velocities_equal_central_differences(cu):
    res, _ = cu
    h = 1e-4
    q_cart = np.random.default_rng(4).uniform(-0.1, 0.1, (6, 3)) + np.array([0.04, 0.015, -0.025])
    q = pm.fractional_q(res.lattice, q_cart)
    v = res.group_velocities(q)
    f = res.frequencies(q)
    assert v.shape == (6, 12, 3)
    worst, compared = 0.0, 0
    for a in range(3):
        e = np.zeros(3)
        e[a] = h
        fd = (res.frequencies(pm.fractional_q(res.lattice, q_cart + e)) - res.frequencies(pm.fractional_q(res.lattice, q_cart - e))) / (2 * h)
        gap = np.minimum(np.diff(f, axis=1, prepend=-np.inf), np.diff(f, axis=1, append=np.inf))
        away = gap > 0.05   # THz: away from crossings
        compared += int(away.sum())
        worst = max(worst, np.abs(v[..., a] - fd)[away].max())
    # max_qpoints splits the q-points of the launches: every q-point is computed on its own, so nothing changes
    split = copy.copy(res)
    split._max_q = 4
    assert np.array_equal(split.group_velocities(q), v)
    m, ms = res.modes(q), split.modes(q)
    assert np.array_equal(ms["frequencies"], m["frequencies"]) and np.array_equal(ms["eigenvectors"], m["eigenvectors"])
    print(f"fitted Cu: velocities against central differences of frequencies {worst / np.abs(v).max():.2e} of the largest ({compared} compared)")
    assert compared >= 36 and worst <= CU_FD_BOUND * np.abs(v).max()


def test_fitted_cu_sound_velocities_along_100(cu):
    res, _ = cu
    qx = 0.01   # 1/A
    q = pm.fractional_q(res.lattice, [[qx, 0, 0], [0, 0, 0]])
    v = res.group_velocities(q)
    f = res.frequencies(q)
    print(f"fitted Cu: [100] sound velocities (THz A) TA {v[0, 0, 0]:.3f} {v[0, 1, 0]:.3f} LA {v[0, 2, 0]:.3f}; f {f[0, :3]}")
    assert (v[0, :3, 0] > 0).all() and v[0, 2, 0] > v[0, 1, 0]
    # the two transverse branches: the cubic degeneracy holds to 1e-3 THz in the frequencies (section 7d), that is 1e-3 / q in f / q
    assert abs(v[0, 0, 0] - v[0, 1, 0]) <= 1e-3 / qx
    assert (v[1, :3] == 0.0).all()   # Gamma: the acoustic modes lie below the cutoff


def test_fitted_cu_projected_dos(cu):
    res, jac = cu
    sigma = 0.1
    d = jac.dos(mesh=(6, 6, 6), sigma=sigma)
    p = jac.projected_dos(mesh=(6, 6, 6), sigma=sigma)
    assert p["projected_dos"].shape == (4, 201) and np.array_equal(p["frequency_points"], d["frequency_points"])
    top = d["dos"].max()
    err = np.abs(p["projected_dos"].sum(0) - d["dos"]).max() / top
    # the four atoms are equivalent up to the fp32 forces: the frequencies keep the cubic degeneracies to 1e-3 THz (section 7d), and a
    # Gaussian of width sigma moves by at most 0.61 / sigma of its height per THz
    spread = np.abs(p["projected_dos"] - p["projected_dos"][0]).max() / top
    print(f"fitted Cu: projected DOS sums to the DOS within {err:.2e} of its maximum; spread over the four atoms {spread:.2e}")
    assert err <= 1e-12 and spread <= 0.61 * 1e-3 / sigma
    assert abs(np.trapezoid(p["projected_dos"].sum(0), p["frequency_points"]) - 12.0) < 1e-2
    e = res.projected_dos(mesh=(2, 2, 2), sigma=sigma, npts=11)["projected_dos"]   # (the default solver's result has the methods too)
    assert e.shape == (4, 11) and np.isfinite(e).all()
