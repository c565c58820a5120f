"""Normal-mode analysis without a GPU: the numpy restatement (tests/nma_reference.py) against closed forms, the host post-processing of
torch_m3gnet.normal_modes (fit_damped_cosine, kappa_rta, mode_statistics, commensurate_qpoints, spectral_energy_density) against exact
inputs and hand-computed arrays, and the argument checks, which raise before any device call."""
import numpy as np
import pytest

import nma_reference as ref


def _partnered_eigenvectors(rng, frac, qpoints):
    """Unitary E[q] with E[-q] = conj(E[q]) diag(exp(-2 pi i G.f_b)) for -q + G in the list (what a real dynamical matrix gives in the
    convention with the phase on atomic positions), so that a real displacement field splits cleanly between q and -q."""
    n3 = 3 * len(frac)
    q = np.asarray(qpoints)
    eig = np.zeros((len(q), n3, n3), dtype=np.complex128)
    done = np.zeros(len(q), dtype=bool)
    for i in range(len(q)):
        if done[i]:
            continue
        other = (-q[i]) % 1.0
        j = int(np.argmin(np.abs(q - other[None]).sum(1)))
        assert np.abs(q[j] - other).max() < 1e-12
        g = np.rint(q[i] + q[j])   # the reciprocal lattice vector G = q + q'
        if j == i:   # a real matrix behind the half phase
            o, _ = np.linalg.qr(rng.normal(size=(n3, n3)))
            eig[i] = np.repeat(np.exp(-1j * np.pi * (frac @ g)), 3)[:, None] * o
        else:
            eig[i] = ref.random_unitary(rng, n3)
            eig[j] = eig[i].conj() * np.repeat(np.exp(-2j * np.pi * (frac @ g)), 3)[:, None]
        done[i] = done[j] = True
    return eig


def test_restatement_parseval():
    """All commensurate q and unitary E: the map v -> Qdot is unitary on the 3 N_s mass-weighted components, so sum |Qdot|^2 =
    sum m |v|^2; the rounding of two sums of 3 N_s products."""
    for seed, n_u, sc in ((1, 1, (2, 1, 3)), (2, 4, (2, 2, 2)), (3, 2, (3, 2, 2))):
        case = ref.random_case(seed, n_u, sc, ref.all_qpoints(sc), n_species=2)
        r = ref.NmaReference(case["lattice"], case["frac"], case["masses"], sc, case["qpoints"], case["eigenvectors"], 3)
        for pos, vel, force in ref.random_frames(case, seed, 4):
            r.sample(pos, vel, force, 0.7)
        assert r.n_samples == 4 and r.lag_count.tolist() == [4, 3, 2]
        assert abs(r.qdot2_sum.sum() - r.kinetic_sum) <= 1e-13 * r.kinetic_sum
        # the displacement too, its mass-weighted mean removed
        assert abs(r.q2_sum.sum() - r.norm_u2_sum) <= 1e-13 * r.norm_u2_sum


def test_restatement_two_travelling_modes_in_closed_form():
    """Two travelling waves u_j = Re[A exp(2 pi i q.f_j) e_b exp(-i w t)] / sqrt(N_c m_b) with exact velocities: mode (q, nu) holds
    Q = A exp(-i w t) / 2, its partner at -q the conjugate, every other mode nothing, and acf[lag] = (T - lag) |A|^2 w^2 / 4
    exp(-i w lag dt): real part |A|^2 w^2 cos(w lag dt) / 4 per sample.  Bound: 1e-12 of the largest term."""
    rng = np.random.default_rng(5)
    sc, n_u, n_lags, n_frames, dt = (4, 3, 2), 3, 6, 9, 1.7
    case = ref.random_case(7, n_u, sc, ref.all_qpoints(sc), n_species=2)
    q = case["qpoints"]
    eig = _partnered_eigenvectors(rng, case["frac"], q)
    assert np.abs(np.einsum("qrn,qrm->qnm", eig.conj(), eig) - np.eye(3 * n_u)).max() < 1e-14
    picks = [(int(np.argmin(np.abs(q - np.array([0.25, 1 / 3, 0.0])).sum(1))), 4, 0.8 - 0.3j, 0.21),
             (int(np.argmin(np.abs(q - np.array([0.5, 2 / 3, 0.5])).sum(1))), 7, -0.2 + 0.5j, 0.057)]
    r = ref.NmaReference(case["lattice"], case["frac"], case["masses"], sc, q, eig, n_lags, remove_com=True)
    f_sites, mass, n_c = r.frac_sites, r.mass, r.n_cells
    for k in range(n_frames):
        u, v = np.zeros_like(r.r0), np.zeros_like(r.r0)
        for iq, nu, amp, w in picks:
            z = (amp * np.exp(2j * np.pi * (f_sites @ q[iq])) * np.exp(-1j * w * k * dt))[:, None] * np.tile(eig[iq][:, nu].reshape(n_u, 3), (n_c, 1))
            z = z / np.sqrt(n_c * mass)[:, None]
            u += z.real
            v += (-1j * w * z).real
        r.sample(r.r0 + u, v)
    want2 = np.zeros(r.qdot2_sum.shape)
    want_acf = np.zeros(r.acf.shape, dtype=np.complex128)
    lags = np.arange(n_lags)
    for iq, nu, amp, w in picks:
        partner = int(np.argmin(np.abs(q - ((-q[iq]) % 1.0)[None]).sum(1)))
        assert partner != iq
        want2[iq, nu] = want2[partner, nu] = n_frames * abs(amp) ** 2 * w ** 2 / 4
        want_acf[iq, nu] = (n_frames - lags) * abs(amp) ** 2 * w ** 2 / 4 * np.exp(-1j * w * lags * dt)
        want_acf[partner, nu] = want_acf[iq, nu].conj()
        assert abs(r.last_q[iq, nu] - amp * np.exp(-1j * w * (n_frames - 1) * dt) / 2) <= 1e-12 * abs(amp)
    top = want2.max()
    assert np.abs(r.qdot2_sum - want2).max() <= 1e-12 * top
    assert np.abs(r.acf - want_acf).max() <= 1e-12 * top
    assert np.abs(r.acf.real[picks[0][0], picks[0][1]] / r.lag_count - abs(picks[0][2]) ** 2 * picks[0][3] ** 2 * np.cos(picks[0][3] * lags * dt) / 4).max() <= 1e-12 * top


def test_restatement_flags_a_non_finite_sample_and_stops():
    case = ref.random_case(11, 2, (2, 2, 1), ref.all_qpoints((2, 2, 1)))
    r = ref.NmaReference(case["lattice"], case["frac"], case["masses"], case["supercell"], case["qpoints"], case["eigenvectors"], 2)
    frames = ref.random_frames(case, 1, 3)
    r.sample(*frames[0][:2])
    kept = (r.n_samples, r.kinetic_sum, r.qdot2_sum.copy(), r.acf.copy())
    bad = frames[1][1].copy()
    bad[3, 1] = np.nan
    r.sample(frames[1][0], bad)
    r.sample(*frames[2][:2])
    assert r.flags == 1 and (r.n_samples, r.kinetic_sum) == kept[:2] and np.array_equal(r.qdot2_sum, kept[2]) and np.array_equal(r.acf, kept[3])


@pytest.mark.parametrize("w_dt", [0.05, 0.3, 1.0])
@pytest.mark.parametrize("ratio", [1e-3, 0.02, 0.2])
@pytest.mark.parametrize("start", [1.0, 1.1])
def test_fit_recovers_an_exact_damped_cosine(w_dt, ratio, start):
    """The model is exact, so only the solver's convergence limits the answer: 1e-8 relative on both parameters, from the true
    frequency and from one 10 % off."""
    from torch_m3gnet.normal_modes import fit_damped_cosine

    dt, n = 4.0, 400
    omega = w_dt / dt
    gamma = ratio * omega
    t = np.arange(n) * dt
    c = 3.7 * np.exp(-gamma * t) * np.cos(omega * t)
    fit = fit_damped_cosine(c, dt, frequency=start * omega / (2 * np.pi) * 1e3)
    print(f"w dt {w_dt}, Gamma / w {ratio}, start x{start}: {fit['iterations']} iterations, frequency off by "
          f"{abs(fit['frequency'] * 2e-3 * np.pi / omega - 1):.1e}, linewidth by {abs(fit['linewidth'] / gamma - 1):.1e}, residual {fit['residual']:.1e}")
    assert fit["converged"]
    assert abs(fit["frequency"] * 2e-3 * np.pi - omega) <= 1e-8 * omega
    assert abs(fit["linewidth"] - gamma) <= 1e-8 * gamma
    assert fit["lifetime"] == pytest.approx(1.0 / (2.0 * gamma), rel=1e-7) and fit["residual"] <= 1e-9


def test_fit_starts_from_the_spectrum_peak_and_refuses_what_it_cannot_fit():
    from torch_m3gnet.normal_modes import fit_damped_cosine, spectral_energy_density

    dt, n, omega, gamma = 5.0, 300, 0.04, 0.002
    t = np.arange(n) * dt
    c = np.exp(-gamma * t) * np.cos(omega * t)
    fit = fit_damped_cosine(c, dt)
    assert abs(fit["frequency"] * 2e-3 * np.pi - omega) <= 1e-8 * omega and abs(fit["linewidth"] - gamma) <= 1e-8 * gamma
    sed = spectral_energy_density(np.stack([c, 2.0 * c]), dt)
    assert sed["sed"].shape == (2, n) and np.allclose(sed["sed"][1], 2.0 * sed["sed"][0])
    peak = sed["frequency"][np.argmax(sed["sed"][0])]
    assert abs(peak - omega / (2 * np.pi) * 1e3) <= 1e3 / (2 * n * dt)   # within one bin of the line
    assert sed["frequency"][1] == pytest.approx(1e3 / (2 * n * dt))
    for bad in (np.zeros(10), np.array([1.0, np.nan, 0.5, 0.2]), np.array([1.0, 0.5, 0.2]), -np.ones(8)):
        assert np.isnan(fit_damped_cosine(bad, dt)["frequency"])


def test_kappa_rta_by_hand():
    from torch_m3gnet.normal_modes import kappa_rta

    v = np.array([[[10.0, 0.0, 0.0], [0.0, 20.0, 0.0]], [[3.0, 4.0, 0.0], [1.0, 1.0, 1.0]]])   # THz A
    tau = np.array([[1000.0, 500.0], [200.0, np.nan]])                                          # fs
    kappa, left_out = kappa_rta(50.0, v, tau)
    unit = 1.380649e-23 * (100.0) ** 2 * 1e-15 / 1e-30   # kB (J/K) x (THz A in m/s)^2 x fs in s / A^3 in m^3
    want = np.zeros((3, 3))
    want[0, 0] = 100.0 * 1000.0 + 9.0 * 200.0
    want[1, 1] = 400.0 * 500.0 + 16.0 * 200.0
    want[0, 1] = want[1, 0] = 12.0 * 200.0
    assert left_out == 1 and np.allclose(kappa, want * unit / 50.0, rtol=1e-14, atol=0.0)
    assert unit == pytest.approx(1.380649e-4)
    # a negative lifetime, an infinite one, a frequency below the cutoff and a weight
    tau2 = np.array([[1000.0, -5.0], [np.inf, 300.0]])
    kappa2, left_out2 = kappa_rta(50.0, v, tau2, weights=0.5, frequencies=np.array([[0.0, 2.0], [2.0, 2.0]]), cutoff_frequency=1e-3)
    want2 = np.ones((3, 3)) * 300.0 * 0.5
    assert left_out2 == 3 and np.allclose(kappa2, want2 * unit / 50.0, rtol=1e-14)
    with pytest.raises(ValueError):
        kappa_rta(50.0, v[:, :, :2], tau)
    with pytest.raises(ValueError):
        kappa_rta(0.0, v, tau)


def test_mode_statistics_and_commensurate_qpoints_by_hand():
    from torch_m3gnet.dynamics import KAPPA, KB
    from torch_m3gnet.normal_modes import commensurate_qpoints, mode_statistics

    read = {"n_samples": 4, "qdot2_sum": np.array([[4.0 * KAPPA * KB * 300.0, 8.0]]), "q2_sum": np.array([[1.0, 2.0 / 0.01]])}
    out = mode_statistics(read, 300.0)
    assert np.allclose(out["mode_temperatures"], [[300.0, 2.0 / (KAPPA * KB)]], rtol=1e-14)
    assert out["effective_frequencies"][0, 1] == pytest.approx(0.2 / (2 * np.pi) * 1e3, rel=1e-14)   # sqrt(8 / 200) = 0.2 rad/fs
    assert out["equipartition_frequencies"][0, 0] == pytest.approx(out["effective_frequencies"][0, 0], rel=1e-14)   # a mode at 300 K
    assert np.isnan(mode_statistics({"n_samples": 2, "qdot2_sum": np.zeros(1), "q2_sum": np.zeros(1)})["effective_frequencies"]).all()
    q = commensurate_qpoints((2, 1, 3))
    assert np.array_equal(q, np.array([[0, 0, 0], [0, 0, 1 / 3], [0, 0, 2 / 3], [0.5, 0, 0], [0.5, 0, 1 / 3], [0.5, 0, 2 / 3]]))
    assert np.array_equal(q, ref.all_qpoints((2, 1, 3))) and len(commensurate_qpoints((5, 5, 6))) == 150
    with pytest.raises(ValueError):
        commensurate_qpoints((2, 0, 1))


def _state_arguments(n_u=2, supercell=(2, 1, 1), n_q=2):
    case = ref.random_case(3, n_u, supercell, np.zeros((n_q, 3)))
    return dict(lattices=[case["lattice"]], frac=[case["frac"]], masses=[case["masses"]], supercells=[supercell],
                qpoints=[case["qpoints"]], eigenvectors=[case["eigenvectors"]], n_lags=4)


@pytest.mark.parametrize("what", ["too_many_atoms", "eigenvector_shape", "qpoint_shape", "negative_lags", "transposed_stack", "mass_count"])
def test_state_arguments_are_refused_before_any_device_call(what, monkeypatch):
    from torch_m3gnet import _lib, normal_modes

    def no_device(*a, **k):
        raise AssertionError("the device layer was reached")

    monkeypatch.setattr(_lib, "load_library", no_device)
    monkeypatch.setattr(normal_modes, "state_tensor", no_device)
    kw = _state_arguments()
    if what == "too_many_atoms":
        assert _lib.NMA_MAX_N == _lib.EIGH_MAX_N == 64
        kw = _state_arguments(n_u=22)   # 3 n_u = 66
    elif what == "eigenvector_shape":
        kw["eigenvectors"] = [kw["eigenvectors"][0][:, :, :5]]
    elif what == "qpoint_shape":
        kw["qpoints"] = [np.zeros((2, 2))]
    elif what == "negative_lags":
        kw["n_lags"] = -1
    elif what == "transposed_stack":
        kw["eigenvectors"] = [kw["eigenvectors"][0][:1]]   # one matrix for two q-points
    elif what == "mass_count":
        kw["masses"] = [np.ones(3)]
    with pytest.raises(ValueError):
        normal_modes.NmaState(**kw)
    kw = _state_arguments(n_u=21)   # 3 n_u = 63 passes the checks and reaches the device layer
    with pytest.raises(AssertionError, match="device layer"):
        normal_modes.NmaState(**kw)


def test_driver_arguments_are_refused():
    from torch_m3gnet import _lib
    from torch_m3gnet.model.build import build_model
    from torch_m3gnet.normal_modes import NormalModeAnalysis

    model = build_model(5.0, 4.0, 3, 3, 95, 16, 1)
    with pytest.raises(ValueError):
        NormalModeAnalysis(model, production="npt")
    with pytest.raises(ValueError):
        NormalModeAnalysis(model, n_lags=-1)
    with pytest.raises(ValueError):
        NormalModeAnalysis(model, n_lags=_lib.NMA_MAX_LAGS + 1)
    with pytest.raises(ValueError):
        NormalModeAnalysis(model, sample_interval=0)
    with pytest.raises(ValueError):
        NormalModeAnalysis(model, temperature=0.0)
    with pytest.raises(TypeError):
        NormalModeAnalysis(model.model)
    md = NormalModeAnalysis(model, temperature=20.0, production="nvt_langevin", n_lags=8)
    with pytest.raises(ValueError):
        md.run([], (2, 2, 2), 10)


def test_exact_translations_at_gamma():
    """Eigenvectors with a 1e-6 admixture between the acoustic and the other modes at Gamma (and at a reciprocal lattice vector) come
    back with exact translations, orthonormal, the other modes moved by no more than the admixture; other q-points are untouched."""
    from torch_m3gnet.normal_modes import exact_translations

    rng = np.random.default_rng(8)
    n_u = 3
    frac, masses = rng.uniform(0, 1, (n_u, 3)), np.array([12.0, 55.0, 12.0])
    q = np.array([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0], [1.0, -2.0, 0.0]])
    eig = np.zeros((3, 9, 9), dtype=np.complex128)
    for i in range(3):
        t = np.zeros((9, 3), dtype=np.complex128)
        for a in range(3):
            t[a::3, a] = np.sqrt(masses / masses.sum()) * np.exp(-2j * np.pi * (frac @ q[i]))
        basis, _ = np.linalg.qr(np.concatenate([t, rng.normal(size=(9, 6)) + 1j * rng.normal(size=(9, 6))], axis=1))
        basis[:, :3] = t @ ref.random_unitary(rng, 3)   # (qr keeps the span of the first three columns)
        mix = np.eye(9) + 1e-6 * (rng.normal(size=(9, 9)) + 1j * rng.normal(size=(9, 9)))
        eig[i], _ = np.linalg.qr(basis[:, rng.permutation(9)] @ mix)
    eig[1] = ref.random_unitary(rng, 9)   # not a reciprocal lattice vector
    out = exact_translations(q, eig, frac, masses)
    assert np.array_equal(out[1], eig[1])
    for i in (0, 2):
        assert np.abs(out[i].conj().T @ out[i] - np.eye(9)).max() < 1e-14
        assert np.abs(out[i] - eig[i]).max() < 1e-5
        uniform = np.tile(np.eye(3), (n_u, 1)) * np.repeat(np.sqrt(masses) * np.exp(-2j * np.pi * (frac @ q[i])), 3)[:, None]
        overlap = np.abs(uniform.conj().T @ out[i])   # [3, 9]: of every mode with the three uniform displacements
        held = np.sort((overlap ** 2).sum(0))
        assert held[:6].max() < 1e-28 * masses.sum() and np.allclose(held[6:], masses.sum(), rtol=1e-13)
        assert (np.abs(uniform.conj().T @ eig[i]) ** 2).sum(0).min() > 1e-14   # the input did leak
    far = ref.random_unitary(rng, 9)[None]   # no translations among its columns: left alone
    assert np.array_equal(exact_translations(np.zeros((1, 3)), far, frac, masses), far)
