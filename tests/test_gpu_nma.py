"""Normal-mode projection on the MI355X at kernel level (torch_m3gnet.normal_modes, C ABI m3g_nma_*; no model) against the numpy
restatement (tests/nma_reference.py), on one batch of four synthetic structures with random unitary eigenvectors, random masses, sites
plus random displacements and random velocities:
    (a) n_u = 1, supercell (2, 1, 3), all 6 q;
    (b) n_u = 4 with two species, (2, 2, 2), all 8 q and one q that is not commensurate;
    (c) n_u = 21 (3 n_u = 63, the largest LDS instantiation), (3, 1, 1), 2 q;
    (d) n_u = 2, (5, 5, 6) = 300 atoms, all 150 q: two chunks of the chunk table, 150 cells over 42 thread groups.
n_lags = 4 over 7 samples, so the ring wraps; every other sample completes its velocities from forces.

The bound.  A mode amplitude is a dot product of K = 3 N_s + 3 n_u terms (the Fourier sum, then the eigenvector) of a projector row
of unit norm with sqrt(m) x: gamma_K |a| |b| = K eps |sqrt(m) x|_2, times 8 for complex arithmetic and the last bits of the phase
(the restatement rounds its own 2 pi q.f, the library reduces q.f first): b = 8 eps (3 N_s + 3 n_u) |sqrt(m) x|_2, with x = v for Qdot
and x = u for Q, the norm taken over the largest sample.  A product of two amplitudes (|Qdot|^2, an acf term, m |v|^2) is then off by at
most 2 |sqrt(m) x| b + b^2, and a sum over T samples by T times that.  Counts are exact."""
import functools

import numpy as np
import pytest
import torch

import nma_reference as ref
from helpers import GOLDEN, record_line

pytestmark = pytest.mark.gpu
DEV = "cuda"
RECORD = "normal_modes.txt"
N_LAGS, N_SAMPLES, KICK = 4, 7, 0.5
NAMES = "abcd"


@functools.lru_cache(maxsize=None)
def case(name: str) -> dict:
    if name == "a":
        return ref.random_case(21, 1, (2, 1, 3), ref.all_qpoints((2, 1, 3)))
    if name == "b":
        return ref.random_case(22, 4, (2, 2, 2), np.concatenate([ref.all_qpoints((2, 2, 2)), [[0.137, 0.291, -0.413]]]), n_species=2)
    if name == "c":
        return ref.random_case(23, 21, (3, 1, 1), [[0.0, 0.0, 0.0], [1 / 3, 0.0, 0.0]], n_species=3)
    return ref.random_case(24, 2, (5, 5, 6), ref.all_qpoints((5, 5, 6)), n_species=2)


@functools.lru_cache(maxsize=None)
def frames(name: str):
    return ref.random_frames(case(name), 100 + NAMES.index(name), N_SAMPLES)


def use_forces(k: int) -> bool:
    return k % 2 == 1


@functools.lru_cache(maxsize=None)
def reference(name: str, remove_com: bool = True, n_samples: int = N_SAMPLES, nan_at: int = -1) -> ref.NmaReference:
    """The restatement of `name` after its first `n_samples` frames (computed once, shared, never changed); `nan_at`: that sample's
    velocity holds a NaN."""
    c = case(name)
    r = ref.NmaReference(c["lattice"], c["frac"], c["masses"], c["supercell"], c["qpoints"], c["eigenvectors"], N_LAGS, remove_com)
    for k, (pos, vel, force) in enumerate(frames(name)[:n_samples]):
        if k == nan_at:
            vel = vel.copy()
            vel[len(vel) // 2, 1] = np.nan
        r.sample(pos, vel, force if use_forces(k) else None, KICK)
    return r


class Batch:
    def __init__(self, names, remove_com=True, n_lags=N_LAGS):
        from torch_m3gnet.normal_modes import NmaState

        self.names = list(names)
        cs = [case(n) for n in self.names]
        self.state = NmaState([c["lattice"] for c in cs], [c["frac"] for c in cs], [c["masses"] for c in cs], [c["supercell"] for c in cs],
                              [c["qpoints"] for c in cs], [c["eigenvectors"] for c in cs], n_lags, remove_com, device=DEV)
        assert self.state.offsets.tolist() == np.concatenate([[0], np.cumsum([c["n_atoms"] for c in cs])]).tolist()

    def sample(self, k: int, nan_in=None, forces=None):
        """Frame k of every structure; `nan_in`: that structure's velocity holds a NaN; `forces`: overrides `use_forces(k)`."""
        from torch_m3gnet.normal_modes import nma_sample

        pos, vel, force = (np.concatenate([frames(n)[k][j] for n in self.names]) for j in range(3))
        if nan_in is not None:
            a = int(self.state.offsets[self.names.index(nan_in)])
            vel[a + case(nan_in)["n_atoms"] // 2, 1] = np.nan
        with_forces = use_forces(k) if forces is None else forces
        nma_sample(self.state, torch.tensor(pos, device=DEV), torch.tensor(vel, device=DEV),
                   torch.tensor(force, device=DEV) if with_forces else None, KICK)

    def run(self, n_samples=N_SAMPLES, nan_in=None, nan_at=-1):
        for k in range(n_samples):
            self.sample(k, nan_in if k == nan_at else None)
        return self

    def result(self, name: str) -> dict:
        """Everything the device holds of structure `name`: its accumulators and its last Qdot, Q."""
        s = self.names.index(name)
        st = self.state
        out = st.of_structure(st.read(), s)
        qdot, q = st.frame()
        a, b = int(st.mode_offsets[s]), int(st.mode_offsets[s + 1])
        out["frame_qdot"], out["frame_q"] = qdot[a:b].reshape(out["qdot2_sum"].shape), q[a:b].reshape(out["qdot2_sum"].shape)
        return out


def bounds(name: str, r: ref.NmaReference):
    """(b_v, b_u, per-product bound for v, for u) of the module docstring; the norms are the largest over the samples `r` accepted."""
    c = case(name)
    k = 3 * c["n_atoms"] + 3 * len(c["frac"])
    b_v, b_u = 8 * ref.EPS * k * r.max_norm_v, 8 * ref.EPS * k * r.max_norm_u
    return b_v, b_u, 2 * r.max_norm_v * b_v + b_v ** 2, 2 * r.max_norm_u * b_u + b_u ** 2


def compare(name: str, got: dict, r: ref.NmaReference) -> dict:
    """Asserts the bounds of the module docstring; returns the measured maxima as fractions of them."""
    b_v, b_u, p_v, p_u = bounds(name, r)
    t = max(r.n_samples, 1)
    assert got["n_samples"] == r.n_samples and np.array_equal(got["lag_count"], r.lag_count) and got["flags"] == r.flags
    worst = {"frame_qdot": np.abs(got["frame_qdot"] - r.last_qdot).max() / b_v, "frame_q": np.abs(got["frame_q"] - r.last_q).max() / b_u,
             "qdot2_sum": np.abs(got["qdot2_sum"] - r.qdot2_sum).max() / (t * p_v), "q2_sum": np.abs(got["q2_sum"] - r.q2_sum).max() / (t * p_u),
             "acf": np.abs(got["acf"] - r.acf).max() / (t * p_v), "kinetic_sum": abs(got["kinetic_sum"] - r.kinetic_sum) / (t * p_v)}
    for key, frac in worst.items():
        assert frac <= 1.0, (name, key, frac)
    return worst


@pytest.fixture(scope="module")
def batch_of_four():
    return Batch(NAMES).run()


def test_values_against_the_restatement(batch_of_four):
    for name in NAMES:
        r = reference(name)
        assert r.n_samples == N_SAMPLES and r.lag_count.tolist() == [7, 6, 5, 4]
        worst = compare(name, batch_of_four.result(name), r)
        c = case(name)
        record_line(RECORD, f"({name}) n_u {len(c['frac'])}, supercell {c['supercell']}, {len(c['qpoints'])} q, {N_SAMPLES} samples, {N_LAGS} lags: "
                            "largest error as a fraction of its bound: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))


def test_parseval_on_the_device(batch_of_four):
    """All commensurate q and unitary E: sum over modes of qdot2_sum equals kinetic_sum, which the device forms from the velocities."""
    for name in "abd":
        got = batch_of_four.result(name)
        total = got["qdot2_sum"][:8].sum() if name == "b" else got["qdot2_sum"].sum()   # (b) without its extra q
        _, _, p_v, _ = bounds(name, reference(name))
        err = abs(total - got["kinetic_sum"])
        record_line(RECORD, f"({name}) Parseval on the device: |sum qdot2_sum - kinetic_sum| = {err:.2e} = {err / got['kinetic_sum']:.1e} relative "
                            f"(bound {N_SAMPLES * p_v:.2e})")
        assert err <= N_SAMPLES * p_v


@pytest.mark.parametrize("remove_com", [True, False])
def test_velocity_completion(remove_com):
    """With forces and a kick the device projects vel + kick kappa F / m: the restatement is fed exactly those velocities, no forces."""
    names = "ab"
    batch = Batch(names, remove_com)
    for k in range(3):
        batch.sample(k, forces=True)
    for name in names:
        c = case(name)
        r = ref.NmaReference(c["lattice"], c["frac"], c["masses"], c["supercell"], c["qpoints"], c["eigenvectors"], N_LAGS, remove_com)
        for pos, vel, force in frames(name)[:3]:
            r.sample(pos, vel + KICK * (ref.KAPPA * force.astype(np.float64) / r.mass[:, None]))
        assert abs(r.last_qdot).max() > 0
        compare(name, batch.result(name), r)
    if not remove_com:   # the net momentum stayed in: the q = 0 modes differ from the run with it removed
        with_com = reference("a", True, 3)
        assert np.abs(batch.result("a")["frame_qdot"][0] - with_com.last_qdot[0]).max() > 1e-3 * with_com.norm_v


def test_a_structure_is_bitwise_the_same_alone_or_anywhere_in_a_batch(batch_of_four):
    alone, first, last = Batch("b").run().result("b"), Batch("bacd").run().result("b"), Batch("acdb").run().result("b")
    second = batch_of_four.result("b")
    for other in (first, last, second):
        assert sorted(other) == sorted(alone)
        for key, want in alone.items():
            assert np.array_equal(np.asarray(other[key]), np.asarray(want)), key
            if isinstance(want, np.ndarray) and want.dtype.kind in "fc":
                assert other[key].tobytes() == want.tobytes(), key


def test_a_nan_velocity_flags_its_structure_only(batch_of_four):
    """(c) gets a NaN velocity in its third sample: flagged, its accumulators stay at two samples (and later samples are refused),
    every other structure is bitwise what it is in the clean run."""
    from torch_m3gnet import _lib

    hurt = Batch(NAMES).run(nan_in="c", nan_at=2)
    got = hurt.result("c")
    assert got["flags"] == _lib.NMA_NONFINITE and got["n_samples"] == 2 and got["lag_count"].tolist() == [2, 1, 0, 0]
    r = reference("c", True, N_SAMPLES, 2)
    assert r.flags == 1 and r.n_samples == 2
    compare("c", got, r)
    two = Batch("c").run(2).result("c")   # the same bits as a run that stopped after two samples
    for key, want in two.items():
        assert np.array_equal(np.asarray(got[key]), np.asarray(want)) or key == "flags", key
    assert np.isfinite(got["acf"]).all() and np.isfinite(got["qdot2_sum"]).all()
    for name in "abd":
        clean, other = batch_of_four.result(name), hurt.result(name)
        assert other["flags"] == 0 and other["n_samples"] == N_SAMPLES
        for key, want in clean.items():
            assert np.array_equal(np.asarray(other[key]), np.asarray(want)), (name, key)


def test_no_autocorrelation_and_argument_checks():
    from torch_m3gnet.normal_modes import nma_sample

    batch = Batch("a", n_lags=0).run(2)
    got = batch.result("a")
    assert got["acf"].shape == (6, 3, 0) and got["lag_count"].shape == (0,) and got["n_samples"] == 2
    r = reference("a", True, 2)
    assert np.abs(got["frame_qdot"] - r.last_qdot).max() <= bounds("a", r)[0]
    with pytest.raises(ValueError):
        nma_sample(batch.state, torch.zeros(5, 3, dtype=torch.float64, device=DEV), torch.zeros(6, 3, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError):
        nma_sample(batch.state, torch.zeros(6, 3, dtype=torch.float64, device=DEV), torch.zeros(6, 3, dtype=torch.float32, device=DEV))


# ---- the convention, pinned against the library's own phonons -----------------------------------------------------------------------
A0 = 3.5025   # the fitted model's lattice constant (tests/test_gpu_phonon_modes.py)
FCC_BASE = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])


def full_force_constants(phi: np.ndarray, supercell) -> np.ndarray:
    """[N, 3, N, 3] from the compact layout Phi[u, j, a, b] (home atom u, supercell atom j = l n_u + v) by translation:
    Phi_full[l_i n_u + u, a, l_k n_u + v, b] = Phi[u, ((l_k - l_i) mod c) n_u + v, a, b], index arithmetic only."""
    n_u, n_s = phi.shape[:2]
    c = np.asarray(supercell)
    cells = ref.supercell_cells(supercell).astype(np.int64)
    full = np.zeros((n_s, 3, n_s, 3))
    for li, cell_i in enumerate(cells):
        shifted = (cells - cell_i[None]) % c[None]
        src = (shifted[:, 0] * c[1] + shifted[:, 1]) * c[2] + shifted[:, 2]   # the cell every l_k lands in
        j = (src[:, None] * n_u + np.arange(n_u)[None]).reshape(-1)
        for u in range(n_u):
            full[li * n_u + u] = phi[u][j].transpose(1, 0, 2)   # [a, k, b]
    return full


def test_convention_against_the_phonons_of_fcc_cu():
    """fcc Cu (conventional cell, the LJ-fitted model), phonons on (3, 3, 3); the same (3, 3, 3) as the MD supercell with all 27 q and E
    from `modes`.  A random displacement u of 1e-2 A (zero mean) and the harmonic force F = -Phi u, formed in numpy from
    `force_constants` (no engine call), are projected as displacement and, F / m, as "velocity": Qf + lambda Qu = 0 for every mode,
    lambda = sign(f) (f / THz unit)^2, to 1e-10 max |lambda| |sqrt(m) u| -- the level at which the existing tests hold `modes` to be
    eigenpairs, with margin.  A wrong phase sign, cell order or a transposed eigenvector breaks it at order one.
    Phi is the finite-difference matrix made symmetric, (Phi + Phi^T) / 2 over (atom, axis) pairs: the dynamical matrix the modes
    belong to is made Hermitian in the same way, (D + D^H) / 2 (include/m3gnet_hip.h), and the fp32 forces behind Phi leave an
    antisymmetric part of about 1e-7 of it, which is printed and which no choice of convention could remove."""
    from torch_m3gnet import _lib
    from torch_m3gnet.model.build import build_model_from_npz
    from torch_m3gnet.normal_modes import NmaState, commensurate_qpoints, nma_sample
    from torch_m3gnet.phonons import Phonons

    sc = (3, 3, 3)
    model = build_model_from_npz(GOLDEN / "model_fitted_lj.npz").to(DEV)
    (res,) = Phonons(model).run([np.eye(3) * A0], [FCC_BASE * A0], [np.full(4, 29)], sc)
    assert not res.error and np.array_equal(res.atomic_numbers, np.full(4, 29)) and np.allclose(res.positions, FCC_BASE * A0)
    q = commensurate_qpoints(sc)
    modes = res.modes(q)
    lam = np.sign(modes["frequencies"]) * (modes["frequencies"] / _lib.PH_THZ) ** 2
    frac = res.positions @ np.linalg.inv(res.lattice)
    state = NmaState([res.lattice], [frac], [res.masses], [sc], [q], [modes["eigenvectors"]], n_lags=0, remove_com=False, device=DEV)
    n = 4 * 27
    mass = np.tile(res.masses, 27)
    r0 = ref.site_fractions(frac, sc) @ res.lattice
    rng = np.random.default_rng(17)
    u = rng.normal(0.0, 1e-2, (n, 3))
    u -= u.mean(0)
    raw = full_force_constants(res.force_constants, sc).reshape(3 * n, 3 * n)
    sym = 0.5 * (raw + raw.T)
    scale = np.abs(lam).max() * np.sqrt((mass[:, None] * u * u).sum())
    worst = {}
    for label, phi in (("symmetric", sym), ("as measured", raw)):
        force = -(phi @ u.reshape(-1)).reshape(n, 3)
        nma_sample(state, torch.tensor(r0 + u, device=DEV), torch.tensor(force / mass[:, None], device=DEV))
        qf, qu = state.frame()
        assert np.abs(qu).max() > 1e-3 * np.sqrt((mass[:, None] * u * u).sum())
        worst[label] = np.abs(qf + lam.reshape(-1) * qu).max() / scale
    record_line(RECORD, f"fcc Cu (3, 3, 3), 27 q, 324 modes: max |Qf + lambda Qu| / (max |lambda| |sqrt(m) u|) = {worst['symmetric']:.2e} with the symmetric "
                        f"force constants (bound 1e-10), {worst['as measured']:.2e} with them as measured (their antisymmetric part "
                        f"{np.abs(raw - raw.T).max() / np.abs(raw).max():.1e} of the largest)")
    assert worst["symmetric"] <= 1e-10
