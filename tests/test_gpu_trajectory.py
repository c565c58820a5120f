"""Trajectory observables on the MI355X (torch_m3gnet.trajectory, C ABI m3g_traj_*) against the numpy restatement
(tests/trajectory_reference.py): the pair histogram to the last count, the ring correlations within fp64 summation-order noise,
bitwise reproducibility and independence of the batch, the full-step velocities against the integrator's, a NaN position, graph
capture, and a MolecularDynamics run with and without observables."""
import functools

import numpy as np
import pytest
import torch

import trajectory_reference as tr

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = [1, 2, 3, 257, 600]   # no pair; one pair; 257 = a full 256-atom tile + a one-atom tile; 600 = three tiles, the last part-filled
NSPEC = [1, 2, 3, 2, 3]
M = 3
SEED = 1
N_FRAMES = 11
KICK = 0.7


@functools.lru_cache(maxsize=None)
def _batch():
    """Cells (cubic, orthorhombic, left-handed, triclinic, perturbed cubic -- the last one the narrowest), species, masses and 11
    frames: unwrapped positions shifted by up to 40 lattice vectors per atom, then a random walk; velocities; float32 forces."""
    rng = np.random.default_rng(SEED)
    lats = [np.eye(3) * 10.4, np.diag([10.0, 11.0, 12.0]),
            np.array([[0.3, 10.2, 0.1], [10.1, -0.2, 0.4], [0.2, 0.3, 10.6]]),          # rows 0 and 1 swapped: det < 0
            np.array([[9.9, 0.0, 0.0], [2.0, 10.1, 0.0], [1.5, -1.2, 10.3]]),
            np.eye(3) * 9.0 + rng.normal(0, 0.05, (3, 3))]
    assert np.linalg.det(lats[2]) < 0
    species = [rng.permutation(np.arange(n) % k) for n, k in zip(SIZES, NSPEC)]
    masses = [rng.uniform(1.0, 200.0, n) for n in SIZES]
    pos0 = [(rng.uniform(0, 1, (n, 3)) + rng.integers(-40, 41, (n, 3))) @ L for n, L in zip(SIZES, lats)]
    n = sum(SIZES)
    pos = [np.concatenate(pos0)]
    for _ in range(N_FRAMES - 1):
        pos.append(pos[-1] + rng.normal(0, 0.1, (n, 3)))
    vel = [rng.normal(0, 0.01, (n, 3)) for _ in range(N_FRAMES)]
    forces = [rng.normal(0, 0.5, (n, 3)).astype(np.float32) for _ in range(N_FRAMES)]
    half = np.array([tr.perpendicular_widths(L).min() / 2 for L in lats])
    return dict(lats=np.stack(lats), species=species, masses=masses, pos=pos, vel=vel, forces=forces, half=half,
                offsets=np.concatenate([[0], np.cumsum(SIZES)]))


def _accumulate(n_samples, bins=64, n_lags=4, remove_com=True, max_species=M, r_max=None, only=None, pos=None, kick_all=False, graph=False):
    """Feed the first `n_samples` frames (odd samples kicked, or all) to a fresh TrajState of the batch, or of structure `only` alone;
    graph: through one captured traj_sample (every sample kicked)."""
    from torch_m3gnet.trajectory import TrajState, traj_sample

    b = _batch()
    off = b["offsets"]
    lo, hi, structs = (0, off[-1], range(len(SIZES))) if only is None else (off[only], off[only + 1], [only])
    offsets = np.concatenate([[0], np.cumsum([SIZES[s] for s in structs])])
    r_max = 0.999 * b["half"].min() if r_max is None else r_max
    st = TrajState(hi - lo, offsets, np.concatenate([b["species"][s] for s in structs]), np.concatenate([b["masses"][s] for s in structs]),
                   r_max, bins, n_lags, remove_com, max_species=max_species, device=DEV)
    lat = torch.tensor(b["lats"][list(structs)], dtype=torch.float64, device=DEV)
    pos = b["pos"] if pos is None else pos
    frames = [(torch.tensor(pos[k][lo:hi], device=DEV), torch.tensor(b["vel"][k][lo:hi], device=DEV),
               torch.tensor(b["forces"][k][lo:hi], device=DEV)) for k in range(n_samples)]
    if graph:
        p, v, f = (torch.empty_like(x) for x in frames[0])
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):   # one stream, no parallel branches; nothing executes here
            traj_sample(st, p, lat, v, f, KICK)
        for pk, vk, fk in frames:
            p.copy_(pk), v.copy_(vk), f.copy_(fk)
            g.replay()
    else:
        for k, (pk, vk, fk) in enumerate(frames):
            traj_sample(st, pk, lat, vk, fk if kick_all or k % 2 == 1 else None, KICK)
    torch.cuda.synchronize()
    out = st.read()
    if n_lags:
        out["frame_pos"], out["frame_vel"] = st.frame(0)
    return out


@functools.lru_cache(maxsize=None)
def _rdf_reference(bins, max_species, n_samples=3):
    b = _batch()
    off, r_max = b["offsets"], 0.999 * b["half"].min()
    H = np.zeros((len(SIZES), max_species * (max_species + 1) // 2, bins), np.uint64)
    margin = np.inf
    for k in range(n_samples):
        for s in range(len(SIZES)):
            h, mg = tr.histogram(b["pos"][k][off[s]:off[s + 1]], b["lats"][s], b["species"][s], r_max, bins, max_species)
            H[s] += h
            margin = min(margin, mg)
    return H, margin


@functools.lru_cache(maxsize=None)
def _corr_reference(remove_com):
    b = _batch()
    off = b["offsets"]
    refs = []
    for s in range(len(SIZES)):
        ref = tr.Correlations(b["masses"][s], b["species"][s], M, 4, remove_com)
        for k in range(N_FRAMES):
            rows = slice(off[s], off[s + 1])
            ref.sample(b["pos"][k][rows], b["vel"][k][rows], b["forces"][k][rows] if k % 2 == 1 else None, KICK)
        refs.append(ref)
    return refs


@pytest.mark.parametrize("bins,max_species", [(64, 3), (512, 8)], ids=["lds_histogram", "global_histogram"])
def test_rdf_counts_equal_the_reference(bins, max_species):
    """(512 bins x 36 species pairs x 4 bytes is beyond the LDS histogram: the counts go straight to the global accumulator.)"""
    H, margin = _rdf_reference(bins, max_species)
    print(f"closest pair distance to a bin edge or r_max: {margin:.3e} A")
    assert margin > 1e-9   # the input guard: then a last-ulp difference cannot move a count
    b = _batch()
    out = _accumulate(3, bins=bins, n_lags=0, max_species=max_species)
    assert H[0].sum() == 0 and H[1].sum() <= 3 and H[4].sum() > 100000
    assert np.array_equal(out["hist"], H)
    assert list(out["n_samples"]) == [3] * 5 and list(out["flags"]) == [0] * 5
    vol = np.abs(np.linalg.det(b["lats"]))
    assert np.abs(out["volume_sum"] / (3 * vol) - 1).max() < 1e-14
    # cross-species rows are where the reference has them, and every species pair of the batch is populated
    assert all(H[4][tr.pair_index(a, c, max_species)].sum() > 0 for a in range(3) for c in range(a, 3))


def test_rdf_range_flag_marks_only_the_cell_that_is_too_narrow():
    from torch_m3gnet import _lib

    half = _batch()["half"]
    r_max = 1.01 * half.min()
    assert (half < r_max).sum() == 1 and half.argmin() == 4
    out = _accumulate(2, n_lags=0, r_max=r_max)
    assert list(out["flags"]) == [0, 0, 0, 0, _lib.TRAJ_RDF_RANGE]


@pytest.mark.parametrize("remove_com", [True, False])
def test_correlations_match_the_reference(remove_com):
    """n_lags = 4 with 11 samples: the ring wraps twice and ends part-way; odd samples are kicked.  The gate is the reference's own
    worst-case rounding bound (trajectory_reference.Correlations: ~ n 2^-53 sum|terms| for the order of the sums, plus the
    centre-of-mass rounding where it is removed) -- measured worst case deviation / bound: profiles/trajectory.txt."""
    refs = _corr_reference(remove_com)
    out = _accumulate(N_FRAMES, bins=0, remove_com=remove_com)
    worst = 0.0
    for s, ref in enumerate(refs):
        assert list(out["lag_count"][s]) == [11, 10, 9, 8] == list(ref.lag_count)
        assert out["n_samples"][s] == N_FRAMES
        for got, want, bound in ((out["msd"][s], ref.msd, ref.bound_msd), (out["vacf"][s], ref.vacf, ref.bound_vacf)):
            dev = np.abs(got - want)
            with np.errstate(invalid="ignore", divide="ignore"):
                worst = max(worst, np.nanmax(np.where(bound > 0, dev / bound, 0.0)))
            assert (dev <= bound).all(), (s, dev, bound)
        assert np.array_equal(out["msd"][s][:, 0], np.zeros(M))
        assert (out["msd"][s][NSPEC[s]:] == 0).all() and (out["vacf"][s][NSPEC[s]:] == 0).all()   # species the structure does not hold
        if SIZES[s] > 1:
            assert (out["msd"][s][: NSPEC[s], 1:] > 0).all()
    print(f"remove_com={remove_com}: worst deviation / bound = {worst:.3e}")


def test_bitwise_reproducible_and_independent_of_the_batch():
    keys = ("hist", "msd", "vacf", "lag_count", "n_samples", "volume_sum", "flags", "frame_pos", "frame_vel")
    first, second = _accumulate(N_FRAMES), _accumulate(N_FRAMES)
    for key in keys:
        assert np.array_equal(first[key], second[key]), key
    off = _batch()["offsets"]
    for s in range(len(SIZES)):
        alone = _accumulate(N_FRAMES, only=s)
        for key in keys[:7]:
            assert np.array_equal(alone[key][0], first[key][s]), (s, key)
        for key in keys[7:]:
            assert np.array_equal(alone[key], first[key][off[s]:off[s + 1]]), (s, key)


@pytest.mark.parametrize("ensemble", ["nve", "nvt_langevin"])
def test_sampler_reconstructs_the_full_step_velocities(ensemble):
    """Sampling before each dyn_step: vacf at lag 0 is the mean of |v + (dt/2) kappa F / m|^2 over the calls, with v read from the
    integrator before each step; after the closing finish_only call the integrator holds the sampler's last reconstruction."""
    # the synthetic MD inputs of tests/test_gpu_dynamics.py, on purpose: the same states and `_forces` its kernel tests drive
    from test_gpu_dynamics import PARAMS, SEEDS, TEMPS, _batch as dyn_batch, _forces, _state
    from torch_m3gnet.dynamics import dyn_step
    from torch_m3gnet.trajectory import TrajState, traj_sample

    sizes, iters, dt = [3, 257], 6, PARAMS["dt"]
    st = _state(ensemble, False, sizes, temps=TEMPS[:2], seeds=SEEDS[:2])
    m = np.concatenate(dyn_batch(sizes)[2])
    species = np.concatenate([np.arange(n) % 2 for n in sizes])
    off = np.concatenate([[0], np.cumsum(sizes)])
    traj = TrajState(sum(sizes), off, species, m, n_lags=2, remove_com=False, device=DEV)
    want = np.zeros((2, 2))
    for k in range(iters):
        f, sv = _forces(sizes, k, 0)
        v = st.read()["v"]
        assert np.array_equal(st.velocities.cpu().numpy(), v)   # the view is the state's own velocities
        kick = 0.0 if k == 0 else dt / 2
        full = v + kick * (tr.KAPPA * f.astype(np.float64) / m[:, None])
        for s in range(2):
            for a in range(2):
                rows = np.arange(off[s], off[s + 1])[species[off[s]:off[s + 1]] == a]
                want[s, a] += (full[rows] ** 2).sum()
        ft = torch.tensor(f, device=DEV)
        traj_sample(traj, st.pos, None, st.velocities, ft, kick)
        dyn_step(st, ft, torch.tensor(sv, device=DEV), finish_only=(k == iters - 1))
    got = traj.read()
    assert list(got["lag_count"][:, 0]) == [iters, iters]
    counts = np.array([[2, 1], [129, 128]])
    mean_got, mean_want = got["vacf"][:, :, 0] / (counts * iters), want / (counts * iters)
    print("mean |v_full|^2, sampler / numpy - 1:", (mean_got / mean_want - 1).ravel())
    assert (np.abs(mean_got - mean_want) <= (257 + 32) * tr.U * mean_want).all()   # positive terms: n u sum|terms|
    v_end = st.read()["v"]
    _, v_last = traj.frame(0)
    assert (np.abs(v_last - v_end) <= 2 * np.spacing(np.abs(v_end))).all()
    assert not np.array_equal(v_end, v)   # (the finish kick did move them)


def test_nan_position_is_counted_nowhere_and_stays_in_its_structure():
    b = _batch()
    clean = _accumulate(3)
    atom = b["offsets"][3] + 5
    pos = [p.copy() for p in b["pos"][:3]]
    for p in pos:
        p[atom, 1] = np.nan
    out = _accumulate(3, pos=pos)
    for s in (0, 1, 2, 4):
        for key in ("hist", "msd", "vacf", "lag_count", "volume_sum", "flags"):
            assert np.array_equal(out[key][s], clean[key][s]), (s, key)
    rows = np.delete(np.arange(b["offsets"][3], b["offsets"][4]), 5)
    H = sum(tr.histogram(p[rows], b["lats"][3], b["species"][3][np.arange(SIZES[3]) != 5], 0.999 * b["half"].min(), 64, M)[0] for p in pos)
    assert np.array_equal(out["hist"][3], H) and H.sum() < clean["hist"][3].sum()
    assert np.isnan(out["msd"][3][b["species"][3][5], 1]) and list(out["n_samples"]) == [3] * 5


def test_captured_sample_replays_bitwise():
    """One traj_sample captured on static buffers, five frames copied in and replayed (the ring of four wraps): the ring position
    is device-resident, so the replays equal five eager samples."""
    eager, graphed = _accumulate(5, kick_all=True), _accumulate(5, graph=True)
    for key, val in eager.items():
        assert np.array_equal(val, graphed[key]), key
    assert list(eager["lag_count"][0]) == [5, 4, 3, 2] and list(eager["n_samples"]) == [5] * 5


def test_md_run_with_observables_leaves_the_trajectory_unchanged():
    from test_gpu_dynamics import _fcc, _fitted_model
    from torch_m3gnet.dynamics import KAPPA, MolecularDynamics
    from torch_m3gnet.trajectory import TrajectoryObservables

    pos0, lat = _fcc(3.5, 2)
    pos = pos0 + np.random.default_rng(4).normal(0, 0.02, pos0.shape)
    z = np.full(32, 29)
    md = MolecularDynamics(_fitted_model(), ensemble="nve", timestep=1.0, temperature=300.0, seed=3)
    (plain,) = md.run([lat], [pos], [z], 40, masses=[np.full(32, 63.546)], loginterval=2)
    obs_in = TrajectoryObservables(rdf_r_max=3.5, rdf_bins=70, n_lags=8, sample_interval=2)
    (res,) = md.run([lat], [pos], [z], 40, masses=[np.full(32, 63.546)], loginterval=2, observables=obs_in)
    assert "observables" not in plain
    for key in ("positions", "velocities", "forces"):
        assert np.array_equal(plain[key], res[key]), key
    for key, val in plain["log"].items():
        assert np.array_equal(val, res["log"][key]), key
    obs = res["observables"]
    assert obs["n_samples"] == 21 and obs["rdf_valid"] and list(obs["species"]) == [29]
    assert list(obs["lag_count"]) == [21 - l for l in range(8)] and np.array_equal(obs["time"], 2.0 * np.arange(8))
    assert obs["msd"][0][0] == 0.0 and (obs["msd"][0][1:] > 0).all()
    ke = res["log"]["ke"]
    assert len(ke) == 21
    from_vacf = 32 * 63.546 * obs["vacf"][0][0] / (2 * KAPPA)
    print("mean KE of the log / KE from vacf(0) - 1:", ke.mean() / from_vacf - 1)
    assert abs(ke.mean() / from_vacf - 1) < 1e-10
    assert obs["g_total"][obs["r_edges"][1:] <= 2.0].max() == 0.0 and obs["g_total"].max() > 1.0
    first_shell = obs["coordination"][0][0][np.searchsorted(obs["r_edges"], 3.0) - 1]
    assert abs(first_shell - 12.0) < 0.5
