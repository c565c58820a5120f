"""ReverseNEMD (torch_m3gnet.transport) on the MI355X under the LJ-fitted model, in the setup of tests/test_gpu_dynamics.py's NVE test
(cutoffs 4.76 / 4.38, a = 3.61): a 2 x 2 x 8 fcc Cu cell of 128 atoms, 8 slabs along z (the cell's origin a quarter of a lattice
constant below an atomic plane, so that every slab holds two whole planes, 16 atoms), 50 K, dt = 1 fs.  One run with an exchange every
10 steps and one control without exchanges from the same start, shared by the tests below; every measured figure goes to
profiles/rnemd.txt through helpers.record_line.

200 Langevin steps, then 700 NVE steps, not more: under this fixture model (its energy jumps where a pair crosses the two-body cutoff)
plain NVE in this cell at 50 K keeps the total energy to 1e-3 eV for about 700 steps and then runs away -- measured without any
exchange, with skins of 0.3, 0.5 and 1.0 A alike: -0.017 eV at NVE step 800, -0.58 eV at 1,100, the temperature 43 K -> 960 K by 1,300
(profiles/rnemd.txt).  At 20 K the same cell holds for 1,500 steps.  The runs here stay inside the window the integrator itself keeps."""
import numpy as np
import pytest

from helpers import CASE_MODEL, GOLDEN, record_line

pytestmark = pytest.mark.gpu
DEV = "cuda"
RECORD = "rnemd.txt"
FCC_BASE = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])
A0, REPS, N_ATOMS, N_SLABS = 3.61, (2, 2, 8), 128, 8
EQUILIBRATION, STEPS, DISCARD, BLOCKS = 200, 700, 200, 5
KB, KAPPA, CU = 8.617333262e-5, 9.648533215665e-3, 63.546


def _model():
    from oracle import m3gnet_oracle as orc
    from torch_m3gnet.model.build import build_model

    params, cfg, elemental = orc.load_model_npz(GOLDEN / f"{CASE_MODEL['cu32fit']}.npz")
    model = build_model(4.76, 4.38, cfg.l_max, cfg.n_max, cfg.num_types, cfg.embedding_dim, cfg.num_blocks, elemental_energies=elemental,
                        energy_scale=cfg.energy_scale, length_scale=cfg.length_scale)
    model.load_state_dict({k: v for k, v in params.items()})
    return model.to(DEV)


def _cell():
    grid = np.stack(np.meshgrid(*[np.arange(n) for n in REPS], indexing="ij"), -1).reshape(-1, 1, 3)
    pos = (grid + FCC_BASE[None]).reshape(-1, 3) * A0
    pos = pos + np.random.default_rng(9).normal(0, 0.01, pos.shape) + [0.0, 0.0, 0.25 * A0]
    return pos, np.diag(REPS) * A0


def _run(model, kind, swap_interval, steps=STEPS, equilibration=EQUILIBRATION, discard=DISCARD, **kw):
    from torch_m3gnet.transport import ReverseNEMD

    pos, lat = _cell()
    md = ReverseNEMD(model, kind=kind, temperature=50.0, timestep=1.0, axis=2, n_slabs=N_SLABS, n_swaps=1, swap_interval=swap_interval,
                     sample_interval=10, skin=0.3, seed=3, **kw)
    (res,) = md.run([lat], [pos], [np.full(N_ATOMS, 29)], steps, equilibration=equilibration, discard=discard, loginterval=5, blocks=BLOCKS)
    assert not res["error"] and res["n_steps"] == steps
    return res


@pytest.fixture(scope="module")
def heat_runs():
    model = _model()
    return _run(model, "heat", 10), _run(model, "heat", 10 ** 6)


def _block_difference(res):
    """Temperature of the source slab minus that of the sink slab in every block (K)."""
    t = res["block_sums"][:, :, 4] / (3.0 * KB * KAPPA * res["block_counts"])
    return t[:, N_SLABS // 2] - t[:, 0]


def test_exchange_conserves_kinetic_energy_and_momentum(heat_runs):
    """Equal masses: the exchange is a permutation of velocity rows, so the kinetic energy and the total momentum before and after
    differ by the rounding of another summation order only: n terms, 2^-52 each relative to the sum of magnitudes (the momentum's
    sum of magnitudes is taken from the final velocities and doubled: the kinetic energy of a 50 K crystal does not change fourfold
    between two moments of the run)."""
    swapped, _ = heat_runs
    ke, mom = swapped["kinetic_energy_at_exchange"], swapped["momentum_at_exchange"]
    n_calls = (STEPS - 1) // 10
    assert ke.shape == (n_calls, 2) and mom.shape == (n_calls, 2, 3) and swapped["n_calls"] == n_calls
    ke_err = float((np.abs(ke[:, 1] - ke[:, 0]) / ke[:, 0]).max())
    scale = 2.0 * CU * np.abs(swapped["velocities"]).sum(0)
    mom_err = float((np.abs(mom[:, 1] - mom[:, 0]) / scale).max())
    record_line(RECORD, f"heat, {n_calls} exchange calls: kinetic energy before / after within {ke_err:.2e} relative, total momentum within "
                        f"{mom_err:.2e} of 2 sum |m v| (bound {N_ATOMS * 2.0 ** -52:.2e})")
    assert ke_err <= N_ATOMS * 2.0 ** -52 and mom_err <= N_ATOMS * 2.0 ** -52


def test_exchange_keeps_the_nve_energy_and_its_books(heat_runs):
    swapped, control = heat_runs
    drift = lambda r: float(np.abs((r["log"]["e_pot"] + r["log"]["ke"]) - (r["log"]["e_pot"] + r["log"]["ke"])[0]).max())
    d_swap, d_control = drift(swapped), drift(control)
    record_line(RECORD, f"heat, {STEPS} NVE steps of 1 fs after {EQUILIBRATION} Langevin steps at 50 K: total-energy excursion {d_swap:.2e} eV with an "
                        f"exchange every 10 steps, {d_control:.2e} eV without (gate: 3 x the control)")
    assert d_swap <= 3.0 * d_control, (d_swap, d_control)
    assert swapped["transferred"] > 0 and 0 < swapped["n_exchanged"] <= swapped["n_calls"] * 1
    assert control["transferred"] == 0.0 and control["n_exchanged"] == 0 and control["n_calls"] == control["n_samples"]
    assert swapped["n_samples"] == control["n_samples"] == (STEPS - 1) // 10 - (DISCARD // 10 - 1)
    assert swapped["counts"].sum() == swapped["n_samples"] * N_ATOMS and swapped["block_counts"].shape == (BLOCKS, N_SLABS)
    assert np.array_equal(swapped["block_counts"].sum(0), swapped["counts"]) and np.allclose(swapped["block_sums"].sum(0)[:, 4] /
                                                                                               (3 * KB * KAPPA * swapped["counts"]),
                                                                                               swapped["temperature_profile"], rtol=1e-12)
    record_line(RECORD, f"heat: {swapped['n_exchanged']} pairs exchanged in {swapped['n_calls']} calls, {swapped['transferred']:.4f} eV transferred after "
                        f"step {DISCARD}; counts per slab and sample {(swapped['counts'] / swapped['n_samples']).round(1).tolist()}")


def test_exchange_builds_a_temperature_difference_and_a_conductivity(heat_runs):
    swapped, control = heat_runs
    d_swap, d_control = _block_difference(swapped), _block_difference(control)
    se = float(np.sqrt(d_swap.var(ddof=1) / BLOCKS + d_control.var(ddof=1) / BLOCKS))
    excess = float(d_swap.mean() - d_control.mean())
    sides = swapped["gradient_sides"]
    kappa = swapped["thermal_conductivity"]
    record_line(RECORD, f"heat: T(source slab) - T(sink slab) = {d_swap.mean():.2f} K with exchanges, {d_control.mean():.2f} K without, over {BLOCKS} "
                        f"blocks of {(STEPS - DISCARD) // BLOCKS} steps: excess {excess:.2f} K = {excess / se:.1f} standard errors")
    record_line(RECORD, "heat: temperature profile (K) " + " ".join(f"{t:.1f}" for t in swapped["temperature_profile"]) + "; control "
                + " ".join(f"{t:.1f}" for t in control["temperature_profile"]))
    record_line(RECORD, f"heat: flux {swapped['flux']:.3e} eV/(A^2 fs), slopes {sides[0]:+.3f} / {sides[1]:+.3f} K/A, kappa {kappa:.2f} W/(m K) "
                        "(LJ-fitted fixture model, 29 A cell, far from stationary: a figure for the record, not a result)")
    assert excess > 3.0 * se, (excess, se)
    assert sides[0] * sides[1] < 0 and sides[0] > 0, sides   # up from the sink slab to the source slab, down beyond it
    assert np.isfinite(kappa) and kappa > 0
    assert swapped["flux"] == pytest.approx(swapped["transferred"] / (2 * (2 * A0) ** 2 * (STEPS - DISCARD)), rel=1e-12)
    assert np.allclose(swapped["slab_centres"], (np.arange(N_SLABS) + 0.5) * A0)


def test_momentum_exchange_shears_the_cell():
    res = _run(_model(), "momentum", 5, steps=600, equilibration=100, discard=0)
    flow = 0
    vx = res["velocity_profile"][:, flow]
    record_line(RECORD, f"momentum, 600 NVE steps, an exchange every 5: {res['n_exchanged']} pairs, {res['transferred']:.4e} amu A/fs transferred; "
                        "v_x per slab (A/fs) " + " ".join(f"{v:+.2e}" for v in vx) + f"; viscosity figure {res['viscosity']:.3e} Pa s (a solid: not a result)")
    assert res["transferred"] > 0 and 0 < res["n_exchanged"] <= res["n_calls"]
    assert vx[0] * vx[N_SLABS // 2] < 0 and vx[0] < 0, vx   # slab 0 gave its fastest +x atoms away
    ke = res["kinetic_energy_at_exchange"]
    assert float((np.abs(ke[:, 1] - ke[:, 0]) / ke[:, 0]).max()) <= N_ATOMS * 2.0 ** -52
