"""PathIntegralMD on the MI355X under the LJ-fitted model, 32-atom Cu cell: one bead without thermostat against classical NVE, the
quantum kinetic energy of an 8-bead ring at 50 K by both estimators, and a ring bitwise the same alone or beside another."""
import functools

import numpy as np
import pytest

from test_gpu_dynamics import _fcc, _fitted_model

pytestmark = pytest.mark.gpu
Z32 = np.full(32, 29)
KB = 8.617333262e-5


def _cell(seed=4, sigma=0.02):
    pos, lat = _fcc(3.61, 2)
    return pos + np.random.default_rng(seed).normal(0, sigma, pos.shape), lat


def test_one_bead_without_thermostat_is_molecular_dynamics_nve():
    """The same fp32 forces; the integrators differ in fp64 rounding only (x += h v twice against x += dt v).  A flipped fp32
    force rounding would move an atom by about dt^2 a 1e-7, below 1e-10 A: the gate of 1e-6 A has room for it.  Measured on the MI355X:
    the positions after 50 steps of 2 fs differ by 8.9e-15 A, the velocities not at all."""
    from torch_m3gnet.data.atomic_masses import masses_of
    from torch_m3gnet.dynamics import MolecularDynamics, maxwell_boltzmann, structure_seeds
    from torch_m3gnet.path_integral import PathIntegralMD

    model, (pos, lat) = _fitted_model(), _cell()
    ring = PathIntegralMD(model, n_beads=1, temperature=300.0, timestep=2.0, thermostat="none", seed=11)
    (res,) = ring.run([lat], [pos], [Z32], 50, loginterval=1)
    # the velocities the ring drew: bead 0's seed derives from the ring's, which derives from `seed`
    key = structure_seeds(int(structure_seeds(11, 1)[0]), 2)[0]
    vel = maxwell_boltzmann(masses_of(Z32), 300.0, int(key))
    md = MolecularDynamics(model, ensemble="nve", timestep=2.0, fix_com=False)
    (ref,) = md.run([lat], [pos], [Z32], 50, velocities=[vel], loginterval=1)
    assert not res["error"] and not ref["error"] and res["n_steps"] == ref["n_steps"] == 50
    assert res["positions"].shape == (1, 32, 3) and np.abs(ref["positions"] - pos).max() > 0.05
    diff = np.abs(res["positions"][0] - ref["positions"]).max()
    print(f"P = 1 without thermostat against NVE after 50 steps of 2 fs: positions differ by {diff:.1e} A, velocities by "
          f"{np.abs(res['velocities'][0] - ref['velocities']).max():.1e} A/fs")
    assert diff < 1e-6
    log = res["log"]
    assert np.allclose(log["ring_kinetic"], ref["log"]["ke"], rtol=1e-9, atol=0) and np.allclose(log["potential"], ref["log"]["e_pot"], rtol=0, atol=1e-9)
    assert not log["spring_energy"].any() and np.array_equal(log["time"], 2.0 * np.arange(51))
    assert np.allclose(log["conserved"], ref["log"]["e_pot"] + ref["log"]["ke"], rtol=0, atol=1e-8)   # no springs, no heat: NVE's total


def _blocked(x, blocks=20):
    b = x[:len(x) // blocks * blocks].reshape(blocks, -1).mean(1)
    return x.mean(), b.std(ddof=1) / np.sqrt(blocks)


@functools.lru_cache(maxsize=None)
def _quantum_run():
    from torch_m3gnet.path_integral import PathIntegralMD

    pos, lat = _cell(sigma=0.0)
    md = PathIntegralMD(_fitted_model(), n_beads=8, temperature=50.0, timestep=2.0, seed=3)
    (res,) = md.run([lat], [pos], [Z32], 3000, loginterval=1)
    return res


def test_eight_beads_at_50_k_hold_more_than_the_classical_kinetic_energy():
    """3,000 steps of 2 fs, the second half in 20 blocks.  Measured on the MI355X (profiles/path_integral.txt): K_cv = 0.5545 +- 0.0026
    eV and K_prim = 0.5586 +- 0.0062 eV against 3 n kT / 2 = 0.2068 eV, a ratio of 2.68; the ring's T 49.7 K; conserved within 3.8e-7
    eV per atom-step (0.29 eV of a ring kinetic energy of 13 eV: the integrator's O(dt^2) at w_max dt = 0.21)."""
    res = _quantum_run()
    assert not res["error"] and res["n_steps"] == 3000
    log, classical = res["log"], 1.5 * 32 * KB * 50.0
    cv, cv_se = _blocked(log["kinetic_centroid_virial"][1500:])
    prim, prim_se = _blocked(log["kinetic_primitive"][1500:])
    drift = np.abs(log["conserved"] - log["conserved"][0]).max() / (32 * 8 * 3000)
    print(f"P = 8 at 50 K: K_cv = {cv:.4f} +- {cv_se:.4f} eV, K_prim = {prim:.4f} +- {prim_se:.4f} eV against 3 n kT / 2 = {classical:.4f} eV "
          f"(ratio {cv / classical:.2f}); T of the ring {log['temperature'][1500:].mean():.1f} K; conserved within {drift:.2e} eV per atom-step")
    assert cv - classical > 5.0 * cv_se, (cv, classical, cv_se)
    assert abs(prim - cv) < 5.0 * np.hypot(prim_se, cv_se), (prim, cv, prim_se, cv_se)
    assert res["positions"].shape == res["velocities"].shape == (8, 32, 3) and np.allclose(res["centroid"], res["positions"].mean(0))


def test_a_ring_is_bitwise_the_same_alone_and_beside_another():
    from torch_m3gnet.path_integral import PathIntegralMD

    model, (pos, lat) = _fitted_model(), _cell()
    other = _cell(seed=8)[0]
    kw = dict(n_beads=3, timestep=1.0, ring_batches=True)
    (alone,) = PathIntegralMD(model, temperature=80.0, seed=[5], **kw).run([lat], [pos], [Z32], 25, loginterval=5)
    both = PathIntegralMD(model, temperature=[80.0, 200.0], seed=[5, 6], **kw).run([lat] * 2, [pos, other], [Z32] * 2, 25, loginterval=5)
    for key in ("positions", "velocities", "centroid"):
        assert np.array_equal(alone[key], both[0][key]), key
    for key, val in alone["log"].items():
        assert np.array_equal(val, both[0]["log"][key]), key
    assert not alone["error"] and alone["n_steps"] == both[1]["n_steps"] == 25 and len(alone["log"]["time"]) == 6
    assert not np.array_equal(both[0]["positions"], both[1]["positions"])
    # and a run continues from its beads
    (more,) = PathIntegralMD(model, temperature=80.0, seed=[5], **kw).run([lat], [alone["positions"]], [Z32], 2)
    assert not more["error"] and np.abs(more["positions"] - alone["positions"]).max() < 0.1
