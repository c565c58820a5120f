"""FreeEnergy on the MI355X under the LJ-fitted model, 32-atom Cu cell at 100 K: the free energy does not depend on the Einstein
crystal it is integrated from, switching and equilibrium sampling agree, a structure is bitwise the same alone or beside another,
and the "msd" mode finds one spring constant per species.

The lattice constant.  Thermodynamic integration rests on the energy being the integral of the forces, and this model's is not where
a pair crosses the two-body cutoff of 5 A: the energy steps by 4.4 meV per pair there (the oracle, one atom of the cell moved along
[110]: -41.694874 eV at r = 5.0001 A, -41.690292 eV at 4.9999 A) and no force goes with the step -- the jump
tests/test_gpu_dynamics.py::test_nve_under_the_fitted_model_conserves_energy keeps its cutoffs away from.  A pair that is inside the
cutoff for a share p of the samples adds 4.4 meV * p to <dH/dlambda>, and p depends on lambda and on the spring constant.  At a = 3.61
A the fourth shell (a sqrt 2 = 5.105 A) lies 0.105 A outside the cutoff, 1.1 standard deviations of a pair distance in the k = 2 eV/A^2
crystal (sqrt(2 kB T / k) = 0.093 A) and 2.0 in the k = 6 one: measured there, F(k = 2) - F(k = 6) = +0.0377 eV at a combined standard
error of 0.0064 eV, and 0.029, 0.031 and 0.025 eV with switches of 1,600, 3,200 and 6,400 steps, 0.0287 eV by equilibrium sampling --
a bias of the model's energy, not of the switch (on the smooth Lennard-Jones crystal of tests/test_nhc_cpu.py the restatement gives
delta_f(2) - delta_f(6) = 0.4414 eV against (3 N - 3) / 2 kB T ln 3 = 0.4402 eV).  Hence a = 3.35 A here: the cutoff lies 0.26 A beyond
the fourth shell (4.738 A) and 0.30 A short of the fifth (5.297 A), 2.8 standard deviations and more, where p < 0.3 % and the bias is
below 1 meV.  The cell is 4 % smaller than the model's own (a0 = 3.505 A, whose fourth shell at 4.957 A sits 0.04 A inside the cutoff)."""
import functools

import numpy as np
import pytest

from test_gpu_dynamics import _fcc, _fitted_model

pytestmark = pytest.mark.gpu
Z32 = np.full(32, 29)
T, A = 100.0, 3.35


def _cell():
    return _fcc(A, 2)


@functools.lru_cache(maxsize=None)
def _switched():
    """The same cell tied by 2 and by 6 eV/A^2, four replicas each, in one batch: 300 + 800 + 300 + 800 steps of 2 fs."""
    from torch_m3gnet.free_energy import FreeEnergy

    pos, lat = _cell()
    fe = FreeEnergy(_fitted_model(), T, [np.full(32, 2.0), np.full(32, 6.0)], timestep=2.0, replicas=4, seed=1)
    return fe.switch([lat] * 2, [pos] * 2, [Z32] * 2, equilibration=300, switch_steps=800)


def test_free_energy_does_not_depend_on_the_spring_constant():
    """f_einstein(2) - f_einstein(6) = 0.454 eV must come back out of the switching work.  Measured on the MI355X
    (profiles/free_energy.txt): F = -34.6787 +- 0.0187 eV at k = 2 and -34.7125 +- 0.0220 eV at k = 6 eV/A^2, 0.0338 eV apart at a combined standard error of 0.0289 eV
    (1.2 of them; 6.4 % of the 0.454 eV), dissipation 0.22 and 0.059 eV per switch: the crystal's own constant is 29 eV/A^2 in this cell, so
    both Einstein crystals are soft ones and the k = 2 switch is far from linear response."""
    from torch_m3gnet.data.atomic_masses import masses_of
    from torch_m3gnet.free_energy import einstein_free_energy

    soft, stiff = _switched()
    assert not soft["error"] and not stiff["error"] and soft["n_steps"] == stiff["n_steps"] == 2200
    gap = abs(soft["f_einstein"] - stiff["f_einstein"])
    closed = einstein_free_energy(masses_of(Z32), 2.0, T, 8 * A ** 3)
    assert abs(gap - 0.454) < 1e-3 and abs(soft["f_einstein"] - closed["f_einstein"]) < 1e-6 and abs(soft["f_com"] - closed["f_com"]) < 1e-9
    diff, se = abs(soft["free_energy"] - stiff["free_energy"]), np.hypot(soft["free_energy_error"], stiff["free_energy_error"])
    for name, r in (("k = 2", soft), ("k = 6", stiff)):
        print(f"{name} eV/A^2: F = {r['free_energy']:.4f} +- {r['free_energy_error']:.4f} eV ({r['per_atom']:.5f} eV/atom), delta_f = "
              f"{r['delta_f'].mean():.4f} eV, dissipation {r['dissipation'].mean():.4f} eV per switch")
    print(f"the two differ by {diff:.4f} eV, combined standard error {se:.4f} eV = {100 * se / gap:.1f} % of the {gap:.3f} eV between the Einstein crystals")
    assert se <= 0.10 * gap, (se, gap)
    assert diff <= 3.0 * se, (diff, se)
    assert soft["delta_f"].shape == (4,) and np.array_equal(soft["spring_constants"], np.full(32, 2.0))
    log = soft["log"]
    assert log["lambda"].shape[0] == 4 and set(log["stage"][0]) == {0, 1, 2, 3} and log["lambda"].min() == 0.0 and log["lambda"].max() == 1.0


def test_switching_and_equilibrium_sampling_agree():
    """delta_f = F_model - F_Einstein(centre of mass held) by both routes, at k = 6 eV/A^2: the nearer of the two to the crystal's own
    29 eV/A^2, so the switch dissipates less there (0.059 against 0.22 eV per switch) and the bias that is left of it in (W01 - W10) / 2
    beyond linear response is the smaller.  Measured on the MI355X (profiles/free_energy.txt): -35.2785 +- 0.0220 eV by switching, -35.2986 +- 0.0054 eV by the 8 nodes (0.9 combined
    standard errors apart)."""
    from torch_m3gnet.free_energy import FreeEnergy

    pos, lat = _cell()
    stiff = _switched()[1]
    fe = FreeEnergy(_fitted_model(), T, 6.0, timestep=2.0, seed=2)
    (res,) = fe.integrate([lat], [pos], [Z32], equilibration=300, steps=1500, n_lambda=8, loginterval=5)
    assert not res["error"] and res["n_steps"] == 1800 and res["mean"].shape == (8,) and (res["variance"] > 0).all()
    assert abs(res["weights"].sum() - 1.0) < 1e-14 and np.all(np.diff(res["lambdas"]) > 0)
    a, a_se = stiff["delta_f"].mean(), stiff["free_energy_error"]
    b, b_se = res["delta_f"], res["delta_f_error"]
    print(f"delta_f by switching {a:.4f} +- {a_se:.4f} eV, by 8 Gauss-Legendre nodes {b:.4f} +- {b_se:.4f} eV; <dH/dlambda> per node "
          f"{np.round(res['mean'], 4).tolist()} +- {np.round(res['standard_error'], 4).tolist()}")
    assert np.isfinite(b_se) and b_se > 0
    assert abs(a - b) <= 3.0 * np.hypot(a_se, b_se), (a, b, a_se, b_se)


def test_a_structure_is_bitwise_the_same_alone_and_beside_another():
    from torch_m3gnet.free_energy import FreeEnergy

    model, (pos, lat) = _fitted_model(), _cell()
    kw = dict(timestep=2.0, replicas=2, structure_batches=True)
    run = dict(equilibration=10, switch_steps=20, loginterval=5)
    (alone,) = FreeEnergy(model, T, 3.0, seed=[5], **kw).switch([lat], [pos], [Z32], **run)
    both = FreeEnergy(model, T, [np.full(32, 3.0), np.full(32, 4.0)], seed=[5, 6], **kw).switch([lat, lat * 1.01], [pos, pos * 1.01], [Z32] * 2, **run)
    for key in ("delta_f", "dissipation", "work_forward", "work_backward"):
        assert np.array_equal(alone[key], both[0][key]), key
    for key, val in alone["log"].items():
        assert np.array_equal(val, both[0]["log"][key]), key
    assert alone["free_energy"] == both[0]["free_energy"] and not alone["error"] and alone["n_steps"] == both[1]["n_steps"] == 60
    assert not np.array_equal(both[0]["delta_f"], both[1]["delta_f"]) and alone["delta_f"][0] != alone["delta_f"][1]


def test_msd_mode_finds_one_spring_constant_per_species():
    from torch_m3gnet.free_energy import FreeEnergy

    pos, lat = _cell()
    fe = FreeEnergy(_fitted_model(), T, "msd", timestep=2.0, replicas=2, seed=3, msd_steps=300)
    (res,) = fe.switch([lat], [pos], [Z32], equilibration=10, switch_steps=20)
    k = res["spring_constants"]
    print(f"msd mode at {T} K: k(Cu) = {k[0]:.3f} eV/A^2 from 300 steps of 2 fs, the second half sampled")
    assert k.shape == (32,) and np.isfinite(k).all() and (k > 0).all() and np.unique(k).size == 1
    assert not res["error"] and np.isfinite(res["free_energy"])
