"""Metadynamics and UmbrellaSampling on the MI355X under the LJ-fitted model, the 32-atom Cu cell of tests/test_gpu_ti_driver.py at
a = 3.35 A (every shell well away from the model's cutoff step, see there).  The CV is the hop coordinate: the projection of atom 0
relative to the centre of the other 31 atoms along [110]."""
import numpy as np
import pytest
import torch

import meta_reference as mr
from test_gpu_dynamics import _fcc, _fitted_model

pytestmark = pytest.mark.gpu
Z32 = np.full(32, 29)
T, A = 300.0, 3.35
REST = list(range(1, 32))


def _cell():
    return _fcc(A, 2)


def _cv():
    from torch_m3gnet.metadynamics import projection

    return projection([0], REST, [1.0, 1.0, 0.0])


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def test_with_the_bias_off_metadynamics_is_molecular_dynamics_bitwise():
    """Height 0, no restraint, no walls: the hills deposited every other step weigh nothing, the biased forces are the engine's to
    the bit, and the run is `MolecularDynamics.run` (Langevin) with the walker's own keys, over 20 steps."""
    from torch_m3gnet.data.atomic_masses import masses_of
    from torch_m3gnet.dynamics import MolecularDynamics, maxwell_boltzmann
    from torch_m3gnet.metadynamics import Metadynamics, walker_keys

    pos, lat = _cell()
    model = _fitted_model()
    meta = Metadynamics(model, _cv(), T, height=0.0, sigma=[0.1], pace=2, bias_factor=8.0, timestep=2.0, seed=5)
    (res,) = meta.run([lat], [pos], [Z32], steps=20)
    v_seed, t_key = walker_keys(5, 1, 1)
    md = MolecularDynamics(model, "nvt_langevin", timestep=2.0, temperature=T, seed=[int(t_key[0, 0])])
    (want,) = md.run([lat], [pos], [Z32], steps=20, velocities=[maxwell_boltzmann(masses_of(Z32), T, int(v_seed[0, 0]))])
    (got,) = res["walkers"]
    for key in ("positions", "velocities", "forces"):
        assert np.array_equal(bits(got[key]), bits(want[key])), key
    assert got["total_energy"] == want["total_energy"] and got["n_steps"] == want["n_steps"] == 20 and not got["error"]
    assert np.array_equal(got["log"]["ke"], want["log"]["ke"])
    assert res["n_hills"] == 10 and not res["hills"].heights.any() and not res["full"] and not res["error"]
    assert res["cv"].shape == (1, 21, 1) and abs(res["cv"][0, 0, 0]) < 1e-12 and np.abs(res["cv"]).max() > 1e-3   # the CV starts at its origin and moves
    assert not res["bias_energy"].any()


def _nve(kappa: float, steps: int = 200):
    """NVE through the thin layer: E_pot + KE + V_bias every step, under a static PROJECTION restraint of `kappa` eV/A^2 centred
    0.15 A along the hop direction (kappa 0: the unbiased run through the same calls)."""
    from torch_m3gnet._driver import atom_offsets
    from torch_m3gnet.data import MaterialGraphKey as K
    from torch_m3gnet.data.atomic_masses import masses_of
    from torch_m3gnet.data.md import VerletGraph
    from torch_m3gnet.dynamics import DynState, dyn_step, maxwell_boltzmann
    from torch_m3gnet.metadynamics import BiasState, bias_forces, projection

    pos, lat = _cell()
    model = _fitted_model()
    cfg = model.engine.cfg
    vg = VerletGraph([lat], [Z32], cfg.cutoff, cfg.threebody_cutoff, skin=0.5, device="cuda")
    m = masses_of(Z32)
    pos_t = torch.tensor(pos, dtype=torch.float64, device=vg.device)
    offsets = atom_offsets([Z32])
    dyn = DynState(pos_t, vg.lattice.clone(), offsets, m, torch.tensor(maxwell_boltzmann(m, 100.0, 3), device=vg.device), 100.0,
                   np.array([1], dtype=np.uint64), ensemble="nve", dt=1.0)
    origin = pos[0] - (m[1:, None] * pos[1:]).sum(0) / m[1:].sum()
    bias = BiasState(offsets, lat[None], [projection([0], REST, [1.0, 1.0, 0.0], origin=origin)], m, [0.1], centres=[0.15], kappa=[kappa],
                     device=vg.device)
    total, cv = [], []
    for k in range(steps + 1):
        out = vg.step(model, pos_t)
        f = bias_forces(bias, pos_t, out[K.FORCES])
        dyn_step(dyn, f, out[K.STRESSES], finish_only=(k == steps))
        total.append((out[K.TOTAL_ENERGY].double() + dyn.obs[:, 0] + bias.obs[:, 2]).clone())
        cv.append(bias.obs[:, 0].clone())
    return torch.stack(total).cpu().numpy()[:, 0], torch.stack(cv).cpu().numpy()[:, 0]


def test_a_static_restraint_conserves_the_total_energy_as_well_as_no_bias_does():
    """200 steps of 1 fs from 100 K.  The restraint (kappa = 2 eV/A^2, 0.15 A off: 22 meV of bias energy at the start) is a smooth
    function of the positions whose forces are exact to fp64, so the drift of E_pot + KE + V_bias is the integrator's and the fp32
    engine's, as in the unbiased run of the same cell through the same calls.  Measured on the MI355X (profiles/metadynamics.txt):
    max |E - E0| = 5.84e-4 eV unbiased and 5.77e-4 eV under the restraint, a ratio of 0.99; the margin of 1.5 is for the different
    trajectory the restraint drives (the CV goes from 0 to 0.030 A)."""
    free, _ = _nve(0.0)
    held, cv = _nve(2.0)
    drift = lambda e: np.abs(e - e[0]).max()   # noqa: E731
    print(f"NVE 200 x 1 fs: max |E - E0| = {drift(free):.3e} eV unbiased, {drift(held):.3e} eV under the restraint; CV from {cv[0]:.4f} to "
          f"{cv.min():.4f} .. {cv.max():.4f} A")
    assert abs(cv[0]) < 1e-12 and cv.max() > 0.02          # the restraint pulls the atom towards its centre
    assert drift(held) <= 1.5 * drift(free), (drift(held), drift(free))


def test_ten_steps_with_pace_two_equal_the_restatement_fed_the_same_forces():
    """The thin layer over the engine, two walkers, well-tempered: at every step the device's CV, bias and hill list against the
    restatement given the device's own positions and engine forces of that step.  The CVs and hill centres are free of exp: bitwise.
    The heights and V_hills within the kernel-level gate: 2 x the response of the restatement to a 1-ulp nudge of every exp, plus
    (n + 8) 2^-52 sum |term| (tests/test_gpu_meta.py::hill_gates)."""
    from torch_m3gnet._driver import Driver, GroupedEvaluation
    from torch_m3gnet.data import MaterialGraphKey as K
    from torch_m3gnet.data.atomic_masses import masses_of
    from torch_m3gnet.dynamics import KB, DynState, dyn_step, maxwell_boltzmann
    from torch_m3gnet.metadynamics import BiasState, bias_forces, projection

    pos, lat = _cell()
    model = _fitted_model()
    ev = GroupedEvaluation(Driver(model).model, [lat, lat], [Z32, Z32], [(0, 2)], 0.5, "cuda")
    m = masses_of(Z32)
    m2 = np.concatenate([m, m])
    pos_t = torch.tensor(np.concatenate([pos, pos]), dtype=torch.float64, device=ev.device)
    vel = np.concatenate([maxwell_boltzmann(m, T, 1), maxwell_boltzmann(m, T, 2)])
    dyn = DynState(pos_t, ev.lattices(), ev.offsets, m2, torch.tensor(vel, device=ev.device), T, np.array([7, 8], dtype=np.uint64),
                   ensemble="nvt_langevin", dt=2.0, friction=0.01)
    origin = pos[0] - (m[1:, None] * pos[1:]).sum(0) / m[1:].sum()
    raw = np.array([1.0, 1.0, 0.0])
    inv_kdt = 1.0 / (KB * 7.0 * T)
    bias = BiasState(ev.offsets, np.stack([lat, lat]), [projection([0], REST, raw, origin=origin)], m2, [0.05], height=0.02, inv_kdt=inv_kdt,
                     max_hills=10, group_offsets=[0, 2], device=ev.device)
    membership = np.zeros(32, dtype=np.uint8)
    membership[0], membership[1:] = 1, 2
    walkers = [dict(lattice=lat, weights=m, origins=origin[None])] * 2
    refs = {sign: mr.Group([mr.Cv(mr.PROJECTION, membership, direction=raw / np.linalg.norm(raw))], walkers, [0.05], 0.02, inv_kdt, 10,
                           exp=mr.nudged_exp(sign) if sign else np.exp) for sign in (0, 1, -1)}
    for k in range(11):
        out = ev.evaluate(pos_t)
        p_host, f_host = pos_t.cpu().numpy(), out[K.FORCES].cpu().numpy()
        deposit = k > 0 and k % 2 == 0
        f = bias_forces(bias, pos_t, out[K.FORCES], deposit=deposit)
        got, got_f = bias.obs.cpu().numpy(), f.cpu().numpy()
        rows = {sign: ref.bias([p_host[:32], p_host[32:]], [f_host[:32], f_host[32:]], deposit=deposit) for sign, ref in refs.items()}
        for w in range(2):
            want, want_f, x = rows[0][w]
            gate = 2.0 * np.maximum(np.abs(rows[1][w][0] - want), np.abs(rows[-1][w][0] - want)) + 8 * 2.0 ** -52 * np.abs(want)
            gate[3] += (x["n_terms"] + 8) * 2.0 ** -52 * x["abs_sum"][0]
            gate[2] += (x["n_terms"] + 8) * 2.0 ** -52 * x["abs_sum"][0]
            gate[5] += (x["n_terms"] + 8) * 2.0 ** -52 * x["abs_sum"][1]
            assert bits(got[w, :1])[0] == bits(want[:1])[0], (k, w, got[w, 0], want[0])
            assert (np.abs(got[w] - want) <= gate).all(), (k, w, got[w], want, gate)
            g_f = gate[5] * np.abs(x["grad"][0]) + np.spacing(np.abs(want_f)).astype(np.float64)
            assert (np.abs(got_f[32 * w:32 * (w + 1)].astype(np.float64) - want_f) <= g_f).all(), (k, w)
        dyn_step(dyn, f, out[K.STRESSES], finish_only=(k == 10))
    out = bias.read()
    ref = refs[0]
    assert out["n_hills"].tolist() == [10] == [ref.n_hills] and out["flags"].tolist() == [0, 0]
    assert np.array_equal(bits(out["centres"][0]), bits(ref.centres))
    gate = 2.0 * np.maximum(np.abs(refs[1].heights - ref.heights), np.abs(refs[-1].heights - ref.heights)) + 8 * 2.0 ** -52 * ref.heights
    assert (np.abs(out["heights"][0] - ref.heights) <= gate).all() and (ref.heights[2:] < 0.02).all() and (ref.heights > 0.0).all()


def test_an_input_is_bitwise_the_same_alone_and_beside_another():
    from torch_m3gnet.metadynamics import Metadynamics

    pos, lat = _cell()
    other = pos + np.random.default_rng(4).normal(0.0, 0.03, pos.shape)
    meta = Metadynamics(_fitted_model(), _cv(), T, height=0.02, sigma=[0.05], pace=2, bias_factor=8.0, walkers=2, timestep=2.0, seed=[11, 12])
    both = meta.run([lat, lat], [pos, other], [Z32, Z32], steps=12)
    for g, (p, seed) in enumerate(((pos, 11), (other, 12))):
        alone = Metadynamics(_fitted_model(), _cv(), T, height=0.02, sigma=[0.05], pace=2, bias_factor=8.0, walkers=2, timestep=2.0, seed=[seed])
        (one,) = alone.run([lat], [p], [Z32], steps=12)
        assert np.array_equal(bits(one["cv"]), bits(both[g]["cv"])) and np.array_equal(bits(one["bias_energy"]), bits(both[g]["bias_energy"]))
        assert np.array_equal(bits(one["hills"].centres), bits(both[g]["hills"].centres)) and one["n_hills"] == both[g]["n_hills"] == 12
        assert np.array_equal(bits(one["hills"].heights), bits(both[g]["hills"].heights))
        for a, b in zip(one["walkers"], both[g]["walkers"]):
            assert np.array_equal(bits(a["positions"]), bits(b["positions"])) and np.array_equal(bits(a["velocities"]), bits(b["velocities"]))
    assert not np.array_equal(both[0]["cv"], both[1]["cv"]) and not np.array_equal(both[0]["cv"][0], both[0]["cv"][1])


def test_umbrella_windows_pull_the_cv_towards_their_centres_in_the_order_kappa_predicts():
    """Two windows centred at +0.6 A, kappa = 4 and 16 eV/A^2, against the crystal's own restoring force on the hop coordinate (of
    the order of the 29 eV/A^2 tests/test_gpu_ti_driver.py quotes): both means move towards +0.6 from the unbiased 0 -- by about
    0.6 kappa / (kappa + 29), 0.07 and 0.2 A, many times the 0.01 A the mean of 300 correlated samples of a coordinate whose thermal
    width is 0.03 A scatters by --, the stiffer window further, neither beyond its centre."""
    from torch_m3gnet.metadynamics import UmbrellaSampling

    pos, lat = _cell()
    us = UmbrellaSampling(_fitted_model(), _cv(), centres=[0.6, 0.6], kappa=[4.0, 16.0], temperature=T, timestep=2.0, friction=0.05, seed=3)
    (res,) = us.run([lat], [pos], [Z32], steps=300, equilibration=100)
    soft, stiff = res["samples"][0].mean(), res["samples"][1].mean()
    print(f"umbrella windows at +0.6 A: mean CV {soft:.4f} A at kappa = 4, {stiff:.4f} A at kappa = 16 eV/A^2")
    assert res["samples"].shape == (2, 301) and not res["error"]
    assert 0.0 < soft < stiff < 0.6, (soft, stiff)
