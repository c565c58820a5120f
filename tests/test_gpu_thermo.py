"""Thermo observables on the MI355X (torch_m3gnet.thermo, C ABI m3g_thermo_*) against the numpy restatement
(tests/thermo_reference.py) over the batch of tests/thermo_cases.py: every row, tensor, mean, co-moment and lag sum within MARGIN = 8
times the reference's own fp64 rounding (measured against its long-double evaluation, per quantity), counts and flags exactly; mode
(b) fed the reference's kinetic energy and tensor against the same reference; bitwise reproducibility and independence of the batch
and of its order; graph capture; the refusal of a frame before any sample; and MolecularDynamics runs under nve, nvt_langevin,
npt_mtk and npt_mtk_cell held to the run's own log.

The measured deviations are in the docstring of test_outputs_match_the_reference and in profiles/thermo.txt."""
import functools

import numpy as np
import pytest
import torch

import thermo_cases as tc
import thermo_reference as ref
from helpers import record_line

pytestmark = pytest.mark.gpu
DEV = "cuda"
RECORD = "thermo.txt"
ACC_KEYS = ("mean", "comoments", "lag_uu", "lag_now", "lag_old", "lag_count", "n_samples", "n_skipped", "flags")
ALL = list(range(len(tc.SIZES)))
OBS_COLUMNS = 12   # the row of the stand-in for an integrator's obs in mode (b): ke in column 0, the tensor in columns 6 .. 11


def _state(order, n_lags=tc.N_LAGS, remove_com=False):
    """A fresh ThermoState of the structures `order` of the batch."""
    from torch_m3gnet.thermo import ThermoState

    b = tc.batch()
    off = b["offsets"]
    offsets = np.concatenate([[0], np.cumsum([tc.SIZES[s] for s in order])])
    return ThermoState(int(offsets[-1]), offsets, np.concatenate([b["masses"][off[s]:off[s + 1]] for s in order]),
                       [tc.P_EXT[s] for s in order], b["cells"][list(order)], n_lags, remove_com, device=DEV)


def _accumulate(n_lags=tc.N_LAGS, remove_com=False, order=None, graph=False, kick_all=False, mode="a", take=None):
    """Feed the eleven frames to a fresh ThermoState of the batch, or of the structures `order` in that order, reading the row and the
    newest ring entry after every sample.  graph: through one captured thermo_sample (every frame kicked: the kick is an argument of
    the call); mode "a": velocities, "b" / "b0": the kinetic energy and (b) the tensor of the long-double reference out of a
    12-column stand-in for an integrator's obs; take: f(tensor) -> the device tensor to use (guarded copies).  Returns {structure:
    its accumulators, `rows` [frames, 11] and `tensors` [frames, 7]}."""
    from torch_m3gnet.thermo import thermo_sample

    b = tc.batch()
    off = b["offsets"]
    order = ALL if order is None else list(order)
    atoms = np.concatenate([np.arange(off[s], off[s + 1]) for s in order])
    st = _state(order, n_lags, remove_com)
    take = (lambda x: x) if take is None else take
    dev = lambda x: take(torch.tensor(np.ascontiguousarray(x), device=DEV))
    src = tc.reference("longdouble", False, n_lags, remove_com, kick_all) if mode != "a" else None
    data = []
    for k, fr in enumerate(b["frames"]):
        d = dict(energies=dev(fr["energies"][order]), stresses=dev(fr["stresses"][order]), lattice=dev(fr["lattice"][order]))
        if mode == "a":
            d.update(vel=dev(fr["vel"][atoms]), forces=dev(fr["forces"][atoms]) if tc.kicked(k, kick_all) else None)
        else:
            obs = np.full((len(order), OBS_COLUMNS), np.nan)
            for at, s in enumerate(order):
                obs[at, 0], obs[at, 6:] = tc.fed(src[s], k)
            d.update(obs=dev(obs))
        data.append(d)
    rows, tensors = [], []

    def sample(d):
        if mode == "a":
            thermo_sample(st, d["energies"], d["stresses"], d["lattice"], d["vel"], d["forces"], tc.KICK)
        else:
            thermo_sample(st, d["energies"], d["stresses"], d["lattice"], kinetic=d["obs"][:, 0],
                          pressure_tensor=d["obs"][:, 6:] if mode == "b" else None)

    def keep():
        row, tensor = st.frame()
        rows.append(row), tensors.append(tensor)

    if graph:
        static = {key: torch.empty_like(val) for key, val in data[0].items()}
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):   # one stream, no parallel branches; nothing executes here
            sample(static)
        for d in data:
            for key, val in d.items():
                static[key].copy_(val)
            g.replay()
            keep()
    else:
        for d in data:
            sample(d)
            keep()
    torch.cuda.synchronize()
    out = st.read()
    per = {}
    for at, s in enumerate(order):
        per[s] = {key: out[key][at] for key in ACC_KEYS}
        per[s]["rows"] = np.stack([r[at] for r in rows])
        per[s]["tensors"] = np.stack([t[at] for t in tensors]) if n_lags else None
    per["state_bytes"] = st.state.numel()
    return per


@functools.lru_cache(maxsize=None)
def _full(n_lags=tc.N_LAGS, remove_com=False):
    """The eleven frames through the whole batch, kept: the bitwise tests compare against it."""
    return _accumulate(n_lags, remove_com)


def _same(a, b, keys=ACC_KEYS + ("rows", "tensors")):
    for key in keys:
        if a[key] is None or b[key] is None:
            assert a[key] is None and b[key] is None, key
            continue
        assert np.array_equal(a[key], b[key], equal_nan=True) and np.asarray(a[key]).dtype == np.asarray(b[key]).dtype, key


def _ratios(got, n_lags, remove_com, names=tc.QUANTITIES, **key):
    """{quantity: deviation / unit} of a device run against the long-double reference; counts and flags are compared exactly."""
    hi = tc.reference("longdouble", n_lags=n_lags, remove_com=remove_com, **key)
    worst = {}
    for s, acc in enumerate(hi):
        g = got[s]
        assert (g["n_samples"], g["n_skipped"], g["flags"]) == (acc.n_samples, acc.n_skipped, acc.flags), s
        assert np.array_equal(g["lag_count"], acc.lag_count), s
    for name in names:
        if name in ("tensors", "lag_uu", "lag_now", "lag_old") and n_lags == 0:
            continue
        have = {}
        for s, acc in enumerate(hi):
            kept = [k for k, bad in enumerate(acc.skipped) if not bad]
            have[s] = got[s][name][kept] if name in ("rows", "tensors") else got[s][name]
        dev, one = tc.deviation(None, name, got=have, n_lags=n_lags, remove_com=remove_com, **key), tc.unit(name, n_lags=n_lags, remove_com=remove_com, **key)
        print(f"n_lags {n_lags} remove_com {int(remove_com)} {name}: deviation {dev:.3e}, unit {one:.3e}")
        assert one > 0 or dev == 0, (name, dev)
        worst[name] = dev / one if one > 0 else 0.0
    return worst


def test_outputs_match_the_reference():
    """Rows and tensors of every frame (m3g_thermo_frame), means, co-moments and lag sums against the long-double reference: the gate
    is MARGIN = 8 units of the fp64 reference's own deviation from it (tests/thermo_cases.py: chosen on the CPU, where another fp64
    evaluation of the reference stays within 1.6 units); counts and flags exactly.  Measured on the MI355X, deviation / unit
    (n_lags 4, remove_com off / on):
      rows 0.746 / 0.746, tensors 1.009 / 1.000, mean 1.000 / 1.000, comoments 1.000 / 1.000, lag_uu 0.811 / 1.620,
      lag_now 0.714 / 0.923, lag_old 1.431 / 0.915
    (the units: rows 5.9e-16, tensors 1.7e-16, mean 2.9e-16, comoments 1.8e-16, lag_uu 9.2e-17, lag_now 1.5e-16, lag_old 8.8e-17 of
    the sum of the absolute values of an entry's terms); n_lags 1 and 0 and both forms of mode (b) are in profiles/thermo.txt."""
    assert tc.long_double_is_wider(), "np.longdouble is no wider than fp64 on this host: the tolerance would measure nothing"
    for n_lags, remove_com in ((tc.N_LAGS, False), (tc.N_LAGS, True), (1, False), (0, False)):
        got = _full(n_lags, remove_com)
        worst = _ratios(got, n_lags, remove_com)
        record_line(RECORD, f"n_lags {n_lags}, remove_com {int(remove_com)}: deviation / unit (gate {tc.MARGIN:g}): "
                            + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
        for key, ratio in worst.items():
            assert ratio <= tc.MARGIN, (n_lags, remove_com, key, ratio)
    got = _full()
    record_line(RECORD, f"state of the test batch ({sum(tc.SIZES)} atoms, {len(tc.SIZES)} structures, n_lags {tc.N_LAGS}): {got['state_bytes']} B")
    # the NaN energy: the row shows it, the ring is empty after it and holds one entry after the next sample
    s, k = tc.NAN_AT
    assert np.isnan(got[s]["rows"][k][0]) and np.isnan(got[s]["rows"][k][3]) and np.isfinite(got[s]["rows"][k][[1, 2, 4]]).all()
    assert np.isnan(got[s]["tensors"][k]).all() and np.isfinite(got[s]["tensors"][k + 1]).all()
    assert all(np.isfinite(got[o]["rows"]).all() and np.isfinite(got[o]["tensors"]).all() for o in ALL if o != s)
    # the means do not depend on the ring
    for other in (1, 0):
        for o in ALL:
            _same(got[o], _full(other)[o], keys=("mean", "comoments", "rows", "n_samples", "n_skipped", "flags"))
    assert _full(0)[0]["lag_uu"].size == 0 and _full(0)[0]["tensors"] is None


def test_mode_b_fed_the_reference_gives_the_accumulators_of_mode_a():
    """ke and the tensor of the long-double mode-(a) reference, rounded to fp64 and read out of a 12-column row (the strides of an
    integrator's obs), against that same reference, in its units; without the tensor (n_lags = 0) the means and co-moments."""
    worst = _ratios(_accumulate(mode="b"), tc.N_LAGS, False)
    record_line(RECORD, f"mode (b), n_lags {tc.N_LAGS}: deviation / unit (gate {tc.MARGIN:g}): " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert all(ratio <= tc.MARGIN for ratio in worst.values()), worst
    # ke alone: p is the integrators' scalar pressure, so only what does not hold p is the mode-(a) number
    got = _accumulate(n_lags=0, mode="b0")
    hi = tc.reference("longdouble", n_lags=0)
    cols = [0, 1, 2, 5, 6, 7, 8, 9, 10]
    for s, acc in enumerate(hi):
        kept = [k for k, bad in enumerate(acc.skipped) if not bad]
        want, scale = tc.quantity(acc, "rows")
        assert tc.scaled((got[s]["rows"][kept] - want)[:, cols], scale[:, cols]) <= tc.MARGIN * tc.unit("rows", n_lags=0), s
    worst = _ratios(got, 0, False, names=("rows", "mean", "comoments"), mode="b0")
    record_line(RECORD, f"mode (b) without a tensor: deviation / unit (gate {tc.MARGIN:g}): " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert all(ratio <= tc.MARGIN for ratio in worst.values()), worst


def test_bitwise_reproducible_alone_and_in_any_order():
    for remove_com in (False, True):
        first, second = _full(tc.N_LAGS, remove_com), _accumulate(remove_com=remove_com)
        permuted = _accumulate(remove_com=remove_com, order=[3, 1, 0, 2])
        for s in ALL:
            _same(first[s], second[s])
            _same(first[s], _accumulate(remove_com=remove_com, order=[s])[s])
            _same(first[s], permuted[s])


def test_captured_sample_replays_bitwise():
    """One thermo_sample captured on static buffers, the eleven frames copied in and replayed: ring positions and counts are
    device-resident, so the replays equal eleven eager samples (the ring wraps more than twice in both); in both modes."""
    eager, graphed = _accumulate(kick_all=True), _accumulate(kick_all=True, graph=True)
    for s in ALL:
        _same(eager[s], graphed[s])
    assert eager[3]["n_samples"] == tc.N_FRAMES and eager[3]["lag_count"].tolist() == [11, 10, 9, 8]
    eager, graphed = _accumulate(mode="b"), _accumulate(mode="b", graph=True)
    for s in ALL:
        _same(eager[s], graphed[s])


def test_frame_before_any_sample_is_refused():
    st = _state([0, 1])
    with pytest.raises(ValueError, match="m3g_thermo_frame: no sample has been taken"):
        st.frame()
    acc = st.read()
    assert all((acc[key] == 0).all() for key in ACC_KEYS)


# ---- MolecularDynamics ---------------------------------------------------------------------------------------------------------------
STEPS = 20


def _md_inputs():
    from test_gpu_dynamics import _fcc

    pos0, lat = _fcc(3.5, 2)
    pos = pos0 + np.random.default_rng(4).normal(0, 0.02, pos0.shape)
    return lat, pos, np.full(32, 29), [np.full(32, 63.546)]


def _run(ensemble, observables, monkeypatch=None, **kw):
    """(result, the raw obs rows the log saw [steps + 1, columns]) of a 20-step run of the 32-atom Cu cell, logged at every step."""
    from test_gpu_dynamics import _fitted_model
    from torch_m3gnet import _driver
    from torch_m3gnet.dynamics import MolecularDynamics

    seen = []
    if monkeypatch is not None:
        real = _driver.MdLog.append

        def append(self, k, energies, obs, lattice=None):
            seen.append(obs.cpu().numpy()[0].copy())
            real(self, k, energies, obs, lattice)

        monkeypatch.setattr(_driver.MdLog, "append", append)
    lat, pos, z, m = _md_inputs()
    md = MolecularDynamics(_fitted_model(), ensemble=ensemble, timestep=1.0, temperature=300.0, seed=3, **kw)
    (res,) = md.run([lat], [pos], [z], STEPS, masses=m, loginterval=1, observables=observables)
    return res, np.array(seen)


@pytest.mark.parametrize("ensemble", ["nve", "nvt_langevin"])
def test_md_means_equal_the_logs_means(ensemble):
    """The sampler's <ke>, <p> and <V> against the means of the log of the same run: the same terms (v + dt/2 a of every atom), summed
    in another order -- 1e-10 relative.  Positions bitwise the same with and without the observable."""
    from torch_m3gnet.thermo import ThermoObservables

    plain, _ = _run(ensemble, None)
    res, _ = _run(ensemble, ThermoObservables(n_lags=4))
    assert "thermo" not in plain and np.array_equal(plain["positions"], res["positions"]) and np.array_equal(plain["velocities"], res["velocities"])
    th, log = res["thermo"], res["log"]
    assert th["n_samples"] == STEPS + 1 == len(log["ke"]) and th["n_skipped"] == 0 and not th["flags"]["nonfinite"]
    for key in ("ke", "p", "v", "e_pot"):
        want = log[key].mean()
        print(f"{ensemble} {key}: sampler {th[key]!r}, log {want!r}")
        assert abs(th[key] - want) <= 1e-10 * abs(want), key
    dof = 32.0 / 31.0 if ensemble == "nve" else 1.0   # the log's t is 2 ke / (3 n kB); nve runs with fix_com: g = 3 n - 3
    assert np.isclose(th["t"], log["t"].mean() * dof, rtol=1e-10) and th["heat_capacity"] is not None and th["bulk_modulus"] is None
    assert th["lag_count"].tolist() == [21, 20, 19, 18] and np.isfinite(th["eta_shear"]).all() and np.isfinite(th["viscosity_bulk"])
    assert np.abs(th["strain"]).max() < 1e-15   # the cell does not move (L0^-1 L0 is the unit matrix up to rounding)


@pytest.mark.parametrize("ensemble", ["npt_mtk", "npt_mtk_cell"])
def test_md_means_are_the_welford_means_of_the_integrators_obs(ensemble, monkeypatch):
    """ke, p and V (and, npt_mtk_cell, the tensor) are the integrator's own obs values, so the device's means are exactly those of the
    header's recursion run on the host over the rows the log saw."""
    from torch_m3gnet.thermo import ThermoObservables

    cell = ensemble == "npt_mtk_cell"
    plain, _ = _run(ensemble, None, pressure=0.0)
    res, obs = _run(ensemble, ThermoObservables(n_lags=3 if cell else 0), monkeypatch, pressure=0.0)
    assert np.array_equal(plain["positions"], res["positions"]) and np.array_equal(plain["lattice"], res["lattice"])
    th = res["thermo"]
    assert th["n_samples"] == STEPS + 1 == len(obs) and th["n_skipped"] == 0
    rows = np.zeros((len(obs), ref.ROW))
    rows[:, 1], rows[:, 2], rows[:, 4] = obs[:, 0], obs[:, 3], obs[:, 2]
    mean = ref.welford(rows)[0]
    for at, key in ((1, "ke"), (2, "v"), (4, "p")):
        print(f"{ensemble} {key}: sampler {th['mean'][at]!r}, host recursion {mean[at]!r}")
    assert th["mean"][1] == mean[1] and th["mean"][2] == mean[2] and th["mean"][4] == mean[4]
    assert th["ke"] == mean[1] and th["v"] == mean[2] and np.isclose(th["p"], res["log"]["p"].mean(), rtol=1e-12)
    assert np.isfinite(th["heat_capacity"]) and np.isfinite(th["bulk_modulus"]) and np.isfinite(th["thermal_expansion"])
    assert np.abs(th["strain"]).max() > 0
    if cell:
        total = np.zeros(7)
        for row in obs:   # the sums of the ring's newest entries, in sample order
            total = total + np.concatenate([row[6:12], [row[2]]])
        assert np.array_equal(th["tensor_mean"], total / len(obs)) and th["lag_count"].tolist() == [21, 20, 19]
        assert th["elastic_constants"].shape == (6, 6)
        # the order of the components, by name: against the log's pressure_tensor, and the log's last entry against the tensor formed
        # here from the final (synchronous) velocities, stresses and cell
        from torch_m3gnet._driver import EV_A3_TO_GPA

        names = ("xx", "yy", "zz", "yz", "zx", "xy")
        logged = dict(zip(names, res["log"]["pressure_tensor"].T))
        axes = dict(x=0, y=1, z=2)
        v, m = res["velocities"], _md_inputs()[3][0]
        vol = abs(np.linalg.det(res["lattice"]))
        for at, name in enumerate(names):
            a, b = axes[name[0]], axes[name[1]]
            assert np.isclose(th["tensor_mean"][at] * EV_A3_TO_GPA, logged[name].mean(), rtol=1e-12, atol=0), name
            own = res["stresses"][at] + (m * v[:, a] * v[:, b]).sum() / ref.KAPPA / vol
            print(f"P_{name} of the last step: log {logged[name][-1] / EV_A3_TO_GPA!r}, from the final state {own!r}")
            assert abs(own - logged[name][-1] / EV_A3_TO_GPA) < 1e-8, name
        assert len({round(abs(float(x)), 12) for x in th["tensor_mean"][:6]}) == 6   # (six different numbers: an exchange would show)
    else:
        assert th["elastic_constants"] is None
    # every second step: the cell copied before the integrator call and the sample taken after it belong to the same k
    half, obs2 = _run(ensemble, ThermoObservables(sample_interval=2), monkeypatch, pressure=0.0)
    rows = np.zeros((len(obs2[::2]), ref.ROW))
    rows[:, 1], rows[:, 2], rows[:, 4] = obs2[::2, 0], obs2[::2, 3], obs2[::2, 2]
    mean = ref.welford(rows)[0]
    th2 = half["thermo"]
    assert th2["n_samples"] == STEPS // 2 + 1 == len(rows) and np.array_equal(half["positions"], plain["positions"])
    assert th2["mean"][1] == mean[1] and th2["mean"][2] == mean[2] and th2["mean"][4] == mean[4]


def test_md_refuses_lags_with_npt_mtk_and_runs_beside_the_other_kinds():
    from test_gpu_dynamics import _fitted_model
    from torch_m3gnet.dynamics import MolecularDynamics
    from torch_m3gnet.local_order import LocalOrderObservables
    from torch_m3gnet.scattering import ScatteringObservables
    from torch_m3gnet.thermo import ThermoObservables
    from torch_m3gnet.trajectory import TrajectoryObservables

    lat, pos, z, m = _md_inputs()
    npt = MolecularDynamics(_fitted_model(), ensemble="npt_mtk", timestep=1.0, temperature=300.0, pressure=0.0, seed=3)
    with pytest.raises(ValueError, match="not supported with npt_mtk: its integrator states no pressure tensor"):
        npt.run([lat], [pos], [z], 2, masses=m, observables=ThermoObservables(n_lags=2))
    others = [TrajectoryObservables(rdf_bins=50, n_lags=8, sample_interval=2), ScatteringObservables(q_max=3.0, n_lags=8, sample_interval=2),
              LocalOrderObservables({29: 3.0}, sample_interval=4, max_samples=4)]
    alone, _ = _run("nvt_nose_hoover", ThermoObservables(n_lags=4, sample_interval=2))
    md = MolecularDynamics(_fitted_model(), ensemble="nvt_nose_hoover", timestep=1.0, temperature=300.0, seed=3)
    (three,) = md.run([lat], [pos], [z], STEPS, masses=m, loginterval=1, observables=others)
    (four,) = md.run([lat], [pos], [z], STEPS, masses=m, loginterval=1, observables=others[:2] + [ThermoObservables(n_lags=4, sample_interval=2)] + others[2:])
    assert np.array_equal(three["positions"], four["positions"]) and np.array_equal(three["scattering"]["s"], four["scattering"]["s"])
    assert {"observables", "scattering", "local_order", "thermo"} <= set(four) and "thermo" not in three
    a, b = alone["thermo"], four["thermo"]
    assert a["n_samples"] == b["n_samples"] == 11 and np.array_equal(a["mean"], b["mean"]) and np.array_equal(a["covariance"], b["covariance"])
    assert np.array_equal(a["shear_acf"], b["shear_acf"]) and np.array_equal(a["time"], np.arange(4) * 2.0) and np.isfinite(a["heat_capacity"])
