"""Batched replica exchange on the MI355X (torch_m3gnet.replica_exchange, C ABI m3g_remd_*): the two kernels against the restatement
(tests/remd_reference.py wrapped around tests/md_reference.py, cases of tests/remd_cases.py), bitwise independence of the batch and
reproducibility, the pairs that are not attempted, the launch count, and ReplicaExchange runs of the 32-atom Cu cell under the
LJ-fitted model."""
import ctypes as C

import numpy as np
import pytest
import torch

import md_reference as mr
import remd_cases as rc
from helpers import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda"
FCC_BASE = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])


class Batch:
    """The ladders `ids` of remd_cases.LADDERS as one DynState / RemdState."""

    def __init__(self, ids):
        from torch_m3gnet.dynamics import DynState
        from torch_m3gnet.replica_exchange import RemdState

        self.ids = list(ids)
        parts = [rc.start(g) for g in self.ids]
        lats, poss, ms, vs = ([x for p in parts for x in p[j]] for j in range(4))
        self.R = [len(rc.LADDERS[g][0]) for g in self.ids]
        self.n = [rc.LADDERS[g][1] for g in self.ids]
        self.l_off = np.concatenate([[0], np.cumsum(self.R)])
        self.offsets = np.concatenate([[0], np.cumsum([len(p) for p in poss])])
        self.a_off = self.offsets[self.l_off]   # first atom of every ladder
        temps = np.concatenate([rc.LADDERS[g][0] for g in self.ids])
        seeds = np.concatenate([np.array(rc.LADDERS[g][3], dtype=np.uint64) for g in self.ids])
        self.S = len(temps)
        pos = torch.tensor(np.concatenate(poss), dtype=torch.float64, device=DEV)
        lat = torch.tensor(np.stack(lats), dtype=torch.float64, device=DEV)
        vel = torch.tensor(np.concatenate(vs), dtype=torch.float64, device=DEV)
        self.dyn = DynState(pos, lat, self.offsets, np.concatenate(ms), vel, temps, seeds, ensemble="nvt_langevin", **rc.PARAMS)
        self.remd = RemdState(self.l_off, temps, np.array([rc.LADDERS[g][2] for g in self.ids], dtype=np.uint64), device=DEV)
        self.history = torch.full((rc.ROUNDS, self.S), -1, dtype=torch.int32, device=DEV)
        self.stress = torch.zeros(self.S, 6, dtype=torch.float32, device=DEV)
        self.obs, self.v_before, self.v_after = [], [], []

    def run(self, ops, nan_force=None, nan_energy=None):
        from torch_m3gnet.dynamics import dyn_step
        from torch_m3gnet.replica_exchange import remd_exchange

        for op in ops:
            if op[0] == "step":
                f = torch.tensor(np.concatenate([rc.forces(g, op[1], nan_force) for g in self.ids]), device=DEV)
                dyn_step(self.dyn, f, self.stress, finish_only=op[2])
                self.obs.append(self.dyn.obs.clone())
            else:
                e = torch.tensor(np.concatenate([rc.energies(g, op[1], nan_energy) for g in self.ids]), device=DEV)
                self.v_before.append(self.dyn.velocities.clone())
                remd_exchange(self.remd, self.dyn, e, self.history)
                self.v_after.append(self.dyn.velocities.clone())
        torch.cuda.synchronize()
        return self

    def result(self) -> dict:
        from torch_m3gnet.replica_exchange import target_temperatures

        out = dict(self.remd.read(), **self.dyn.read())
        out.update(pos=self.dyn.pos.cpu().numpy(), t0=target_temperatures(self.dyn).cpu().numpy(), history=self.history.cpu().numpy(),
                   obs=torch.stack(self.obs).cpu().numpy(), v_before=torch.stack(self.v_before).cpu().numpy(),
                   v_after=torch.stack(self.v_after).cpu().numpy())
        return out


def _rel(a, b, floor=1e-300):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), floor))


def _compare(batch: Batch, out: dict, refs: list) -> None:
    """Every ladder of the batch against its reference run: integers and target temperatures exactly, the integrator's numbers and
    the statistics to 1e-12."""
    for j, ref in enumerate(refs):
        lad, lo, hi, n = ref["ladder"], batch.l_off[j], batch.l_off[j + 1], batch.n[j]
        R, na = hi - lo, lad.n_attempts
        assert out["n_attempts"][j] == na
        assert list(out["held"][lo:hi]) == lad.held and list(out["holder"][lo:hi] - lo) == lad.holder
        assert np.array_equal(out["history"][:na, lo:hi], np.array(lad.history[1:])) and (out["history"][na:, lo:hi] == -1).all()
        assert list(out["attempts"][lo:hi - 1]) == lad.attempts and list(out["accepts"][lo:hi - 1]) == lad.accepts
        assert out["attempts"][hi - 1] == 0 and out["accepts"][hi - 1] == 0
        assert list(out["round_trips"][lo:hi]) == lad.round_trips
        assert list(out["count"][lo:hi]) == lad.count
        assert np.array_equal(out["t0"][lo:hi], np.array([lad.T[h] for h in lad.held]))   # the thermostat targets, exactly
        assert _rel(out["mean"][lo:hi], np.array(lad.mean)) < 1e-12 and _rel(out["m2"][lo:hi], np.array(lad.m2), 1e-30) < 1e-12
        for r, dref in enumerate(ref["refs"]):
            s = lo + r
            a, b = batch.offsets[s], batch.offsets[s + 1]
            assert out["flags"][s] == dref.flags and out["n_steps"][s] == dref.n_steps, (j, r, out["flags"][s], dref.flags)
            assert _rel(out["pos"][a:b], dref.pos) < 1e-12, (j, r, _rel(out["pos"][a:b], dref.pos))
            assert _rel(out["v"][a:b], dref.v, 1e-4) < 1e-12, (j, r, _rel(out["v"][a:b], dref.v, 1e-4))
            if not dref.flags & mr.ERROR:
                for q in range(4):
                    assert _rel(out["obs"][:, s, q], ref["obs"][:, r, q]) < 1e-12, (j, r, q)
        # the rescale kernel: every replica's velocities times its scale, bitwise -- a scale of 1 leaves them untouched
        for x, scale in enumerate(ref["scales"]):
            per_atom = np.repeat(np.array(scale), n)[:, None]
            a, b = batch.a_off[j], batch.a_off[j + 1]
            assert np.array_equal(out["v_after"][x, a:b], out["v_before"][x, a:b] * per_atom), (j, x)
            same = per_atom[:, 0] == 1.0
            assert np.array_equal(out["v_after"][x, a:b][same], out["v_before"][x, a:b][same])


def _assert_margins(refs) -> None:
    """Accept / reject compares two transcendental results: every attempted pair with Delta < 0 must be decided by far more than
    their rounding in the reference, or the case proves nothing (tests/test_remd_cpu.py checks the same without a GPU)."""
    for ref in refs:
        margins = ref["ladder"].margins
        assert margins and all(abs(m) > 1e-9 for m in margins), min(abs(m) for m in margins)


@pytest.mark.parametrize("ids", [[0, 1, 2], [0], [1], [2], [2, 0]])
def test_kernels_match_the_restatement(ids):
    ops = rc.schedule()
    refs = [rc.reference(g, ops) for g in ids]
    _assert_margins(refs)
    batch = Batch(ids).run(ops)
    out = batch.result()
    _compare(batch, out, refs)
    for ref in refs:   # swaps happened, so the steps after them ran at the new temperatures
        assert sum(ref["ladder"].accepts) > 0
        assert all(dref.n_steps == 2 * rc.ROUNDS for dref in ref["refs"])
    if len(ids) == 3:
        accepts = sum(sum(ref["ladder"].accepts) for ref in refs)
        assert 0 < accepts < sum(sum(ref["ladder"].attempts) for ref in refs)   # both verdicts occur
        # the Langevin noise picked the swapped temperature up: a reference that keeps the starting temperatures ends elsewhere
        ref = refs[2]
        stale = rc.reference(2, [op for op in ops if op[0] == "step"])
        r = next(r for r in range(5) if ref["ladder"].held[r] != r)
        assert _rel(stale["refs"][r].pos, ref["refs"][r].pos) > 1e-6


def test_ladders_are_bitwise_independent_of_the_batch_and_reproducible():
    ops = rc.schedule()
    first, second = Batch([0, 1, 2]).run(ops), Batch([0, 1, 2]).run(ops)
    a, b = first.result(), second.result()
    for key in a:
        assert np.array_equal(a[key], b[key], equal_nan=True), key
    for j, g in enumerate([0, 1, 2]):
        alone = Batch([g]).run(ops)
        o = alone.result()
        lo, hi, x, y = first.l_off[j], first.l_off[j + 1], first.a_off[j], first.a_off[j + 1]
        for key in ("held", "attempts", "accepts", "count", "mean", "m2", "round_trips", "flags", "n_steps", "t0"):
            assert np.array_equal(o[key], a[key][lo:hi]), (g, key)
        assert np.array_equal(o["holder"], a["holder"][lo:hi] - lo) and o["n_attempts"][0] == a["n_attempts"][j]
        assert np.array_equal(o["history"], a["history"][:, lo:hi])
        assert np.array_equal(o["pos"], a["pos"][x:y]) and np.array_equal(o["v"], a["v"][x:y])
        assert np.array_equal(o["obs"], a["obs"][:, lo:hi], equal_nan=True)
        assert np.array_equal(o["v_after"], a["v_after"][:, x:y])


def test_a_failed_replica_is_left_out_and_the_rest_of_its_ladder_goes_on():
    """A NaN force at call 6 (round 3) on replica 1 of the five-replica ladder: M3G_DYN_ERROR.  From then on the pairs it is part of
    keep their attempt counts, its velocities stay bitwise what they were, and the other pairs of the ladder go on."""
    from torch_m3gnet import _lib

    ops = rc.schedule()
    nan_force = {(2, 6): 1 * 3 + 2}   # an atom of replica 1
    refs = [rc.reference(g, ops, nan_force=nan_force) for g in (1, 2)]
    _assert_margins(refs)
    batch = Batch([1, 2]).run(ops, nan_force=nan_force)
    out = batch.result()
    _compare(batch, out, refs)
    s = 3 + 1
    assert [bool(f & _lib.DYN_ERROR) for f in out["flags"]] == [False] * 4 + [True] + [False] * 3
    a, b = batch.offsets[s], batch.offsets[s + 1]
    assert np.array_equal(out["v"][a:b], out["v_before"][3][a:b]) and np.array_equal(out["v_after"][-1][a:b], out["v_before"][3][a:b])
    lad = refs[1]["ladder"]
    k = lad.held[1]                               # the index it is stuck at
    assert (out["history"][3:, s] == k).all()
    healthy = rc.reference(2, ops)["ladder"]
    stuck = [p for p in (k - 1, k) if 0 <= p < 4]
    for p in range(4):
        if p in stuck:
            assert lad.attempts[p] <= 2 and lad.attempts[p] < healthy.attempts[p]   # only the attempts before the failure (rounds 0 - 2)
        else:
            assert lad.attempts[p] == healthy.attempts[p] == 6
    assert out["count"][3 + k] == 3 and (np.delete(out["count"][3:], k) == rc.ROUNDS).all()


def test_a_non_finite_energy_skips_its_pairs_for_that_attempt_only():
    ops = rc.schedule()
    nan_energy = {(2, 4): 2, (1, 5): 0}
    refs = [rc.reference(g, ops, nan_energy=nan_energy) for g in (1, 2)]
    _assert_margins(refs)
    batch = Batch([1, 2]).run(ops, nan_energy=nan_energy)
    out = batch.result()
    _compare(batch, out, refs)
    assert np.isfinite(out["mean"]).all() and np.isfinite(out["m2"]).all() and np.isfinite(out["v"]).all()
    for j, (g, rnd, r) in enumerate([(1, 5, 0), (2, 4, 2)]):
        lad = refs[j]["ladder"]
        k = lad.history[rnd][r]                  # the index the replica held at that attempt
        assert lad.history[rnd + 1][r] == k      # it did not move
        assert sum(lad.count) == rc.ROUNDS * lad.R - 1 and lad.count[k] == rc.ROUNDS - 1
        for p in range(lad.R - 1):               # the pairs of that parity it was part of lost exactly that attempt
            lost = 1 if (p % 2 == rnd % 2 and p in (k - 1, k)) else 0
            assert lad.attempts[p] == rc.ROUNDS // 2 - lost, (g, p)
        assert sum(out["attempts"][batch.l_off[j]:batch.l_off[j + 1]]) == sum(lad.attempts)


def test_an_exchange_while_started_changes_only_counter_statistics_and_history():
    from torch_m3gnet import _lib
    from torch_m3gnet.dynamics import dyn_step
    from torch_m3gnet.replica_exchange import remd_exchange, target_temperatures

    ops = rc.started_schedule()
    refs = [rc.reference(g, ops) for g in (0, 1, 2)]
    _assert_margins(refs)
    batch = Batch([0, 1, 2]).run(ops)
    out = batch.result()
    _compare(batch, out, refs)
    for x in (1, 4):
        assert np.array_equal(out["v_after"][x], out["v_before"][x])
        assert np.array_equal(out["history"][x], out["history"][x - 1])
    assert list(out["n_attempts"]) == [6, 6, 6] and (out["count"] == 6).all()
    assert list(out["attempts"][[0, 2, 3, 5, 6, 7, 8]]) == [2, 2, 2, 2, 2, 2, 2]   # two attempts of every pair fell out (one of each parity)
    # one such call on its own: everything but the counter, the statistics and the history row stays bitwise
    fresh = Batch([2])
    f = torch.tensor(rc.forces(2, 0), device=DEV)
    dyn_step(fresh.dyn, f, fresh.stress)
    before = (fresh.remd.read(), fresh.dyn.read(), target_temperatures(fresh.dyn).clone(), fresh.dyn.pos.clone())
    assert all(fl & _lib.DYN_STARTED for fl in before[1]["flags"])
    remd_exchange(fresh.remd, fresh.dyn, torch.tensor(rc.energies(2, 0), device=DEV), fresh.history)
    after = (fresh.remd.read(), fresh.dyn.read())
    for key in ("held", "holder", "attempts", "accepts", "round_trips"):
        assert np.array_equal(before[0][key], after[0][key]), key
    for key in ("flags", "n_steps", "v"):
        assert np.array_equal(before[1][key], after[1][key]), key
    assert torch.equal(before[2], target_temperatures(fresh.dyn)) and torch.equal(before[3], fresh.dyn.pos)
    assert after[0]["n_attempts"][0] == 1 and (after[0]["count"] == 1).all()
    assert np.array_equal(after[0]["mean"], rc.energies(2, 0).astype(np.float64)) and (after[0]["m2"] == 0).all()
    assert fresh.history[0].tolist() == [0, 1, 2, 3, 4] and (fresh.history[1:] == -1).all()


def test_exchange_is_two_kernel_launches_whatever_the_batch():
    """The launch sequence of one m3g_remd_exchange captured (not executed) on a side stream: two kernel nodes and nothing else, for
    one ladder and for three."""
    from torch_m3gnet.replica_exchange import remd_exchange

    hip = C.CDLL("libamdhip64.so")
    hip.hipGraphGetNodes.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    hip.hipGraphNodeGetType.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    for ids in ([2], [0, 1, 2]):
        batch = Batch(ids)
        e = torch.tensor(np.concatenate([rc.energies(g, 0) for g in ids]), device=DEV)
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        graph, n = C.c_void_p(), C.c_size_t()
        with torch.cuda.stream(stream):
            assert hip.hipStreamBeginCapture(C.c_void_p(stream.cuda_stream), 2) == 0   # relaxed mode: this thread's other calls go on
            try:
                remd_exchange(batch.remd, batch.dyn, e, batch.history)
            finally:
                assert hip.hipStreamEndCapture(C.c_void_p(stream.cuda_stream), C.byref(graph)) == 0
        assert hip.hipGraphGetNodes(graph, None, C.byref(n)) == 0
        assert n.value == 2, n.value
        nodes = (C.c_void_p * 2)()
        assert hip.hipGraphGetNodes(graph, nodes, C.byref(n)) == 0
        for node in nodes:
            kind = C.c_int(-1)
            assert hip.hipGraphNodeGetType(C.c_void_p(node), C.byref(kind)) == 0
            assert kind.value == 0   # hipGraphNodeTypeKernel
        hip.hipGraphDestroy(graph)
        assert batch.remd.read()["n_attempts"].tolist() == [0] * len(ids)   # captured, not run


# ---- ReplicaExchange under the LJ-fitted model ----------------------------------------------------------------------------------------
TEMPS = [300.0, 350.0, 410.0, 480.0]
STEPS, INTERVAL = 200, 10


def _fcc(a, n):
    grid = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1).reshape(-1, 1, 3)
    return (grid + FCC_BASE[None]).reshape(-1, 3) * a, np.eye(3) * n * a


@pytest.fixture(scope="module")
def cu_runs():
    from torch_m3gnet.dynamics import structure_seeds
    from torch_m3gnet.model.build import build_model_from_npz
    from torch_m3gnet.replica_exchange import ReplicaExchange

    model = build_model_from_npz(GOLDEN / "model_fitted_lj.npz").to(DEV)
    pos, lat = _fcc(3.61, 2)
    other = pos + np.random.default_rng(3).normal(0, 0.03, pos.shape)
    z = np.full(32, 29)
    kw = dict(timestep=2.0, friction=0.02, exchange_interval=INTERVAL)
    both = ReplicaExchange(model, TEMPS, seed=4, **kw).run([lat, lat], [pos, other], [z, z], STEPS, loginterval=1)
    alone = ReplicaExchange(model, TEMPS, seed=[int(structure_seeds(4, 2)[1])], **kw).run([lat], [other], [z], STEPS, loginterval=1)
    return both, alone


def test_replica_exchange_run_keeps_its_books(cu_runs):
    both, _ = cu_runs
    n_att = (STEPS - 1) // INTERVAL
    assert n_att == 19 and len(both) == 2
    for res in both:
        assert not res["error"] and not any(r["error"] for r in res["replicas"])
        assert np.array_equal(res["temperatures"], TEMPS)
        hist = res["temperature_index"]
        assert hist.shape == (n_att + 1, 4) and (np.sort(hist, axis=1) == np.arange(4)[None]).all() and list(hist[0]) == [0, 1, 2, 3]
        assert list(res["attempts"]) == [10, 9, 10]   # pairs of parity a % 2 at attempts a = 0 .. 18
        accepts = np.rint(res["acceptance"] * res["attempts"]).astype(int)
        assert (accepts >= 0).all() and (accepts <= res["attempts"]).all() and accepts.sum() > 0
        moves = (np.diff(hist, axis=0) != 0).sum() // 2
        assert moves == accepts.sum()
        assert np.isfinite(res["mean_energy"]).all() and (res["heat_capacity"] > 0).all() and (res["round_trips"] >= 0).all()
        for idx, rep in enumerate(res["replicas"]):   # ordered by the temperature held at the end
            assert rep["temperature"] == TEMPS[idx] == rep["target_temperature"]
            assert hist[-1, rep["replica"]] == idx and rep["n_steps"] == STEPS
            assert rep["log"]["step"].tolist() == list(range(STEPS + 1))
        # across an accepted swap the kinetic temperature changes by exactly T_new / T_old, and not at all otherwise
        t_kin = res["kinetic_temperature"]
        assert t_kin.shape == (n_att, 2, 4)
        for a in range(n_att):
            for r in range(4):
                ratio = TEMPS[hist[a + 1, r]] / TEMPS[hist[a, r]]
                if ratio == 1.0:
                    assert t_kin[a, 1, r] == t_kin[a, 0, r]
                else:
                    assert abs(t_kin[a, 1, r] / t_kin[a, 0, r] / ratio - 1.0) < 1e-12, (a, r)


def test_replica_exchange_ladder_alone_equals_the_ladder_in_the_batch(cu_runs):
    both, (alone,) = cu_runs
    res = both[1]
    for key in ("temperatures", "attempts", "acceptance", "mean_energy", "heat_capacity", "round_trips", "temperature_index",
                "kinetic_temperature"):
        assert np.array_equal(alone[key], res[key]), key
    for ra, rb in zip(alone["replicas"], res["replicas"]):
        assert ra["replica"] == rb["replica"] and ra["total_energy"] == rb["total_energy"]
        for key in ("positions", "velocities", "forces"):
            assert np.array_equal(ra[key], rb[key]), key
        for key in ra["log"]:
            assert np.array_equal(ra["log"][key], rb["log"][key]), key
    assert not np.array_equal(both[0]["replicas"][0]["positions"], res["replicas"][0]["positions"])
