"""Batched atom-swap Monte Carlo on the MI355X (torch_m3gnet.monte_carlo, C ABI m3g_mc_*): the three kernels against the restatement
(tests/mc_reference.py, cases of tests/mc_cases.py), the runs over a dynamics state, bitwise independence of the batch and
reproducibility, the protocol, the launch counts, and SwapMonteCarlo runs (pure and hybrid) of a 32-atom two-species fcc cell under a
committed golden model."""
import ctypes as C

import numpy as np
import pytest
import torch

import mc_cases as mcc
import mc_reference as mcr
import md_reference as mr
from helpers import build_engine_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
FCC_BASE = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])


def _rel(a, b, floor=1e-300):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), floor))


class Batch:
    """The structures `ids` of mcc.STRUCTURES as one McState with caller-owned species, current energies, forces and stresses."""

    def __init__(self, ids, rounds=mcc.ROUNDS, bad=None, with_forces=True):
        from torch_m3gnet.monte_carlo import McState

        self.ids, self.rounds, self.with_forces = list(ids), rounds, with_forces
        sizes = [len(mcc.STRUCTURES[g][0]) for g in self.ids]
        self.offsets = np.concatenate([[0], np.cumsum(sizes)])
        self.S, self.N = len(self.ids), int(self.offsets[-1])
        self.mc = McState(self.offsets, [mcc.STRUCTURES[g][1] for g in self.ids], np.array([mcc.STRUCTURES[g][2] for g in self.ids], dtype=np.uint64),
                          np.concatenate([mcc.mask(g) for g in self.ids]), device=DEV)
        dev = lambda x: torch.tensor(np.ascontiguousarray(x), device=DEV)
        self.types = dev(np.concatenate([mcc.STRUCTURES[g][0] for g in self.ids]))
        # every evaluation of the run, made once: call 0 is the start, call r + 1 the trial of round r
        self.e_all = dev(np.array([[mcc.energies(g, c, bad) for g in self.ids] for c in range(rounds + 1)], dtype=np.float32))
        self.e = self.e_all[0].clone()
        self.f = self.s = self.f_all = self.s_all = None
        if with_forces:
            self.f_all = dev(np.stack([np.concatenate([mcc.forces(g, c) for g in self.ids]) for c in range(rounds + 1)]))
            self.s_all = dev(np.stack([np.stack([mcc.stresses(g, c) for g in self.ids]) for c in range(rounds + 1)]))
            self.f, self.s = self.f_all[0].clone(), self.s_all[0].clone()
        self.history = torch.full((rounds, self.S, 3), mcc.UNTOUCHED, dtype=torch.int32, device=DEV)
        self.types_log, self.e_log = [], []

    def propose(self):
        from torch_m3gnet.monte_carlo import mc_propose

        mc_propose(self.mc, self.types, self.e)

    def decide(self, r):
        from torch_m3gnet.monte_carlo import mc_decide

        if self.with_forces:
            mc_decide(self.mc, self.types, self.e_all[r + 1], self.e, self.f_all[r + 1], self.f, self.s_all[r + 1], self.s, history=self.history)
        else:
            mc_decide(self.mc, self.types, self.e_all[r + 1], self.e, history=self.history)

    def run(self):
        for r in range(self.rounds):
            self.propose()
            self.decide(r)
            self.types_log.append(self.types.clone())
            self.e_log.append(self.e.clone())
        torch.cuda.synchronize()
        return self

    def result(self) -> dict:
        out = self.mc.read()
        out.update(types=self.types.cpu().numpy(), e=self.e.cpu().numpy(), history=self.history.cpu().numpy(),
                   types_log=torch.stack(self.types_log).cpu().numpy(), e_log=torch.stack(self.e_log).cpu().numpy())
        if self.with_forces:
            out.update(f=self.f.cpu().numpy(), s=self.s.cpu().numpy())
        return out


def _compare(batch: Batch, out: dict, refs: list) -> None:
    """Every structure of the batch against its reference run: picks, verdicts, species, counters and history exactly, the current
    energies / forces / stresses bitwise, the Welford statistics to 1e-12."""
    for j, ref in enumerate(refs):
        mc, a, b = ref["mc"], batch.offsets[j], batch.offsets[j + 1]
        assert np.array_equal(out["history"][:, j], mc.history_array(batch.rounds, mcc.UNTOUCHED)), j
        assert np.array_equal(out["types_log"][:, a:b], ref["types"]), j
        assert np.array_equal(out["e_log"][:, j].view(np.int32), ref["e"].view(np.int32)), j
        assert out["flags"][j] == mc.flags and out["n_proposals"][j] == mc.counter
        assert (out["attempts"][j], out["accepts"][j], out["nonfinite"][j], out["count"][j]) == (mc.attempts, mc.accepts, mc.nonfinite, mc.count)
        if mc.attempts:
            assert tuple(out["pair"][j]) == mc.pair
            assert abs(out["mean"][j] - mc.mean) <= 1e-12 * abs(mc.mean) and abs(out["m2"][j] - mc.m2) <= 1e-12 * max(mc.m2, 1e-30), j
        else:
            assert out["mean"][j] == 0.0 and out["m2"][j] == 0.0
        if batch.with_forces:
            assert np.array_equal(out["f"][a:b].view(np.int32), ref["f"].view(np.int32)), j
            assert np.array_equal(out["s"][j].view(np.int32), ref["s"].view(np.int32)), j


@pytest.fixture(scope="module")
def references():
    return [mcc.reference(g) for g in range(len(mcc.STRUCTURES))]


@pytest.fixture(scope="module")
def full_run():
    return Batch(range(len(mcc.STRUCTURES))).run()


def test_kernels_match_the_restatement(references, full_run):
    """All eight structures in one batch through 200 propose / decide rounds with forces and stresses."""
    out = full_run.result()
    _compare(full_run, out, references)
    for g, ref in enumerate(references):
        mc = ref["mc"]
        if g in (6, 7):   # one species / one active row
            assert mc.flags == mcr.NO_PAIR and mc.attempts == 0 and (out["history"][:, g] == -1).all()
            continue
        assert min(abs(m) for m in mc.margins) > 1e-9          # (tests/test_mc_cpu.py checks the same without a GPU)
        assert 0 < mc.accepts < mc.attempts == mcc.ROUNDS      # both verdicts occur
    # the masked structure: the rows outside the mask never changed, and no row of the left-out species was ever picked
    a, b = full_run.offsets[3], full_run.offsets[4]
    z, inactive = mcc.STRUCTURES[3][0], ~mcc.mask(3)
    assert (out["types_log"][:, a:b][:, inactive] == z[inactive][None]).all()
    assert not inactive[out["history"][:, 3, :2]].any()


def test_energies_only_is_one_launch_less_and_decides_the_same(references):
    """Without forces and stresses (pure lattice Monte Carlo) the verdicts, species and statistics are the same."""
    ids = [0, 3, 5, 6]
    batch = Batch(ids, with_forces=False).run()
    _compare(batch, batch.result(), [references[g] for g in ids])


def test_structures_are_bitwise_independent_of_the_batch_and_reproducible(full_run):
    a = full_run.result()
    b = Batch(range(len(mcc.STRUCTURES))).run().result()
    for key in a:
        assert np.array_equal(a[key], b[key]), key
    for j in range(len(mcc.STRUCTURES)):
        o = Batch([j]).run().result()
        x, y = full_run.offsets[j], full_run.offsets[j + 1]
        for key in ("flags", "n_proposals", "attempts", "accepts", "nonfinite", "count", "mean", "m2", "pair", "e", "s"):
            assert np.array_equal(o[key][0], a[key][j]), (j, key)
        assert np.array_equal(o["history"][:, 0], a["history"][:, j]) and np.array_equal(o["e_log"][:, 0], a["e_log"][:, j])
        assert np.array_equal(o["types_log"], a["types_log"][:, x:y]) and np.array_equal(o["f"], a["f"][x:y])


# ---- over a dynamics state -------------------------------------------------------------------------------------------------------------
class DynBatch:
    """mcc.DYN_STRUCTURES as one DynState (Langevin) + McState."""

    def __init__(self):
        from torch_m3gnet import _lib
        from torch_m3gnet.dynamics import DynState
        from torch_m3gnet.monte_carlo import McState

        self.ids = ids = list(mcc.DYN_STRUCTURES)
        parts = [mcc.start(g) for g in ids]
        self.offsets = np.concatenate([[0], np.cumsum([len(p[1]) for p in parts])])
        self.S, self.N = len(ids), int(self.offsets[-1])
        temps = [mcc.STRUCTURES[g][1] for g in ids]
        seeds = np.array([mcc.STRUCTURES[g][2] for g in ids], dtype=np.uint64)
        dev = lambda x: torch.tensor(np.ascontiguousarray(x), device=DEV)
        self.dyn = DynState(dev(np.concatenate([p[1] for p in parts])), dev(np.stack([p[0] for p in parts])), self.offsets,
                            np.concatenate([p[2] for p in parts]), dev(np.concatenate([p[3] for p in parts])), temps, seeds,
                            ensemble="nvt_langevin", **mcc.DYN_PARAMS)
        self.mc = McState(self.offsets, temps, seeds, np.concatenate([mcc.mask(g) for g in ids]), device=DEV)
        mass_at, vel_at = C.c_size_t(), C.c_size_t()
        _lib.check(self.dyn.lib.m3g_dyn_state_view(self.N, self.S, C.byref(mass_at), C.byref(vel_at)))
        self.masses = self.dyn.state[mass_at.value:mass_at.value + 8 * self.N].view(torch.float64)   # live view
        self.types = dev(np.concatenate([mcc.STRUCTURES[g][0] for g in ids]))
        self.e = dev(np.array([mcc.energies(g, 0) for g in ids], dtype=np.float32))
        self.stress = torch.zeros(self.S, 6, dtype=torch.float32, device=DEV)
        self.history = torch.full((mcc.DYN_ROUNDS, self.S, 3), mcc.UNTOUCHED, dtype=torch.int32, device=DEV)
        self.snaps = []   # per swap: (m, v) before the proposal, after it, after the verdict

    def snap(self):
        return self.masses.clone(), self.dyn.velocities.clone()

    def run(self, ops, nan_force=None):
        from torch_m3gnet.dynamics import dyn_step
        from torch_m3gnet.monte_carlo import mc_decide, mc_propose

        for op in ops:
            if op[0] == "step":
                f = torch.tensor(np.concatenate([mcc.forces(g, op[1], nan_force) for g in self.ids]), device=DEV)
                dyn_step(self.dyn, f, self.stress, finish_only=op[2])
            else:
                trial = torch.tensor(np.array([mcc.energies(g, op[1] + 1) for g in self.ids], dtype=np.float32), device=DEV)
                before = self.snap()
                mc_propose(self.mc, self.types, self.e, self.dyn)
                mid = self.snap()
                mc_decide(self.mc, self.types, trial, self.e, dyn=self.dyn, history=self.history)
                self.snaps.append((before, mid, self.snap()))
        torch.cuda.synchronize()
        return self


def _swapped(x: np.ndarray, pair) -> np.ndarray:
    y = x.copy()
    if pair is not None:
        i, j = pair
        y[[i, j]] = x[[j, i]]
    return y


def _compare_dyn(batch: DynBatch, refs: list, n_swaps: int) -> None:
    out, dout = batch.mc.read(), batch.dyn.read()
    pos, types, e, hist = batch.dyn.pos.cpu().numpy(), batch.types.cpu().numpy(), batch.e.cpu().numpy(), batch.history.cpu().numpy()
    snaps = [[(m.cpu().numpy(), v.cpu().numpy()) for m, v in trio] for trio in batch.snaps]
    assert len(snaps) == n_swaps
    for j, ref in enumerate(refs):
        mc, dref, a, b = ref["mc"], ref["dyn"], batch.offsets[j], batch.offsets[j + 1]
        want = mc.history_array(mcc.DYN_ROUNDS, mcc.UNTOUCHED)
        assert np.array_equal(hist[:, j], want), j
        assert out["flags"][j] == mc.flags and (out["attempts"][j], out["accepts"][j], out["n_proposals"][j]) == (mc.attempts, mc.accepts, mc.counter)
        assert np.array_equal(types[a:b], np.array(mc.types)) and e[j] == np.float32(ref["e"])
        assert dout["flags"][j] == dref.flags and dout["n_steps"][j] == dref.n_steps
        assert _rel(pos[a:b], dref.pos) < 1e-12 and _rel(dout["v"][a:b], dref.v, 1e-4) < 1e-12, j
        assert np.array_equal(snaps[-1][2][0][a:b], dref.m)   # the masses, which no arithmetic touches: the reference's, bitwise
        for x, (before, mid, after) in enumerate(snaps):
            i, jj, verdict = want[x]
            pair = None if i < 0 else (i, jj)
            for q in (0, 1):   # masses, velocities: the two rows exchanged by the proposal, and exchanged back by a rejection, bitwise
                assert np.array_equal(mid[q][a:b], _swapped(before[q][a:b], pair)), (j, x, q)
                assert np.array_equal(after[q][a:b], mid[q][a:b] if verdict == 1 or pair is None else before[q][a:b]), (j, x, q)
            assert np.array_equal(after[0][a:b], ref["mv"][x][0]) and _rel(after[1][a:b], ref["mv"][x][1], 1e-4) < 1e-12
            ke = [float((m[a:b] * (v[a:b] ** 2).sum(1)).sum()) for m, v in (before, mid, after)]
            assert abs(ke[1] - ke[0]) <= 1e-13 * ke[0] and abs(ke[2] - ke[0]) <= 1e-13 * ke[0], (j, x, ke)


def test_masses_and_velocities_travel_with_the_atoms():
    ops = mcc.schedule()
    refs = [mcc.dyn_reference(g, ops) for g in mcc.DYN_STRUCTURES]
    batch = DynBatch().run(ops)
    _compare_dyn(batch, refs, mcc.DYN_ROUNDS)
    accepts = sum(ref["mc"].accepts for ref in refs)
    assert 0 < accepts < sum(ref["mc"].attempts for ref in refs)   # accepted and rejected trials both occur


def test_a_proposal_while_started_or_on_a_failed_structure_is_not_attempted():
    from torch_m3gnet import _lib

    ops = mcc.started_schedule()
    refs = [mcc.dyn_reference(g, ops) for g in mcc.DYN_STRUCTURES]
    batch = DynBatch().run(ops)
    _compare_dyn(batch, refs, 6)
    hist = batch.history.cpu().numpy()
    assert (hist[[1, 4]] == -1).all() and (hist[[0, 2, 3, 5], :, 2] >= 0).all() and (hist[6:] == mcc.UNTOUCHED).all()
    for x in (1, 4):
        for q in (0, 1):
            assert torch.equal(batch.snaps[x][0][q], batch.snaps[x][2][q])
    # a NaN force at call 6 (round 3) on the 65-atom structure: M3G_DYN_ERROR; from then on it is not attempted, the others go on
    ops = mcc.schedule()
    nan_force = {(3, 6): 17}
    refs = [mcc.dyn_reference(g, ops, nan_force=nan_force) for g in mcc.DYN_STRUCTURES]
    batch = DynBatch().run(ops, nan_force=nan_force)
    _compare_dyn(batch, refs, mcc.DYN_ROUNDS)
    assert [bool(f & _lib.DYN_ERROR) for f in batch.dyn.read()["flags"]] == [False, True, False]
    hist = batch.history.cpu().numpy()
    assert (hist[3:, 1] == -1).all() and (hist[:3, 1, 2] >= 0).all() and (hist[:, [0, 2], 2] >= 0).all()
    assert refs[1]["mc"].attempts == 3


# ---- protocol ---------------------------------------------------------------------------------------------------------------------------
def _state(batch: Batch) -> dict:
    torch.cuda.synchronize()
    out = batch.mc.read()
    out.update(types=batch.types.cpu().numpy(), e=batch.e.cpu().numpy(), f=batch.f.cpu().numpy(), s=batch.s.cpu().numpy(),
               history=batch.history.cpu().numpy())
    return out


def test_protocol_order_errors_idle_decides_and_non_finite_trials():
    from torch_m3gnet import _lib

    bad = {(1, 3): float("-inf"), (2, 3): float("nan"), (4, 3): float("inf")}
    batch = Batch([1, 2, 4], rounds=4, bad=bad)
    start = _state(batch)
    batch.propose()
    first = _state(batch)
    assert (first["flags"] == _lib.MC_PENDING).all() and (first["n_proposals"] == 1).all() and not np.array_equal(first["types"], start["types"])
    # propose twice without decide: M3G_MC_ERR_ORDER, the counter, and nothing else
    batch.propose()
    second = _state(batch)
    assert (second["flags"] == _lib.MC_PENDING | _lib.MC_ERR_ORDER).all() and (second["n_proposals"] == 2).all()
    for key in second:
        if key not in ("flags", "n_proposals"):
            assert np.array_equal(first[key], second[key]), key
    batch.decide(0)
    third = _state(batch)
    assert (third["flags"] == _lib.MC_ERR_ORDER).all() and (third["attempts"] == 1).all()
    assert (third["history"][0] == mcc.UNTOUCHED).all() and (third["history"][1, :, 2] >= 0).all()   # the row of the second call
    assert np.array_equal(third["history"][1, :, :2], first["pair"])
    # decide without a pending proposal changes nothing
    batch.decide(1)
    fourth = _state(batch)
    for key in fourth:
        assert np.array_equal(third[key], fourth[key]), key
    # a non-finite trial energy (call 3 = the trial of round 2) is rejected and everything restored bitwise
    batch.propose()
    pending = _state(batch)
    assert not np.array_equal(pending["types"], fourth["types"])
    batch.decide(2)
    fifth = _state(batch)
    assert (fifth["nonfinite"] == 1).all() and np.array_equal(fifth["accepts"], fourth["accepts"]) and (fifth["attempts"] == 2).all()
    for key in ("types", "e", "f", "s"):
        assert np.array_equal(fifth[key].view(np.int32 if fifth[key].dtype == np.float32 else fifth[key].dtype),
                              fourth[key].view(np.int32 if fourth[key].dtype == np.float32 else fourth[key].dtype)), key
    assert (fifth["history"][2, :, 2] == 0).all() and np.isfinite(fifth["mean"]).all() and np.isfinite(fifth["m2"]).all()


def test_propose_is_one_launch_and_decide_two_or_one_whatever_the_batch():
    """The launch sequences captured (not executed) on a side stream: kernel nodes only."""
    hip = C.CDLL("libamdhip64.so")
    hip.hipGraphGetNodes.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    hip.hipGraphNodeGetType.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    for ids in ([4], [0, 1, 2, 3, 4, 5]):
        for with_forces, what, want in ((True, "propose", 1), (True, "decide", 2), (False, "decide", 1)):
            batch = Batch(ids, rounds=1, with_forces=with_forces)
            torch.cuda.synchronize()
            stream = torch.cuda.Stream()
            stream.wait_stream(torch.cuda.current_stream())
            graph, n = C.c_void_p(), C.c_size_t()
            with torch.cuda.stream(stream):
                assert hip.hipStreamBeginCapture(C.c_void_p(stream.cuda_stream), 2) == 0   # relaxed mode: this thread's other calls go on
                try:
                    batch.propose() if what == "propose" else batch.decide(0)
                finally:
                    assert hip.hipStreamEndCapture(C.c_void_p(stream.cuda_stream), C.byref(graph)) == 0
            assert hip.hipGraphGetNodes(graph, None, C.byref(n)) == 0
            assert n.value == want, (ids, what, with_forces, n.value)
            nodes = (C.c_void_p * want)()
            assert hip.hipGraphGetNodes(graph, nodes, C.byref(n)) == 0
            for node in nodes:
                kind = C.c_int(-1)
                assert hip.hipGraphNodeGetType(C.c_void_p(node), C.byref(kind)) == 0
                assert kind.value == 0   # hipGraphNodeTypeKernel
            hip.hipGraphDestroy(graph)
            assert batch.mc.read()["n_proposals"].tolist() == [0] * len(ids)   # captured, not run


# ---- SwapMonteCarlo on the engine ----------------------------------------------------------------------------------------------------
# model_default_seed0 is a randomly initialised network: exchanging a Cu and an Au atom of this cell moves its energy (~ -1 eV) by
# 1e-6 - 2e-6 eV (its float32 grid there is 6e-8 eV), so kB T must be of that size for both verdicts to occur: kB 0.02 K = 1.7e-6 eV
T_PURE, TRIALS = 0.02, 40
SEEDS = [2 ** 63 + 21, 77, 2 ** 64 - 5]


def _cell(seed=3):
    """32-atom fcc cell, 16 Cu + 16 Au on shuffled sites, positions off the lattice by 0.03 A so that no two sites are equivalent."""
    grid = np.stack(np.meshgrid(*[np.arange(2)] * 3, indexing="ij"), -1).reshape(-1, 1, 3)
    pos = (grid + FCC_BASE[None]).reshape(-1, 3) * 3.9
    rng = np.random.default_rng(seed)
    z = rng.permutation(np.repeat([29, 79], 16))
    return np.eye(3) * 7.8, pos + rng.normal(0, 0.03, pos.shape), z


@pytest.fixture(scope="module")
def model():
    m, _ = build_engine_model("cu32", "ref")   # model_default_seed0: the embedding makes the energy depend on the species
    return m.to(DEV)


@pytest.fixture(scope="module")
def pure_runs(model):
    from torch_m3gnet.monte_carlo import SwapMonteCarlo

    lat, pos, z = _cell()
    others = [_cell(4), _cell(5)]
    kw = dict(structure_batches=True)
    alone = SwapMonteCarlo(model, T_PURE, seed=[SEEDS[1]], **kw)
    res = alone.run([lat], [pos], [z], TRIALS, loginterval=1)
    three = SwapMonteCarlo(model, [0.5 * T_PURE, T_PURE, 2.0 * T_PURE], seed=SEEDS, **kw).run(
        [others[0][0], lat, others[1][0]], [others[0][1], pos, others[1][1]], [others[0][2], z, others[1][2]], TRIALS, loginterval=1)
    return alone, res[0], three


def test_swap_monte_carlo_tracks_the_energy_of_the_configuration_it_holds(model, pure_runs):
    from torch_m3gnet.data.graph_gpu import batch_from_arrays
    from torch_m3gnet.data.md import VerletGraph

    driver, res, _ = pure_runs
    lat, pos, z = _cell()
    assert res["attempts"] == TRIALS and res["nonfinite"] == 0 and not res["error"] and "velocities" not in res
    assert np.array_equal(res["positions"], pos) and np.array_equal(res["lattice"], lat)            # bitwise: nothing moves
    assert sorted(res["atomic_numbers"]) == sorted(z) and not np.array_equal(res["atomic_numbers"], z)
    cfg = driver.model.engine.cfg
    fresh = driver.model(batch_from_arrays([lat], [pos], [res["atomic_numbers"]], cfg.cutoff, cfg.threebody_cutoff, device=DEV))
    e_fresh = float(fresh["total_energy"][0])
    print(f"tracked {res['total_energy']:.7f} eV, fresh evaluation of the final species {e_fresh:.7f} eV")
    assert abs(res["total_energy"] - e_fresh) <= 1e-5 * abs(e_fresh)
    # the same evaluation path on the same lists gives the tracked energy bit for bit (a swap moves this model's energy by ~20 ulp)
    again = VerletGraph([lat], [res["atomic_numbers"]], cfg.cutoff, cfg.threebody_cutoff, skin=driver.skin, device=DEV)
    assert float(again.step(driver.model, torch.tensor(pos, device=DEV), forces=False)["total_energy"][0]) == res["total_energy"]
    # every recorded pick and verdict re-derived by the restatement from the recorded energies
    ref = mcr.SwapReference(z - 1, T_PURE, SEEDS[1])
    # the energy of the starting configuration, as the run evaluated it (VerletGraph.step, energies only)
    vg = VerletGraph([lat], [z], cfg.cutoff, cfg.threebody_cutoff, skin=driver.skin, device=DEV)
    e = float(vg.step(driver.model, torch.tensor(pos, device=DEV), forces=False)["total_energy"][0])
    assert res["energy_at"].tolist() == list(range(TRIALS)) and res["swaps"].shape == (TRIALS, 3)
    for t in range(TRIALS):
        i, j, verdict = res["swaps"][t]
        assert ref.propose(e) == (i, j), t
        got, e = ref.decide(res["trial_energy"][t], e)
        assert got == verdict and e == res["energy"][t], t
    assert np.array_equal(np.array(ref.types) + 1, res["atomic_numbers"])
    assert min(abs(m) for m in ref.margins) > 1e-6   # the restatement's exp and the device's differ by ~1e-16: no verdict is near a tie
    share = ref.accepts / ref.attempts
    print(f"acceptance at {T_PURE} K: {share:.3f} ({ref.accepts} of {ref.attempts})")
    assert 0.1 <= share <= 0.9
    assert res["acceptance"] == share and res["mean_energy"] == pytest.approx(res["energy"].mean(), rel=1e-12)
    assert res["heat_capacity"] == pytest.approx(res["energy"].var() / (mcr.KB * T_PURE ** 2), rel=1e-6)


def test_swap_monte_carlo_structure_alone_equals_the_structure_in_a_batch(pure_runs):
    _, res, three = pure_runs
    assert np.array_equal(three[1]["swaps"], res["swaps"])
    for key in ("atomic_numbers", "energy", "trial_energy", "positions"):
        assert np.array_equal(three[1][key], res[key]), key
    assert three[1]["total_energy"] == res["total_energy"] and three[1]["mean_energy"] == res["mean_energy"]
    assert not np.array_equal(three[0]["swaps"], res["swaps"])


MD_STEPS, HYBRID_TRIALS, T_HYBRID = 5, 6, 0.02


def test_hybrid_run_equals_the_restatement_fed_the_devices_forces(model):
    """The hybrid loop written out with the thin layers, recording what the engine returned at every evaluation; DynReference +
    SwapReference fed those forces and energies reproduce it, and SwapMonteCarlo(md_steps=5) gives the same run bitwise."""
    from torch_m3gnet.data.atomic_masses import masses_of
    from torch_m3gnet.data.md import VerletGraph
    from torch_m3gnet.dynamics import DynState, dyn_step, maxwell_boltzmann
    from torch_m3gnet.monte_carlo import McState, SwapMonteCarlo, mc_decide, mc_propose

    lat, pos, z = _cell()
    seed = SEEDS[0]
    driver = SwapMonteCarlo(model, T_HYBRID, md_steps=MD_STEPS, timestep=2.0, friction=0.02, seed=[seed], structure_batches=True)
    res = driver.run([lat], [pos], [z], HYBRID_TRIALS, loginterval=1)[0]
    # the same loop by hand
    eng, cfg = driver.model, driver.model.engine.cfg
    vg = VerletGraph([lat], [z], cfg.cutoff, cfg.threebody_cutoff, skin=driver.skin, device=DEV)
    types = torch.tensor(z - 1, dtype=torch.int64, device=DEV)
    vg.use_atom_types(types)
    m = masses_of(z)
    v0 = maxwell_boltzmann(m, T_HYBRID, seed)
    pos_t = torch.tensor(pos, dtype=torch.float64, device=DEV)
    dyn = DynState(pos_t, vg.lattice.clone(), [0, 32], m, torch.tensor(v0, device=DEV), [T_HYBRID], np.array([seed], dtype=np.uint64),
                   ensemble="nvt_langevin", dt=2.0, friction=0.02)
    mc = McState([0, 32], [T_HYBRID], np.array([seed], dtype=np.uint64), np.ones(32, bool), device=DEV)
    history = torch.full((HYBRID_TRIALS, 1, 3), mcc.UNTOUCHED, dtype=torch.int32, device=DEV)
    dref = mr.DynReference(pos, lat, m, v0, "nvt_langevin", temperature=T_HYBRID, seed=seed, dt=2.0, friction=0.02)
    ref = mcr.SwapReference(z - 1, T_HYBRID, seed)
    steps = HYBRID_TRIALS * MD_STEPS
    for k in range(steps + 1):
        out = vg.step(eng, pos_t)
        f64 = out["forces"].double().cpu().numpy()
        if k > 0 and k % MD_STEPS == 0:
            cur = {key: out[key].clone() for key in ("total_energy", "forces", "stresses")}
            dyn_step(dyn, cur["forces"], cur["stresses"], finish_only=True)
            dref.step(f64, out["stresses"].double().cpu().numpy()[0], finish_only=True)
            mc_propose(mc, types, cur["total_energy"], dyn)
            pair = ref.propose_dyn(float(cur["total_energy"][0]), dref)
            trial = vg.step(eng, pos_t)
            mc_decide(mc, types, trial["total_energy"], cur["total_energy"], trial["forces"], cur["forces"], trial["stresses"], cur["stresses"],
                      dyn, history)
            verdict, _ = ref.decide_dyn(float(trial["total_energy"][0]), float(out["total_energy"][0]), dref)
            assert pair is not None and tuple(history[k // MD_STEPS - 1, 0].tolist()) == (pair[0], pair[1], verdict)
            f_cur = (trial if verdict else out)["forces"]
            assert torch.equal(cur["forces"], f_cur) and torch.equal(cur["stresses"], (trial if verdict else out)["stresses"])
            if k < steps:
                dyn_step(dyn, cur["forces"], cur["stresses"])
                dref.step(f_cur.double().cpu().numpy(), cur["stresses"].double().cpu().numpy()[0])
        else:
            dyn_step(dyn, out["forces"], out["stresses"], finish_only=(k == steps))
            dref.step(f64, out["stresses"].double().cpu().numpy()[0], finish_only=(k == steps))
    st = dyn.read()
    assert st["flags"][0] == dref.flags == 0 and st["n_steps"][0] == dref.n_steps == steps
    assert _rel(pos_t.cpu().numpy(), dref.pos) < 1e-12 and _rel(st["v"], dref.v) < 1e-12
    assert _rel(pos_t.cpu().numpy() - pos, dref.pos - pos) < 1e-9   # the displacements themselves (small at this temperature)
    assert np.array_equal(types.cpu().numpy(), np.array(ref.types)) and ref.attempts == HYBRID_TRIALS
    assert np.array_equal(history[:, 0].cpu().numpy(), ref.history_array(HYBRID_TRIALS, mcc.UNTOUCHED))
    # the driver ran the same loop
    assert np.array_equal(res["swaps"], history[:, 0].cpu().numpy())
    assert np.array_equal(res["positions"], pos_t.cpu().numpy()) and np.array_equal(res["velocities"], st["v"])
    assert np.array_equal(res["atomic_numbers"], types.cpu().numpy() + 1) and res["attempts"] == HYBRID_TRIALS and not res["error"]
    assert not np.array_equal(res["positions"], pos)
