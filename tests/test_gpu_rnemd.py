"""Reverse non-equilibrium MD on the MI355X at kernel level (torch_m3gnet.transport, C ABI m3g_rnemd_*; no model): the two kernels
against the restatement (tests/rnemd_reference.py) BITWISE -- velocities, pairs, counters, the transferred amount, slab counts and slab
sums, whose device order the restatement repeats -- on a batch of 7, 257 and 64 atoms: a part-filled chunk, a one-row second chunk that
holds the best candidate, triclinic cells with positions spread over -2 .. 3 cells, atoms exactly on slab planes and at f = -1e-17,
a slab 0 with fewer atoms than n_swaps, an empty middle slab, duplicated velocity rows, equal and mixed masses, an `active` mask."""
import ctypes as C

import numpy as np
import pytest
import torch

import rnemd_cases as cases
from rnemd_cases import AXIS, CASES, FLOW, SIZES

pytestmark = pytest.mark.gpu
DEV = "cuda"


class Batch:
    def __init__(self, case, ids=(0, 1, 2), cold_c=False):
        from torch_m3gnet.dynamics import DynState
        from torch_m3gnet.transport import RnemdState

        self.kind, self.n_slabs, self.n_swaps, self.mixed, self.masked = case
        self.ids = list(ids)
        self.parts = cases.parts_of(case, self.ids, cold_c)
        self.offsets = np.concatenate([[0], np.cumsum([len(p[1]) for p in self.parts])])
        self.S, self.N = len(self.parts), int(self.offsets[-1])
        pos = torch.tensor(np.concatenate([p[1] for p in self.parts]), dtype=torch.float64, device=DEV)
        self.lat = np.stack([p[0] for p in self.parts])
        self.v0 = np.concatenate([p[3] for p in self.parts])
        self.dyn = DynState(pos, torch.tensor(self.lat, device=DEV), self.offsets, np.concatenate([p[2] for p in self.parts]),
                            torch.tensor(self.v0, device=DEV), 300.0, np.arange(self.S, dtype=np.uint64), ensemble="nve", dt=1.0)
        active = np.concatenate([p[4] for p in self.parts]) if self.masked else None
        self.rn = RnemdState(self.offsets, self.lat, self.kind, AXIS, self.n_slabs, self.n_swaps, flow_axis=FLOW, active=active, device=DEV)
        self.refs = cases.references(case, self.parts)
        self.force = torch.zeros(self.N, 3, dtype=torch.float32, device=DEV)
        self.stress = torch.zeros(self.S, 6, dtype=torch.float32, device=DEV)

    def settle(self, nan_row=None, finish_only=True):
        """One dyn_step at zero forces (the synchronous point of the exchange); `nan_row`: that row's force is NaN."""
        from torch_m3gnet.dynamics import dyn_step

        f = self.force.clone()
        if nan_row is not None:
            f[nan_row, 1] = float("nan")
        dyn_step(self.dyn, f, self.stress, finish_only=finish_only)
        return self

    def exchange(self, swap=True, sample=True, check=True):
        """One device call; the restatement makes the same call on what the device held before it, and must agree bitwise after."""
        from torch_m3gnet.transport import rnemd_exchange

        pos, before = self.dyn.pos.cpu().numpy(), self.dyn.velocities.cpu().numpy()
        flags = self.dyn.read()["flags"]
        rnemd_exchange(self.rn, self.dyn, self.dyn.pos, swap=swap, sample=sample)
        after = self.dyn.velocities.cpu().numpy()
        if check:
            want = before.copy()
            for s, ref in enumerate(self.refs):
                a, b = self.offsets[s], self.offsets[s + 1]
                ref.exchange(pos[a:b], want[a:b], swap=swap, sample=sample, flags=int(flags[s]))
            assert np.array_equal(after.view(np.int64), want.view(np.int64)), "velocities"
            assert np.array_equal(self.dyn.pos.cpu().numpy(), pos)
            self.compare(self.rn.read())
        return before, after

    def compare(self, out):
        for s, ref in enumerate(self.refs):
            assert (out["n_calls"][s], out["n_exchanged"][s], out["n_samples"][s]) == (ref.n_calls, ref.n_exchanged, ref.n_samples), s
            assert np.array_equal(out["last_pairs"][s], ref.last_pairs), (s, out["last_pairs"][s], ref.last_pairs)
            assert out["transferred"][s].tobytes() == np.float64(ref.transferred).tobytes(), (s, out["transferred"][s], ref.transferred)
            assert np.array_equal(out["count"][s], ref.count), (s, out["count"][s], ref.count)
            assert np.array_equal(out["sums"][s].view(np.int64), ref.sums.view(np.int64)), (s, np.abs(out["sums"][s] - ref.sums).max())

    def result(self) -> dict:
        return dict(self.rn.read(), v=self.dyn.velocities.cpu().numpy())


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_kernels_match_the_restatement_bitwise(case):
    kind, n_slabs, n_swaps, mixed, masked = case
    batch = Batch(case).settle()
    assert np.array_equal(batch.dyn.velocities.cpu().numpy(), batch.v0) and batch.dyn.read()["flags"].tolist() == [0, 0, 0]
    for call in range(3):   # the second and third calls find what the ones before left, and add to the accumulators
        before, after = batch.exchange()
        pairs = batch.rn.read()["last_pairs"]
        for s in range(3):
            a, b = batch.offsets[s], batch.offsets[s + 1]
            rows = pairs[s][pairs[s] >= 0]
            assert len(set(rows)) == len(rows)
            rest = np.setdiff1d(np.arange(b - a), rows)
            assert np.array_equal(after[a:b][rest], before[a:b][rest])                  # rows not in last_pairs: bitwise untouched
            assert batch.parts[s][4][rows].all()                                        # only active rows move
            if not mixed and kind == "heat":
                assert sorted(map(tuple, after[a:b])) == sorted(map(tuple, before[a:b]))   # a permutation of the rows
            if not mixed and kind == "momentum":
                assert sorted(after[a:b, FLOW]) == sorted(before[a:b, FLOW]) and np.array_equal(after[a:b, 1:], before[a:b, 1:])
        if call == 0:
            first = pairs.copy()
    cases.check_construction(case, batch.refs, first, 3)


def test_no_exchange_where_slab_0_is_not_ahead_and_swap_off_touches_nothing():
    for case in (("heat", 2, 8, False, False), ("momentum", 2, 8, False, False)):
        batch = Batch(case, cold_c=True).settle()
        before, after = batch.exchange()
        a, b = batch.offsets[2], batch.offsets[3]
        assert np.array_equal(after[a:b], before[a:b]) and not np.array_equal(after[:a], before[:a])
        out = batch.rn.read()
        assert out["n_exchanged"][2] == 0 and (out["last_pairs"][2] == -1).all() and out["transferred"][2] == 0.0
        assert out["n_calls"][2] == 1 and out["count"][2].sum() == 64 and out["n_exchanged"][1] == 8
        before, after = batch.exchange(swap=False)     # sampling only: every velocity stays, the pairs of the last swapping call too
        assert np.array_equal(after, before)
        again = batch.rn.read()
        assert np.array_equal(again["last_pairs"], out["last_pairs"]) and np.array_equal(again["transferred"], out["transferred"])
        assert again["n_samples"].tolist() == [2, 2, 2] and np.array_equal(again["count"], 2 * out["count"])
        before, after = batch.exchange(sample=False)   # exchange only: the accumulators stay
        final = batch.rn.read()
        assert np.array_equal(final["count"], again["count"]) and np.array_equal(final["sums"], again["sums"]) and final["n_calls"].tolist() == [3] * 3


def test_a_flagged_structure_is_untouched_and_unsampled_and_its_neighbours_are_unaffected():
    from torch_m3gnet import _lib

    case = ("heat", 6, 3, True, True)
    # ERROR: a NaN force on a row of B in the finishing kick freezes B; A and C go on
    batch = Batch(case).settle(finish_only=False).settle(nan_row=7 + 5)
    flags = batch.dyn.read()["flags"]
    assert [bool(f & _lib.DYN_ERROR) for f in flags] == [False, True, False] and not any(f & _lib.DYN_STARTED for f in flags[[0, 2]])
    before, after = batch.exchange()
    a, b = batch.offsets[1], batch.offsets[2]
    assert np.array_equal(after[a:b].view(np.int64), before[a:b].view(np.int64))
    out = batch.rn.read()
    assert (out["n_calls"].tolist(), out["n_samples"].tolist()) == ([1, 0, 1], [1, 0, 1])
    assert out["count"][1].sum() == 0 and (out["sums"][1] == 0).all() and (out["last_pairs"][1] == -1).all() and out["transferred"][1] == 0.0
    assert out["n_exchanged"][0] + out["n_exchanged"][2] > 0
    # the neighbours equal their runs alone through the same calls
    for g in (0, 2):
        alone = Batch(case, ids=[g]).settle(finish_only=False).settle()
        alone.exchange()
        o = alone.result()
        lo, hi = batch.offsets[g], batch.offsets[g + 1]
        assert np.array_equal(o["v"], after[lo:hi])
        for key in ("n_calls", "n_exchanged", "transferred", "n_samples", "last_pairs", "count", "sums"):
            assert np.array_equal(o[key][0], out[key][g]), (g, key)
    # STARTED: half-step velocities -- nothing of any structure is written
    batch = Batch(case).settle(finish_only=False)
    assert all(f & _lib.DYN_STARTED for f in batch.dyn.read()["flags"])
    before, after = batch.exchange()
    assert np.array_equal(after.view(np.int64), before.view(np.int64))
    out = batch.rn.read()
    assert out["n_calls"].tolist() == [0, 0, 0] and out["count"].sum() == 0 and (out["last_pairs"] == -1).all()


@pytest.mark.parametrize("case", [CASES[1], CASES[4]], ids=lambda c: "-".join(map(str, c)))
def test_structures_are_bitwise_independent_of_the_batch_and_reproducible(case):
    def run(ids):
        batch = Batch(case, ids=ids).settle()
        for _ in range(2):
            batch.exchange(check=False)
        return batch, batch.result()

    first, a = run((0, 1, 2))
    _, b = run((0, 1, 2))
    for key in a:
        assert np.array_equal(a[key], b[key]), key
    for order in ([0], [1], [2], [2, 0]):
        _, o = run(order)
        for j, g in enumerate(order):
            lo, hi = first.offsets[g], first.offsets[g + 1]
            at = sum(SIZES[x] for x in order[:j])
            assert np.array_equal(o["v"][at:at + SIZES[g]].view(np.int64), a["v"][lo:hi].view(np.int64)), (order, g)
            for key in ("n_calls", "n_exchanged", "transferred", "n_samples", "last_pairs", "count", "sums"):
                assert np.array_equal(o[key][j], a[key][g]), (order, g, key)
    assert a["n_exchanged"][1] > 0


def test_exchange_capture_replays_bitwise():
    from torch_m3gnet.transport import rnemd_exchange

    case = CASES[1]
    eager, graphed = Batch(case).settle(), Batch(case).settle()
    for _ in range(4):
        rnemd_exchange(eager.rn, eager.dyn, eager.dyn.pos)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rnemd_exchange(graphed.rn, graphed.dyn, graphed.dyn.pos)
    assert graphed.rn.read()["n_calls"].tolist() == [0, 0, 0]   # captured, not run
    for _ in range(4):
        g.replay()
    torch.cuda.synchronize()
    a, b = eager.result(), graphed.result()
    for key in a:
        assert np.array_equal(a[key], b[key]), key
    assert a["n_calls"].tolist() == [4, 4, 4] and a["n_exchanged"][1] > 0


def test_exchange_is_two_kernel_launches_whatever_the_batch():
    """The launch sequence of one m3g_rnemd_exchange captured (not executed) on a side stream: two kernel nodes and nothing else."""
    from torch_m3gnet.transport import rnemd_exchange

    hip = C.CDLL("libamdhip64.so")
    hip.hipGraphGetNodes.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    hip.hipGraphNodeGetType.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    for case, ids in ((CASES[0], [0]), (CASES[2], [0, 1, 2])):
        batch = Batch(case, ids=ids).settle()
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        graph, n = C.c_void_p(), C.c_size_t()
        with torch.cuda.stream(stream):
            assert hip.hipStreamBeginCapture(C.c_void_p(stream.cuda_stream), 2) == 0   # relaxed mode: this thread's other calls go on
            try:
                rnemd_exchange(batch.rn, batch.dyn, batch.dyn.pos)
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
        assert batch.rn.read()["n_calls"].tolist() == [0] * len(ids)   # captured, not run
