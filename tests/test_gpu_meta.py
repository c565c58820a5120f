"""Collective-variable biasing on the MI355X at kernel level (torch_m3gnet.metadynamics, C ABI m3g_meta_*; no model, synthetic
forces): the three kernels against the restatement (tests/meta_reference.py) on the batch of tests/meta_cases.py -- 2, 7, 257 and 600
atoms in groups of 1, 1, 1 and 2 walkers, triclinic cells, positions spread over -2 .. 3 cells.  Everything free of `exp` BITWISE
(the CVs, the COORDINATION gradient rows, restraint and wall energies, dV/ds and forces_out without hills); the hill terms within a
gate derived in `hill_gates`."""
import ctypes as C

import numpy as np
import pytest
import torch

import meta_cases as mc
import meta_reference as mr

pytestmark = pytest.mark.gpu
DEV = "cuda"
ALL = (0, 1, 2, 3, 4)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


class Batch:
    """The device side of `slots` of mc.BATCH in walker groups of `groups`, and the restatement of the same."""

    def __init__(self, kinds, slots=ALL, groups=mc.GROUPS, restraint=True, height=0.05, inv_kdt=0.0, max_hills=16, exp=np.exp, device=True):
        self.kinds, self.slots, self.groups, self.n_cv = tuple(kinds), tuple(slots), tuple(groups), len(kinds)
        parts = [mc.structure(*mc.BATCH[q]) for q in self.slots]
        self.offsets = np.concatenate([[0], np.cumsum([len(p[1]) for p in parts])])
        self.S, self.N = len(parts), int(self.offsets[-1])
        self.positions = [p[1].copy() for p in parts]
        self.forces = np.concatenate([p[4] for p in parts])
        self.membership = np.concatenate([p[3][:self.n_cv] for p in parts], axis=1)
        self.refs = mc.reference_groups(self.kinds, self.slots, self.groups, restraint, height, inv_kdt, max_hills, exp=exp)
        self.state = None
        if not device:
            return
        from torch_m3gnet import metadynamics as md

        cvs = []
        for k, kind in enumerate(self.kinds):   # (the index lists are replaced by `membership` below: one atom each satisfies the checks)
            cvs.append({"distance": lambda: md.distance([0], [1]), "projection": lambda: md.projection([0], [1], mc.RAW_DIRECTIONS[k]),
                        "coordination": lambda: md.coordination([0], [1], mc.R0[k], mc.POWER[k], mc.R_CUT[k])}[kind]())
        rs = [mc.restraints(self.kinds, q, restraint) for q in self.slots]
        self.state = md.BiasState(self.offsets, np.stack([p[0] for p in parts]), cvs, np.concatenate([p[2] for p in parts]), mc.SIGMA[:self.n_cv],
                                  height=height, inv_kdt=inv_kdt, max_hills=max_hills, group_offsets=np.concatenate([[0], np.cumsum(self.groups)]),
                                  centres=np.stack([r[0] for r in rs]), kappa=np.stack([r[1] for r in rs]), walls=np.stack([r[2] for r in rs]),
                                  origins=np.stack([p[5][:self.n_cv] for p in parts]), membership=self.membership, device=DEV)
        self.pos = torch.tensor(np.concatenate(self.positions), device=DEV)
        self.f = torch.tensor(self.forces, device=DEV)

    def set_positions(self, slot_at: int, pos) -> None:
        self.positions[slot_at] = np.asarray(pos, dtype=np.float64)
        if self.state is not None:
            self.pos = torch.tensor(np.concatenate(self.positions), device=DEV)

    def set_hills(self, centres, heights) -> None:
        for ref, c, h in zip(self.refs, centres, heights):
            ref.set_hills(c, h)
        if self.state is not None:
            self.state.set_hills(centres, heights)

    def reference(self, deposit=False):
        return mc.reference_call(self.refs, self.slots, self.groups, deposit, self.positions)

    def device(self, deposit=False, alias=False) -> dict:
        from torch_m3gnet.metadynamics import bias_forces

        f = self.f.clone()
        out = bias_forces(self.state, self.pos, f, deposit=deposit, out=f if alias else None)
        return {"obs": self.state.obs.cpu().numpy(), "forces_out": out.cpu().numpy(), "gradients": self.state.gradients.cpu().numpy()}

    def result(self) -> dict:
        return dict(self.state.read(), obs=self.state.obs.cpu().numpy(), forces_out=self.state.forces_out.cpu().numpy())


CV_CASES = [("distance",), ("projection",), ("coordination",), ("coordination", "distance"), ("projection", "coordination"),
            ("coordination", "coordination")]


@pytest.mark.parametrize("kinds", CV_CASES, ids="-".join)
@pytest.mark.parametrize("restraint", [True, False], ids=["restraint-walls", "free"])
def test_everything_free_of_exp_matches_the_restatement_bitwise(kinds, restraint):
    batch = Batch(kinds, restraint=restraint)
    want_obs, want_f, extras = batch.reference()
    for alias in (False, True):
        got = batch.device(alias=alias)
        for col, what in ((0, "s_0"), (1, "s_1"), (2, "V"), (3, "V_hills"), (4, "V_restraint + walls"), (5, "dV/ds_0"), (6, "dV/ds_1"), (7, "height")):
            assert np.array_equal(bits(got["obs"][:, col]), bits(want_obs[:, col])), (what, got["obs"][:, col], want_obs[:, col])
        assert np.array_equal(bits(got["forces_out"]), bits(want_f)), np.abs(got["forces_out"] - want_f).max()
        for k, kind in enumerate(kinds):
            if kind != "coordination":
                continue
            grad = np.concatenate([x["grad"][k] for x in extras])
            rows = batch.membership[k] != 0
            assert np.array_equal(bits(got["gradients"][k][rows]), bits(grad[rows])), (k, np.abs(got["gradients"][k][rows] - grad[rows]).max())
            assert np.abs(grad[rows]).max() > 0.0
    untouched = (batch.membership == 0).all(axis=0)
    assert untouched.sum() > 20 and np.array_equal(bits(got["forces_out"][untouched]), bits(batch.forces[untouched]))   # membership 0: the bits pass through
    if restraint:
        assert (want_obs[:, 4] > 0).all() and not np.array_equal(got["forces_out"][~untouched], batch.forces[~untouched])
    else:
        assert np.array_equal(bits(got["forces_out"]), bits(batch.forces))   # no bias at all: every row passes, -0.0 included
    assert batch.state.read()["flags"].tolist() == [0] * 5


def test_a_coordination_pair_exactly_at_r_cut_contributes_exactly_zero():
    from torch_m3gnet import metadynamics as md

    lattice, pos, weights, _, forces, _ = mc.structure(0)
    r = mr.min_image_distance(pos, lattice, 0, 1)
    assert 2.0 < r < 4.0
    for r_cut, inside in ((r, False), (np.nextafter(r, np.inf), True), (r + 0.5, True)):
        state = md.BiasState([0, 2], lattice[None], [md.coordination([0], [1], 2.5, 3, r_cut)], weights, [0.5], centres=[1.0], kappa=[3.0], device=DEV)
        f = torch.tensor(forces, device=DEV)
        out = md.bias_forces(state, torch.tensor(pos, device=DEV), f).cpu().numpy()
        s, grad = state.obs.cpu().numpy()[0, 0], state.gradients.cpu().numpy()[0]
        ref = mr.evaluate([mr.Cv(mr.COORDINATION, [1, 2], p=3, r0=2.5, r_cut=r_cut)], pos, lattice, weights)
        assert bits(np.array([s]))[0] == bits(ref["s"])[0] and np.array_equal(bits(grad), bits(ref["grad"][0]))
        if inside:
            assert s >= 0.0 and (r_cut == r + 0.5) == (s > 1e-3)
        else:
            assert bits(np.array([s]))[0] == 0 and not grad.any() and np.array_equal(bits(out), bits(forces))   # +0.0, zero rows, untouched forces


def spread(batch, c: int) -> None:
    """Before call c > 0 every structure is stretched by 1 %: the centre CVs move off the hills deposited so far."""
    if c > 0:
        for at in range(batch.S):
            batch.set_positions(at, batch.positions[at] * 1.01)


def hill_gates(make, calls, move=None):
    """The gate of every quantity that holds an `exp`, from the restatement alone.  Two parts.  (1) The rounding of a sum of n terms
    in fp64 in two orders differs by at most (n - 1) 2^-53 sum |term| each, to first order; the device's order IS the restatement's, so
    this part only covers the terms themselves being rounded differently after an exp that differs: (n + 8) 2^-52 sum |term|, the 8
    for the products and the restraint terms added to the sum (sum |term| from the restatement, per sum).  (2) The device's exp and
    numpy's are each within 1 ulp of the true value, so they differ by at most 2 ulp; a hill's height is itself w0 exp(-V_hills
    inv_kdt) of earlier sums, so the differences compound.  The compounding is MEASURED: the whole sequence of calls is run through
    the restatement with every exp moved up, and down, by one ulp; the response to so small a change is linear, so twice the larger of
    the two responses bounds a 2-ulp difference.  Inputs keep V_hills inv_kdt <= 10 and the CVs of order 1 .. 10, so no exp
    argument amplifies a relative error by more than ~10.  Returns per call (gate of obs [S,8], gate of forces_out [N,3], gate of the
    hill heights per group)."""
    runs = {}
    for sign in (0, 1, -1):
        batch = make(mr.nudged_exp(sign) if sign else np.exp)
        rows = []
        for c, deposit in enumerate(calls):
            if move is not None:
                move(batch, c)
            obs, f_out, extras = batch.reference(deposit)
            rows.append((obs, f_out, extras, [ref.heights.copy() for ref in batch.refs], [ref.centres.copy() for ref in batch.refs],
                         [ref.n_hills for ref in batch.refs]))
        runs[sign] = (batch, rows)
    batch, plain = runs[0]
    gates = []
    for c, (obs, f_out, extras, heights, _, _) in enumerate(plain):
        response = lambda pick: 2.0 * np.maximum(np.abs(pick(runs[1][1][c]) - pick(plain[c])), np.abs(pick(runs[-1][1][c]) - pick(plain[c])))   # noqa: E731
        g_obs = response(lambda r: r[0])
        for s, x in enumerate(extras):
            rounding = (x["n_terms"] + 8) * 2.0 ** -52 * x["abs_sum"]
            g_obs[s, 2] += rounding[0] + 8 * 2.0 ** -52 * abs(obs[s, 2])
            g_obs[s, 3] += rounding[0]
            g_obs[s, 5:5 + batch.n_cv] += rounding[1:] + 8 * 2.0 ** -52 * np.abs(obs[s, 5:5 + batch.n_cv])
            g_obs[s, 7] += 8 * 2.0 ** -52 * abs(obs[s, 7])
        # forces_out = (float)(f - sum_k dV/ds_k grad_k): the gate of dV/ds_k times |grad_k|, and one float32 ulp where the rounding flips
        g_f = np.zeros_like(f_out, dtype=np.float64)
        for s, x in enumerate(extras):
            a, b = batch.offsets[s], batch.offsets[s + 1]
            for k in range(batch.n_cv):
                g_f[a:b] += g_obs[s, 5 + k] * np.abs(x["grad"][k])
        g_f += np.spacing(np.abs(f_out)).astype(np.float64) * (g_f > 0)
        g_h = [response(lambda r, g=g: r[3][g]) + 8 * 2.0 ** -52 * np.abs(heights[g]) for g in range(len(batch.refs))]
        gates.append((g_obs, g_f, g_h))
    return plain, gates


def starting_hills(kinds, n, seed=3):
    """n hills per group around where each group's first walker starts, heights of 0.2 .. 2 meV: V_hills below 1 eV at n = 1,000."""
    rng = np.random.default_rng(seed)
    centres, heights = [], []
    at = 0
    for R in mc.GROUPS:
        s = mc.cv_values(tuple(kinds), *mc.BATCH[at])
        centres.append(s[None, :] + rng.normal(0.0, 1.0, (n, len(kinds))) * mc.SIGMA[:len(kinds)] * 1.5)
        heights.append(rng.uniform(0.0002, 0.002, n))
        at += R
    return centres, heights


HILL_CASES = [(("projection",), 8.0), (("projection",), 0.0), (("distance", "projection"), 8.0), (("distance", "projection"), 0.0)]


@pytest.mark.parametrize("kinds,inv_kdt", HILL_CASES, ids=lambda v: "-".join(v) if isinstance(v, tuple) else ("well-tempered" if v else "plain"))
@pytest.mark.parametrize("loaded", [0, 1000], ids=["deposited", "1000-loaded"])
def test_hill_terms_match_the_restatement_within_the_derived_gate(kinds, inv_kdt, loaded):
    """Zero hills, then eight deposits through the deposit path (nine calls, the last one evaluating all eight; two walkers append
    16; the structures are stretched between the calls so that no walker sits on its own hills), or 1,000 hills loaded by m3g_meta_set_hills (a multiple of the two walkers) and two more deposits on top.  The gate is
    `hill_gates`; V_hills stays below ~1.2 eV and inv_kdt = 8 / eV (DeltaT ~ 1450 K), so V_hills inv_kdt <= 10."""
    calls = [True] * 8 + [False] if not loaded else [True, True, False]

    def make(exp, device=False):
        batch = Batch(kinds, height=0.05, inv_kdt=inv_kdt, max_hills=loaded + 16, exp=exp, device=device)
        if loaded:
            batch.set_hills(*starting_hills(kinds, loaded))
        return batch

    move = None if loaded else spread
    plain, gates = hill_gates(make, calls, move)
    batch = make(np.exp, device=True)
    worst = 0.0
    for c, deposit in enumerate(calls):
        if move is not None:
            move(batch, c)
        got = batch.device(deposit)
        (obs, f_out, extras, heights, centres, n_hills), (g_obs, g_f, g_h) = plain[c], gates[c]
        assert max(x["abs_sum"][0] for x in extras) * inv_kdt <= 10.0
        assert np.array_equal(bits(got["obs"][:, :2]), bits(obs[:, :2])) and np.array_equal(bits(got["obs"][:, 4]), bits(obs[:, 4]))
        err = np.abs(got["obs"] - obs)
        assert (err <= g_obs).all(), (c, err.max(), np.argwhere(err > g_obs)[:4], g_obs.max())
        assert (np.abs(got["forces_out"].astype(np.float64) - f_out) <= g_f).all(), c
        out = batch.state.read()
        for g in range(len(batch.refs)):
            assert out["n_hills"][g] == n_hills[g]
            assert np.array_equal(bits(out["centres"][g]), bits(centres[g])), (c, g)      # the centres are CVs: free of exp
            assert (np.abs(out["heights"][g] - heights[g]) <= g_h[g]).all(), (c, g)
        worst = max(worst, (err[:, 3] / np.maximum(g_obs[:, 3], 1e-300)).max())
    assert (plain[-1][0][:, 3] > 0).all() and g_obs[:, 3].max() < 1e-9 * np.abs(plain[-1][0][:, 3]).max()   # the gate is a rounding gate
    assert worst <= 1.0
    if inv_kdt:
        assert (plain[-1][3][3][loaded + 2:loaded + 4] < 0.05).all()     # well-tempered: the heights decay under the hills before
    else:
        assert (plain[-1][3][3][loaded:loaded + 4] == 0.05).all()    # plain: exp(-0) = 1 exactly


def test_two_walkers_write_their_slots_in_order_and_a_full_list_is_sticky():
    batch = Batch(("projection", "distance"), slots=(3, 4, 1), groups=(2, 1), max_hills=5, restraint=False)
    seen = []
    for c in range(7):
        if c in (1, 4):   # the walkers move between deposits
            batch.set_positions(0, batch.positions[0] + 0.01 * (c + 1))
            batch.set_positions(1, batch.positions[1] - 0.02 * (c + 1))
        got = batch.device(deposit=(c != 3))
        seen.append(got["obs"].copy())
        out = batch.state.read()
        deposits = c + 1 - (c >= 3)
        two, one = min(deposits, 2), min(deposits, 5)      # max_hills = 5 holds two deposits of two walkers, five of one
        assert out["n_hills"].tolist() == [2 * two, one] and out["deposits"].tolist() == [two, two, one]
        assert out["flags"].tolist() == [2 * (deposits > 2)] * 2 + [2 * (deposits > 5)], (c, out["flags"])
    steps = [0, 1, 2, 4, 5, 6]     # the calls that deposited
    for d in range(2):
        for r in range(2):           # walker r of the pair wrote slot d * 2 + r at its own CV of that call
            assert np.array_equal(bits(out["centres"][0, 2 * d + r]), bits(seen[steps[d]][r, :2]))
            assert out["heights"][0, 2 * d + r] == seen[steps[d]][r, 7] > 0.0
    assert not out["centres"][0, 4].any() and out["heights"][0, 4] == 0.0            # nothing is written past the last full deposit
    assert (seen[steps[2]][:2, 7] == 0.0).all() and seen[steps[2]][2, 7] > 0.0      # a full group deposits nothing, its neighbour goes on
    for d in range(5):
        assert np.array_equal(bits(out["centres"][1, d]), bits(seen[steps[d]][2, :2]))
    assert (seen[-1][:, 3] > 0).all()   # the run goes on under the hills it has


def test_a_nan_position_is_flagged_passes_its_forces_and_leaves_the_others_untouched():
    kinds = ("coordination", "projection")
    clean, dirty = Batch(kinds, max_hills=4), Batch(kinds, max_hills=4)
    row = int(np.flatnonzero(dirty.membership[0, dirty.offsets[2]:dirty.offsets[3]])[5])
    pos = dirty.positions[2].copy()
    pos[row, 1] = np.nan
    dirty.set_positions(2, pos)
    for deposit in (True, False):
        a, b = clean.device(deposit), dirty.device(deposit)
        lo, hi = dirty.offsets[2], dirty.offsets[3]
        assert np.array_equal(bits(b["forces_out"][lo:hi]), bits(dirty.forces[lo:hi]))
        others = np.r_[0:lo, hi:dirty.N]
        assert np.array_equal(bits(a["forces_out"][others]), bits(b["forces_out"][others]))
        assert np.array_equal(bits(a["obs"][[0, 1, 3, 4]]), bits(b["obs"][[0, 1, 3, 4]]))
        assert not b["obs"][2, 2:].any()
    x, y = clean.state.read(), dirty.state.read()
    assert y["flags"].tolist() == [0, 0, 1, 0, 0] and x["flags"].tolist() == [0] * 5
    assert y["n_hills"].tolist() == x["n_hills"].tolist() == [1, 1, 1, 2]             # the slot arithmetic holds
    assert y["heights"][2, 0] == 0.0 and not y["centres"][2, 0].any() and x["heights"][2, 0] > 0.0
    for g in (0, 1, 3):
        assert np.array_equal(bits(x["centres"][g]), bits(y["centres"][g])) and np.array_equal(bits(x["heights"][g]), bits(y["heights"][g]))
    want_obs, want_f, _ = dirty.reference(True)     # the restatement flags and passes the same
    assert dirty.refs[2].flags == [1] and np.array_equal(bits(want_f[lo:hi]), bits(dirty.forces[lo:hi]))


def _walk(batch, calls=(False, True, True, False)):
    for deposit in calls:
        batch.device(deposit)
    return batch.result()


@pytest.mark.parametrize("kinds", [("coordination", "distance"), ("projection",)], ids="-".join)
def test_a_group_is_bitwise_the_same_alone_and_in_the_batch_and_runs_repeat(kinds):
    whole, again = _walk(Batch(kinds, inv_kdt=8.0)), _walk(Batch(kinds, inv_kdt=8.0))
    for key in whole:
        assert np.array_equal(whole[key], again[key], equal_nan=True), key
    offsets = Batch(kinds, device=False).offsets
    at = 0
    for g, R in enumerate(mc.GROUPS):
        alone = _walk(Batch(kinds, slots=ALL[at:at + R], groups=(R,), inv_kdt=8.0))
        rows = slice(offsets[at], offsets[at + R])
        assert np.array_equal(bits(alone["obs"]), bits(whole["obs"][at:at + R])), g
        assert np.array_equal(bits(alone["forces_out"]), bits(whole["forces_out"][rows])), g
        assert np.array_equal(bits(alone["centres"][0]), bits(whole["centres"][g])) and np.array_equal(bits(alone["heights"][0]), bits(whole["heights"][g]))
        assert alone["n_hills"][0] == whole["n_hills"][g] == 2 * R and alone["flags"].tolist() == whole["flags"][at:at + R].tolist()
        at += R


def test_bias_capture_replays_bitwise():
    from torch_m3gnet.metadynamics import bias_forces

    kinds = ("coordination", "projection")
    eager, graphed = Batch(kinds, inv_kdt=8.0), Batch(kinds, inv_kdt=8.0)
    for _ in range(4):
        bias_forces(eager.state, eager.pos, eager.f, deposit=True)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        bias_forces(graphed.state, graphed.pos, graphed.f, deposit=True)
    assert graphed.state.read()["n_hills"].tolist() == [0, 0, 0, 0]   # captured, not run
    for _ in range(4):
        g.replay()
    torch.cuda.synchronize()
    a, b = eager.result(), graphed.result()
    for key in a:
        assert np.array_equal(a[key], b[key]), key
    assert a["n_hills"].tolist() == [4, 4, 4, 8]


def test_bias_is_three_kernel_launches_whatever_the_batch():
    """The launch sequence of one m3g_meta_bias captured (not executed) on a side stream: three kernel nodes and nothing else."""
    from torch_m3gnet.metadynamics import bias_forces

    hip = C.CDLL("libamdhip64.so")
    hip.hipGraphGetNodes.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    hip.hipGraphNodeGetType.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    for kinds, slots, groups, hills in ((("distance",), (0,), (1,), 0), (("coordination", "projection"), ALL, mc.GROUPS, 1000)):
        batch = Batch(kinds, slots=slots, groups=groups, max_hills=hills + 4)
        if hills:
            batch.state.set_hills(*starting_hills(kinds, hills))
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        graph, n = C.c_void_p(), C.c_size_t()
        with torch.cuda.stream(stream):
            assert hip.hipStreamBeginCapture(C.c_void_p(stream.cuda_stream), 2) == 0   # relaxed mode: this thread's other calls go on
            try:
                bias_forces(batch.state, batch.pos, batch.f, deposit=True)
            finally:
                assert hip.hipStreamEndCapture(C.c_void_p(stream.cuda_stream), C.byref(graph)) == 0
        assert hip.hipGraphGetNodes(graph, None, C.byref(n)) == 0
        assert n.value == 3, n.value
        nodes = (C.c_void_p * 3)()
        assert hip.hipGraphGetNodes(graph, nodes, C.byref(n)) == 0
        for node in nodes:
            kind = C.c_int(-1)
            assert hip.hipGraphNodeGetType(C.c_void_p(node), C.byref(kind)) == 0
            assert kind.value == 0   # hipGraphNodeTypeKernel
        hip.hipGraphDestroy(graph)
        assert batch.state.read()["n_hills"].tolist() == [hills] * len(groups)   # captured, not run


@pytest.mark.parametrize("name,change,reason", mc.REFUSALS, ids=[r[0] for r in mc.REFUSALS])
def test_init_refuses_on_a_real_state_and_leaves_it_untouched(name, change, reason):
    from torch_m3gnet import _lib

    lib = _lib.load_library()
    state = torch.full((1 << 16,), 0x5A, dtype=torch.uint8, device=DEV)
    args = mc.init_arguments()
    change(args)
    assert mc.call_init(lib, _lib, args, state.data_ptr(), state.numel()) == _lib.M3G_ERR_VALUE, name
    assert reason in lib.m3g_last_error(), (name, lib.m3g_last_error())
    torch.cuda.synchronize()
    assert bool((state == 0x5A).all())
    if name == "unknown kind":   # (once) the arguments are valid as they stand, and a short buffer is a size error
        good = mc.init_arguments()
        assert mc.call_init(lib, _lib, good, state.data_ptr(), state.numel()) == _lib.M3G_OK, lib.m3g_last_error()
        assert mc.call_init(lib, _lib, good, state.data_ptr(), 64) == _lib.M3G_ERR_SIZE
