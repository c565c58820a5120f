"""CPU checks of batched atom-swap Monte Carlo: the restatement (tests/mc_reference.py, the yardstick of the GPU tests) samples the
canonical distribution of small rings exactly enumerated and keeps its books, the GPU cases are decided far from a tie, and the C ABI /
SwapMonteCarlo refuse bad arguments before touching a device."""
import ctypes as C
import itertools
import math
import re
from pathlib import Path

import numpy as np
import pytest

import mc_cases as mcc
import mc_reference as mcr

ROOT = Path(__file__).resolve().parent.parent
N_TRIALS, N_BLOCKS = 200000, 100


def ring_energy(t, eps) -> float:
    return sum(eps[t[k]][t[(k + 1) % len(t)]] for k in range(len(t)))


def exact_moments(species, eps, T):
    """Mean and variance of E over all distinct arrangements of `species` on the ring, Boltzmann-weighted; and their number."""
    states = sorted(set(itertools.permutations(species)))
    e = np.array([ring_energy(s, eps) for s in states])
    w = np.exp(-(e - e.min()) / (mcr.KB * T))
    w /= w.sum()
    mean = float((w * e).sum())
    return mean, float((w * (e - mean) ** 2).sum()), len(states)


# (species on the ring, bond energies eV (symmetric), temperature K, Philox seed, number of distinct arrangements)
RINGS = [
    ([0] * 4 + [1] * 4, {(0, 0): 0.0, (1, 1): 0.0, (0, 1): 0.03}, 400.0, 2 ** 63 + 1, 70),
    ([0] * 2 + [1] * 3 + [2] * 4, {(0, 0): 0.0, (1, 1): 0.01, (2, 2): 0.0, (0, 1): 0.05, (0, 2): 0.02, (1, 2): 0.04}, 500.0, 17, 1260),
    ([0] * 1 + [1] * 2 + [2] * 6, {(0, 0): 0.0, (1, 1): 0.05, (2, 2): 0.01, (0, 1): 0.01, (0, 2): 0.04, (1, 2): 0.02}, 300.0, 2 ** 64 - 9, 252),
]


@pytest.mark.parametrize("species,bonds,T,seed,n_states", RINGS)
def test_restatement_samples_the_canonical_distribution_of_a_ring(species, bonds, T, seed, n_states):
    """Swap chains on rings of 8-9 sites with a nearest-neighbour pair energy: the chain mean of E over 200,000 trials lies within 4
    standard errors (from 100 block means) of the mean over all arrangements.  Unequal compositions: the proposal must be symmetric
    although the second pick depends on the first."""
    k = max(species) + 1
    eps = [[bonds[min(a, b), max(a, b)] for b in range(k)] for a in range(k)]
    mean, var, n = exact_moments(species, eps, T)
    assert n == n_states
    start = list(np.random.default_rng(3).permutation(species))
    mc = mcr.SwapReference(start, T, seed)
    e = ring_energy(mc.types, eps)
    trace = np.empty(N_TRIALS)
    for a in range(N_TRIALS):
        assert mc.propose(e) is not None
        _, e = mc.decide(ring_energy(mc.types, eps), e)
        trace[a] = e
    assert sorted(mc.types) == sorted(species) and e == pytest.approx(ring_energy(mc.types, eps), abs=1e-15)
    assert mc.attempts == mc.count == N_TRIALS and mc.nonfinite == 0
    assert mc.mean == pytest.approx(trace.mean(), rel=1e-12) and mc.m2 == pytest.approx(((trace - trace.mean()) ** 2).sum(), rel=1e-9)
    blocks = trace.reshape(N_BLOCKS, -1)
    se = blocks.mean(1).std(ddof=1) / math.sqrt(N_BLOCKS)
    dev = (trace.mean() - mean) / se
    sq = ((blocks - mean) ** 2).mean(1)
    dev_var = (sq.mean() - var) / (sq.std(ddof=1) / math.sqrt(N_BLOCKS))
    acceptance = mc.accepts / mc.attempts
    print(f"{n} arrangements: <E> exact {mean:.6f} chain {trace.mean():.6f} ({dev:+.2f} standard errors); var exact {var:.3e} "
          f"chain {sq.mean():.3e} ({dev_var:+.2f}); acceptance {acceptance:.3f}")
    assert abs(dev) < 4.0, (dev, mean, trace.mean(), se)
    assert abs(dev_var) < 4.0, (dev_var, var, sq.mean())
    assert 0.1 < acceptance < 0.9


# ---- bookkeeping -----------------------------------------------------------------------------------------------------------------------
def test_restatement_keeps_its_books():
    z, T, seed, _ = mcc.STRUCTURES[3]
    active = mcc.mask(3)
    ref = mcc.reference(3, 60)
    mc = ref["mc"]
    assert mc.counter == 60 and mc.attempts == 60 and 0 < mc.accepts < 60 and mc.count == 60
    assert sorted(mc.types) == sorted(z.tolist())                                  # the multiset of species
    assert (ref["types"][:, ~active] == z[~active][None]).all()                    # inactive rows are never touched
    assert (ref["types"] != z[None]).any()
    hist = mc.history_array(60, mcc.UNTOUCHED)
    assert active[hist[:, 0]].all() and active[hist[:, 1]].all() and (hist[:, 0] != hist[:, 1]).all()
    assert list(hist[:, 2]) == ref["verdicts"] and hist[:, 2].sum() == mc.accepts
    # every row of the history replays: the two rows held different species before, and an accepted swap exchanged them
    t = z.copy()
    for (i, j, ok), after in zip(hist, ref["types"]):
        assert t[i] != t[j]
        if ok:
            t[i], t[j] = t[j], t[i]
        assert (t == after).all()


def test_restatement_skips_what_the_semantics_say():
    # one species, or one active row: NO_PAIR, never attempted, the counter still advances
    for g in (6, 7):
        z, T, seed, _ = mcc.STRUCTURES[g]
        mc = mcr.SwapReference(z, T, seed, mcc.mask(g))
        assert mc.flags == (mcr.NO_PAIR if g == 7 else 0)
        for a in range(5):
            assert mc.propose(-1.0) is None and mc.decide(-2.0, -1.0) == (None, -1.0)
        assert mc.flags == mcr.NO_PAIR and mc.counter == 5 and mc.attempts == 0 and mc.types == z.tolist()
        assert (mc.history_array(6, mcc.UNTOUCHED) == [[-1] * 3] * 5 + [[mcc.UNTOUCHED] * 3]).all()
    z, T, seed, _ = mcc.STRUCTURES[2]
    mc = mcr.SwapReference(z, T, seed)
    calls = skipped = 0
    # a current energy that is not finite: not attempted
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert mc.propose(bad) is None and mc.decide(-1.0, bad)[0] is None
        calls, skipped = calls + 1, skipped + 1
    assert mc.types == z.tolist() and mc.flags == 0
    # a trial energy that is not finite is rejected explicitly -- -inf too, which dE <= 0 would accept -- and restored
    for bad in (float("nan"), float("inf"), -float("inf")):
        i, j = mc.propose(-1.0)
        assert mc.types != z.tolist() and mc.flags == mcr.PENDING
        assert mc.decide(bad, -1.0) == (0, -1.0) and mc.types == z.tolist() and mc.flags == 0
        calls += 1
    assert mc.nonfinite == 3 and mc.accepts == 0 and mc.mean == -1.0 and mc.m2 == 0.0
    # dynamics flags: STARTED or ERROR are not attempted
    import md_reference as mr

    for fl in (mr.STARTED, mr.ERROR, mr.STARTED | mr.ERROR):
        assert mc.propose(-1.0, fl) is None
        mc.decide(-1.0, -1.0)
        calls, skipped = calls + 1, skipped + 1
    # a proposal while one is pending: ERR_ORDER, nothing else changes; a decide with nothing pending changes nothing
    pair = mc.propose(-1.0)
    before = (list(mc.types), mc.pair, mc.u2)
    assert mc.propose(-1.0) is None and mc.flags == mcr.PENDING | mcr.ERR_ORDER and (list(mc.types), mc.pair, mc.u2) == before
    assert mc.decide(-2.0, -1.0) == (1, -2.0) and mc.flags == mcr.ERR_ORDER
    calls, skipped = calls + 2, skipped + 1
    snapshot = (list(mc.types), mc.attempts, mc.count, mc.mean, dict(mc.history))
    assert mc.decide(-3.0, -2.0) == (None, -2.0) and (list(mc.types), mc.attempts, mc.count, mc.mean, dict(mc.history)) == snapshot
    assert mc.counter == calls and mc.attempts + skipped == calls
    assert mc.history[calls - 1] == (pair[0], pair[1], 1) and calls - 2 not in mc.history   # the call that found one pending wrote no row


def test_the_gpu_cases_are_decided_far_from_a_tie():
    """The inputs of tests/test_gpu_mc.py in the restatement: every uphill trial has |log u - x| > 1e-9, so a device exp that differs
    in its last bits decides the same; both verdicts occur in every structure that swaps."""
    for g in range(len(mcc.STRUCTURES)):
        ref = mcc.reference(g, with_forces=False)
        mc = ref["mc"]
        if g in (6, 7):
            assert mc.attempts == 0 and mc.flags == mcr.NO_PAIR
            continue
        assert mc.attempts == mcc.ROUNDS and 0.1 * mcc.ROUNDS < mc.accepts < 0.9 * mcc.ROUNDS, (g, mc.accepts)
        assert mc.margins and min(abs(m) for m in mc.margins) > 1e-9 and max(abs(m) for m in mc.margins) < 50.0
    for ops in (mcc.schedule(), mcc.started_schedule()):
        for g in mcc.DYN_STRUCTURES:
            ref = mcc.dyn_reference(g, ops)
            assert min(abs(m) for m in ref["mc"].margins) > 1e-9
            for k0, k1, k2 in ref["ke"]:   # the terms of the kinetic energy trade rows: the sum changes by its rounding at most
                assert abs(k1 - k0) <= 1e-13 * k0 and abs(k2 - k0) <= 1e-13 * k0
    assert 0 < sum(mcc.dyn_reference(g, mcc.schedule())["mc"].accepts for g in mcc.DYN_STRUCTURES) < 3 * mcc.DYN_ROUNDS


def test_short_range_order_of_ordered_and_segregated_cells():
    from torch_m3gnet.monte_carlo import short_range_order

    # rock salt: every first neighbour is of the other species -> alpha_ab = 1 - 1 / c_b = -1, alpha_aa = 1
    a = 4.0
    grid = np.stack(np.meshgrid(*[np.arange(2)] * 3, indexing="ij"), -1).reshape(-1, 3)
    z = np.where(grid.sum(1) % 2 == 0, 11, 17)
    sro = short_range_order(np.eye(3) * a, grid * a / 2, z, 0.5 * a * 1.1)
    assert sro[11, 17] == pytest.approx(-1.0) and sro[17, 11] == pytest.approx(-1.0) and sro[11, 11] == pytest.approx(1.0)
    # the second shell alone holds like atoms only, so the two shells together: 6 unlike + 12 like of 18
    sro = short_range_order(np.eye(3) * a, grid * a / 2, z, 0.5 * a * 1.5)
    assert sro[11, 17] == pytest.approx(1.0 - (6 / 18) / 0.5) and sro[11, 11] == pytest.approx(1.0 - (12 / 18) / 0.5)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            short_range_order(np.eye(3) * a, grid * a / 2, z, bad)


# ---- argument checks (no device needed: refused before any HIP call) ------------------------------------------------------------------
def _lib():
    from torch_m3gnet import _lib

    return _lib, _lib.load_library()


def _init(lib, N, S, offsets, temps, seeds="default", active="default", state=C.c_void_p(256), nbytes=1 << 30):
    offs = None if offsets is None else np.array(offsets, dtype=np.int64)
    t = None if temps is None else np.array(temps, dtype=np.float64)
    sd = np.arange(S, dtype=np.uint64) if isinstance(seeds, str) else seeds
    act = np.ones(max(N, 1), dtype=np.uint8) if isinstance(active, str) else active
    return lib.m3g_mc_init(N, S, None if offs is None else offs.ctypes.data, None if t is None else t.ctypes.data,
                           None if sd is None else sd.ctypes.data, None if act is None else act.ctypes.data, state, nbytes, None)


def test_header_prototypes_are_exported_and_the_abi_version_stays():
    _l, lib = _lib()
    header = (ROOT / "include" / "m3gnet_hip.h").read_text()
    declared = set(re.findall(r"\b(m3g_mc_[a-z_]+)\s*\(", header))
    assert declared == {"m3g_mc_state_bytes", "m3g_mc_init", "m3g_mc_propose", "m3g_mc_decide", "m3g_mc_read"}
    for name in declared:
        assert hasattr(lib, name) and name in _l.SYMBOLS, name
    assert int(re.search(r"#define M3G_ABI_VERSION (\S+)", header).group(1)) == _l.ABI_VERSION == 11
    info = _l.M3GInfo()
    assert lib.m3g_get_info(C.byref(info)) == 0 and info.abi_version == 11
    value = lambda name: int(re.search(rf"#define {name} (\S+)", header).group(1))
    assert (value("M3G_MC_NO_PAIR"), value("M3G_MC_PENDING"), value("M3G_MC_ERR_ORDER")) == (_l.MC_NO_PAIR, _l.MC_PENDING, _l.MC_ERR_ORDER)
    assert (_l.MC_NO_PAIR, _l.MC_PENDING, _l.MC_ERR_ORDER) == (mcr.NO_PAIR, mcr.PENDING, mcr.ERR_ORDER)


def test_c_abi_state_bytes_grow_with_atoms_and_structures():
    _l, lib = _lib()
    sizes = {}
    for N, S in [(2, 1), (10000, 1), (10000, 100), (20000, 100)]:
        n = C.c_size_t()
        assert lib.m3g_mc_state_bytes(N, S, C.byref(n)) == _l.M3G_OK
        sizes[N, S] = n.value
    assert sizes[2, 1] < sizes[10000, 1] < sizes[10000, 100] < sizes[20000, 100]
    n = C.c_size_t()
    for N, S in [(0, 1), (4, 0), (3, 4), (-1, 1)]:
        assert lib.m3g_mc_state_bytes(N, S, C.byref(n)) == _l.M3G_ERR_VALUE
    assert lib.m3g_mc_state_bytes(4, 1, None) == _l.M3G_ERR_VALUE


@pytest.mark.parametrize("offsets", [[0, 3, 2, 6], [0, 2, 2, 6], [1, 3, 5, 6], [0, 2, 4, 5], [0, 2, 4, 7]])
def test_c_abi_refuses_bad_offsets(offsets):
    _l, lib = _lib()
    assert _init(lib, 6, 3, offsets, [300.0] * 3) == _l.M3G_ERR_VALUE
    assert b"m3g_mc_init: offsets" in lib.m3g_last_error()


@pytest.mark.parametrize("temps", [[0.0, 300.0], [-5.0, 300.0], [300.0, float("inf")], [float("nan"), 300.0]])
def test_c_abi_refuses_bad_temperatures(temps):
    _l, lib = _lib()
    assert _init(lib, 6, 2, [0, 3, 6], temps) == _l.M3G_ERR_VALUE
    assert b"temperature" in lib.m3g_last_error()


def test_c_abi_refuses_null_pointers_short_buffers_and_lone_force_buffers():
    _l, lib = _lib()
    d = C.c_void_p(256)
    offs, temps = [0, 3, 6], [300.0, 400.0]
    assert _init(lib, 6, 2, None, temps) == _l.M3G_ERR_VALUE
    assert _init(lib, 6, 2, offs, None) == _l.M3G_ERR_VALUE
    assert _init(lib, 6, 2, offs, temps, seeds=None) == _l.M3G_ERR_VALUE
    assert _init(lib, 6, 2, offs, temps, active=None) == _l.M3G_ERR_VALUE
    assert _init(lib, 6, 2, offs, temps, state=None) == _l.M3G_ERR_VALUE
    assert _init(lib, 1, 2, offs, temps) == _l.M3G_ERR_VALUE   # fewer atoms than structures
    mc, dyn = C.c_size_t(), C.c_size_t()
    assert lib.m3g_mc_state_bytes(6, 2, C.byref(mc)) == _l.M3G_OK and lib.m3g_dyn_state_bytes(6, 2, C.byref(dyn)) == _l.M3G_OK
    assert _init(lib, 6, 2, offs, temps, nbytes=mc.value - 1) == _l.M3G_ERR_SIZE
    big = 1 << 30
    pr = lib.m3g_mc_propose
    assert pr(6, 2, None, big, d, None, 0, d, None) == _l.M3G_ERR_VALUE
    assert pr(6, 2, d, big, None, None, 0, d, None) == _l.M3G_ERR_VALUE
    assert pr(6, 2, d, big, d, None, 0, None, None) == _l.M3G_ERR_VALUE
    assert pr(1, 2, d, big, d, None, 0, d, None) == _l.M3G_ERR_VALUE
    assert pr(6, 2, d, mc.value - 1, d, None, 0, d, None) == _l.M3G_ERR_SIZE
    assert pr(6, 2, d, big, d, d, dyn.value - 1, d, None) == _l.M3G_ERR_SIZE
    assert b"dynamics state" in lib.m3g_last_error()
    de = lib.m3g_mc_decide
    ok = dict(state=d, types=d, trial=d, tf=None, ts=None, e=d, f=None, s=None, hist=None, rows=0, dyn=None, dyn_bytes=0, nbytes=big)

    def decide(**kw):
        a = dict(ok, **kw)
        return de(6, 2, a["state"], a["nbytes"], a["types"], a["dyn"], a["dyn_bytes"], a["trial"], a["tf"], a["ts"], a["e"], a["f"], a["s"],
                  a["hist"], a["rows"], None)

    for name in ("state", "types", "trial", "e"):
        assert decide(**{name: None}) == _l.M3G_ERR_VALUE, name
    assert decide(hist=d, rows=-1) == _l.M3G_ERR_VALUE
    for lone in (dict(tf=d), dict(f=d), dict(ts=d), dict(s=d), dict(tf=d, f=d, ts=d)):   # forces or stresses without their partner
        assert decide(**lone) == _l.M3G_ERR_VALUE, lone
        assert b"together" in lib.m3g_last_error()
    assert decide(nbytes=mc.value - 1) == _l.M3G_ERR_SIZE
    assert decide(dyn=d, dyn_bytes=dyn.value - 1) == _l.M3G_ERR_SIZE
    none = [None] * 9
    assert lib.m3g_mc_read(6, 2, None, big, *none, None) == _l.M3G_ERR_VALUE
    assert lib.m3g_mc_read(1, 2, d, big, *none, None) == _l.M3G_ERR_VALUE
    assert lib.m3g_mc_read(6, 2, d, mc.value - 1, *none, None) == _l.M3G_ERR_SIZE


def test_swap_monte_carlo_argument_validation():
    from torch_m3gnet.model.build import build_model
    from torch_m3gnet.monte_carlo import SwapMonteCarlo

    model = build_model(5.0, 4.0, 3, 3, 95, 16, 1)
    mc = SwapMonteCarlo(model, 300.0)
    assert mc.md_steps == 0 and mc.structure_batches is False and mc.friction == 0.01 and mc.species is None
    assert SwapMonteCarlo(model, [300.0, 400.0], species=[29, 79], md_steps=5, structure_batches=True).md_steps == 5
    for bad in (0.0, -1.0, float("inf"), float("nan"), [300.0, 0.0], [[300.0]], []):
        with pytest.raises(ValueError):
            SwapMonteCarlo(model, bad)
    for kw in (dict(md_steps=-1), dict(md_steps=2.5), dict(timestep=0.0), dict(friction=-0.1), dict(skin=0.0), dict(structure_batches=1),
               dict(species=[]), dict(species=[0, 29]), dict(species=[29.5])):
        with pytest.raises(ValueError):
            SwapMonteCarlo(model, 300.0, **kw)
    with pytest.raises(TypeError):
        SwapMonteCarlo(model.model, 300.0)
    # counted in run() before anything touches the device
    lat, pos, z = np.eye(3) * 5.0, np.zeros((2, 3)) + [[0.0], [2.5]], np.array([29, 79])
    with pytest.raises(ValueError, match="one value or one per structure"):
        SwapMonteCarlo(model, [300.0, 400.0]).run([lat] * 3, [pos] * 3, [z] * 3, 5)
    with pytest.raises(ValueError, match="not both"):
        SwapMonteCarlo(model, 300.0, species=[29]).run([lat], [pos], [z], 5, sites=[[True, True]])
    with pytest.raises(ValueError, match="sites"):
        SwapMonteCarlo(model, 300.0).run([lat], [pos], [z], 5, sites=[[True]])
    with pytest.raises(ValueError, match="sites"):
        SwapMonteCarlo(model, 300.0).run([lat] * 2, [pos] * 2, [z] * 2, 5, sites=[[True, True]])
    for trials in (-1, 2.5):
        with pytest.raises(ValueError):
            SwapMonteCarlo(model, 300.0).run([lat], [pos], [z], trials)
