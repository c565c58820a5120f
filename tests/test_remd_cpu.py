"""CPU checks of batched replica exchange: the restatement (tests/remd_reference.py, the yardstick of the GPU tests) reproduces the
analytic acceptance of a harmonic ladder and keeps its books, and the C ABI / ReplicaExchange refuse bad arguments before touching a
device."""
import ctypes as C
import math

import numpy as np
import pytest

import remd_reference as rr

N_ATTEMPTS = 20000


def _gamma_pdf(x, shape):
    return np.exp((shape - 1.0) * np.log(x) - x - math.lgamma(shape))


def analytic_acceptance(t_lo, t_hi, dof, n=3000, upper=60.0):
    """E[min(1, exp Delta)] of the pair (T_lo, T_hi) whose holders' energies are Gamma(dof / 2, KB T): midpoint rule over the two
    densities in units of KB T each (x = E_lo / KB T_lo, y = E_hi / KB T_hi), Delta = (1 - T_lo/T_hi) x - (T_hi/T_lo - 1) y.  The
    integrand has a kink on Delta = 0 only, so the rule's error is O(h^2) ~ 1e-4 of the result, far below the sampling margin."""
    h = upper / n
    x = (np.arange(n) + 0.5) * h
    w = _gamma_pdf(x, dof / 2.0) * h
    delta = (1.0 - t_lo / t_hi) * x[:, None] - (t_hi / t_lo - 1.0) * x[None, :]
    return float(w @ np.minimum(1.0, np.exp(np.minimum(delta, 0.0))) @ w), float(w.sum())


@pytest.mark.parametrize("temps,dof,seed", [([300.0, 380.0, 500.0, 700.0], 6, 11), ([100.0, 150.0, 180.0, 400.0, 500.0], 10, 2 ** 63 + 7),
                                            ([250.0, 600.0], 4, 5)])
def test_restatement_reproduces_the_analytic_acceptance_of_a_harmonic_ladder(temps, dof, seed):
    """Exchange-only chains: between attempts the holder of T_k draws a fresh E from Gamma(dof / 2, KB T_k), the potential energy of
    `dof` harmonic degrees of freedom, so every attempt of pair k is an independent Bernoulli trial of the analytic probability."""
    R = len(temps)
    lad = rr.LadderReference(temps, seed)
    g = np.random.default_rng([seed % 2 ** 32, 1]).standard_gamma(dof / 2.0, size=(N_ATTEMPTS, R))
    scales = set()
    for a in range(N_ATTEMPTS):
        E = [0.0] * R
        for k in range(R):
            E[lad.holder[k]] = g[a, k] * rr.KB * temps[k]
        scales.update(lad.exchange(E))
    hist = np.array(lad.history)
    assert hist.shape == (N_ATTEMPTS + 1, R) and lad.n_attempts == N_ATTEMPTS
    assert (np.sort(hist, axis=1) == np.arange(R)[None]).all()                  # every row a permutation
    assert lad.count == [N_ATTEMPTS] * R                                         # every index sampled at every attempt
    assert sorted(lad.holder[k] for k in range(R)) == list(range(R)) and all(lad.held[lad.holder[k]] == k for k in range(R))
    assert lad.round_trips == rr.round_trips_of(hist)
    if R > 2:
        assert sum(lad.round_trips) > 0
    for k in range(R - 1):
        n = lad.attempts[k]
        assert n == (N_ATTEMPTS + 1 - (k & 1)) // 2                              # the parity schedule
        p, norm = analytic_acceptance(temps[k], temps[k + 1], dof)
        assert abs(norm - 1.0) < 1e-4   # (the rule integrates the density itself to h^2 / 24 at worst)
        measured = lad.accepts[k] / n
        margin = 4.0 * math.sqrt(p * (1.0 - p) / n)
        print(f"pair {k}: measured {measured:.4f}  analytic {p:.4f}  margin {margin:.4f}")
        assert abs(measured - p) < margin, (k, measured, p, margin)
        assert math.sqrt(temps[k + 1] / temps[k]) in scales and math.sqrt(temps[k] / temps[k + 1]) in scales
    # the energy statistics of index k are those of Gamma(dof / 2, KB T_k): mean (dof / 2) KB T, variance (dof / 2) (KB T)^2
    for k in range(R):
        kt = rr.KB * temps[k]
        sample = g[:, k] * kt
        assert lad.mean[k] == pytest.approx(sample.mean(), rel=1e-12) and lad.m2[k] == pytest.approx(((sample - sample.mean()) ** 2).sum(), rel=1e-10)
        assert lad.mean[k] == pytest.approx(0.5 * dof * kt, rel=0.05)


def test_restatement_skips_pairs_that_are_started_failed_or_not_finite():
    import md_reference as mr

    temps = [300.0, 400.0, 500.0, 600.0]
    lad = rr.LadderReference(temps, 3)
    E = [0.0, -1.0, -2.0, -3.0]   # every Delta > 0: all attempted pairs accept
    assert lad.exchange(E, [mr.STARTED] * 4) == [1.0] * 4 and lad.attempts == [0, 0, 0] and lad.count == [1] * 4 and lad.n_attempts == 1
    assert lad.exchange(E, [0, 0, mr.ERROR, 0]) == [1.0] * 4 and lad.attempts == [0, 0, 0] and lad.count == [2, 2, 1, 2]   # odd: pair (1, 2)
    scale = lad.exchange([0.0, float("nan"), -2.0, -3.0])   # even: (0, 1) has the NaN, (2, 3) goes on
    assert scale[:2] == [1.0, 1.0] and scale[2] == math.sqrt(600.0 / 500.0) and scale[3] == math.sqrt(500.0 / 600.0)
    assert lad.attempts == [0, 0, 1] and lad.accepts == [0, 0, 1] and lad.held == [0, 1, 3, 2] and lad.count == [3, 2, 2, 3]
    assert lad.history[-1] == [0, 1, 3, 2] and lad.margins == []


def test_the_gpu_cases_are_decided_far_from_a_tie():
    """The inputs of tests/test_gpu_remd.py in the restatement: every attempted pair with Delta < 0 has |log u - Delta| > 1e-9, so a
    device exp that differs in its last bits decides the same; both verdicts occur, and Delta is of order 1."""
    import remd_cases as rc

    runs = [(rc.schedule(), {}), (rc.started_schedule(), {}), (rc.schedule(), dict(nan_force={(2, 6): 5})),
            (rc.schedule(), dict(nan_energy={(2, 4): 2, (1, 5): 0}))]
    for ops, kw in runs:
        for g in range(len(rc.LADDERS)):
            lad = rc.reference(g, ops, **kw)["ladder"]
            assert lad.margins and min(abs(m) for m in lad.margins) > 1e-9, (g, kw)
            assert max(abs(m) for m in lad.margins) < 50.0
            assert (np.sort(np.array(lad.history), axis=1) == np.arange(lad.R)[None]).all()
            assert lad.round_trips == rr.round_trips_of(lad.history)
    lads = [rc.reference(g, rc.schedule())["ladder"] for g in range(3)]
    assert 0 < sum(sum(lad.accepts) for lad in lads) < sum(sum(lad.attempts) for lad in lads)


# ---- argument checks (no device needed: refused before any HIP call) ------------------------------------------------------------
def _lib():
    from torch_m3gnet import _lib

    return _lib, _lib.load_library()


def _init(lib, S, G, offsets, temps, seeds=None, state=C.c_void_p(256), nbytes=1 << 30):
    offs = None if offsets is None else np.array(offsets, dtype=np.int64)
    t = None if temps is None else np.array(temps, dtype=np.float64)
    sd = np.arange(G, dtype=np.uint64) if seeds is None else seeds
    return lib.m3g_remd_init(S, G, None if offs is None else offs.ctypes.data, None if t is None else t.ctypes.data,
                             sd.ctypes.data if isinstance(sd, np.ndarray) else sd, state, nbytes, None)


def test_c_abi_state_bytes_grow_with_replicas_and_ladders():
    _l, lib = _lib()
    sizes = {}
    for S, G in [(4, 1), (4, 2), (4000, 1), (4000, 1000), (8000, 1000)]:
        n = C.c_size_t()
        assert lib.m3g_remd_state_bytes(S, G, C.byref(n)) == _l.M3G_OK
        sizes[S, G] = n.value
    assert sizes[4000, 1] > sizes[4, 1] and sizes[8000, 1000] > sizes[4000, 1000] > sizes[4000, 1] and sizes[4, 2] >= sizes[4, 1]
    assert 76 * 4000 <= sizes[4000, 1] < 76 * 4000 + 16 * 256   # 76 bytes per replica, 14 regions rounded up to 256 bytes
    n = C.c_size_t()
    for S, G in [(4, 0), (3, 2), (1, 1), (0, 1), (4, -1)]:   # no ladder, or not two replicas per ladder
        assert lib.m3g_remd_state_bytes(S, G, C.byref(n)) == _l.M3G_ERR_VALUE
    assert lib.m3g_remd_state_bytes(4, 1, None) == _l.M3G_ERR_VALUE


@pytest.mark.parametrize("offsets", [[0, 3, 2, 6], [0, 2, 2, 6], [1, 3, 5, 6], [0, 2, 4, 5], [0, 2, 4, 7]])
def test_c_abi_refuses_bad_ladder_offsets(offsets):
    _l, lib = _lib()
    assert _init(lib, 6, 3, offsets, [100.0, 200.0] * 3) == _l.M3G_ERR_VALUE
    assert b"ladder_offsets" in lib.m3g_last_error()


def test_c_abi_refuses_a_ladder_of_one_replica():
    _l, lib = _lib()
    assert _init(lib, 5, 2, [0, 1, 5], [100.0, 100.0, 200.0, 300.0, 400.0]) == _l.M3G_ERR_VALUE
    assert b"fewer than 2" in lib.m3g_last_error()
    assert _init(lib, 5, 2, [0, 4, 5], [100.0, 200.0, 300.0, 400.0, 100.0]) == _l.M3G_ERR_VALUE


@pytest.mark.parametrize("temps", [[100.0, 100.0, 300.0, 50.0, 60.0], [100.0, 90.0, 300.0, 50.0, 60.0], [0.0, 90.0, 300.0, 50.0, 60.0],
                                   [-5.0, 90.0, 300.0, 50.0, 60.0], [100.0, 200.0, float("inf"), 50.0, 60.0],
                                   [100.0, float("nan"), 300.0, 50.0, 60.0], [100.0, 200.0, 300.0, 60.0, 50.0],
                                   [100.0, 200.0, 300.0, 60.0, 60.0]])
def test_c_abi_refuses_bad_temperatures(temps):
    _l, lib = _lib()
    assert _init(lib, 5, 2, [0, 3, 5], temps) == _l.M3G_ERR_VALUE
    assert b"temperatures" in lib.m3g_last_error()


def test_c_abi_refuses_null_pointers_and_short_buffers():
    _l, lib = _lib()
    dummy = C.c_void_p(256)
    offs, temps = [0, 3, 5], [100.0, 200.0, 300.0, 50.0, 60.0]
    assert _init(lib, 5, 2, None, temps) == _l.M3G_ERR_VALUE
    assert _init(lib, 5, 2, offs, None) == _l.M3G_ERR_VALUE
    assert _init(lib, 5, 2, offs, temps, seeds=C.c_void_p(None)) == _l.M3G_ERR_VALUE
    assert _init(lib, 5, 2, offs, temps, state=None) == _l.M3G_ERR_VALUE
    assert _init(lib, 5, 3, [0, 2, 4, 5], temps) == _l.M3G_ERR_VALUE   # S < 2 G
    remd, dyn = C.c_size_t(), C.c_size_t()
    assert lib.m3g_remd_state_bytes(5, 2, C.byref(remd)) == _l.M3G_OK and lib.m3g_dyn_state_bytes(40, 5, C.byref(dyn)) == _l.M3G_OK
    assert _init(lib, 5, 2, offs, temps, nbytes=remd.value - 1) == _l.M3G_ERR_SIZE
    big = 1 << 30
    ex = lib.m3g_remd_exchange
    assert ex(40, 5, 2, None, big, dummy, big, dummy, None, 0, None) == _l.M3G_ERR_VALUE
    assert ex(40, 5, 2, dummy, big, None, big, dummy, None, 0, None) == _l.M3G_ERR_VALUE
    assert ex(40, 5, 2, dummy, big, dummy, big, None, None, 0, None) == _l.M3G_ERR_VALUE
    assert ex(40, 5, 2, dummy, big, dummy, big, dummy, dummy, -1, None) == _l.M3G_ERR_VALUE
    assert ex(4, 5, 2, dummy, big, dummy, big, dummy, None, 0, None) == _l.M3G_ERR_VALUE    # fewer atoms than replicas
    assert ex(40, 5, 3, dummy, big, dummy, big, dummy, None, 0, None) == _l.M3G_ERR_VALUE   # S < 2 G
    assert ex(40, 5, 2, dummy, remd.value - 1, dummy, big, dummy, None, 0, None) == _l.M3G_ERR_SIZE
    assert ex(40, 5, 2, dummy, big, dummy, dyn.value - 1, dummy, None, 0, None) == _l.M3G_ERR_SIZE
    assert b"dynamics state" in lib.m3g_last_error()
    none = [None] * 9
    assert lib.m3g_remd_read(5, 2, None, big, *none, None) == _l.M3G_ERR_VALUE
    assert lib.m3g_remd_read(5, 3, dummy, big, *none, None) == _l.M3G_ERR_VALUE
    assert lib.m3g_remd_read(5, 2, dummy, remd.value - 1, *none, None) == _l.M3G_ERR_SIZE
    at = C.c_size_t()
    assert lib.m3g_remd_target_view(40, 5, None) == _l.M3G_ERR_VALUE and lib.m3g_remd_target_view(4, 5, C.byref(at)) == _l.M3G_ERR_VALUE
    assert lib.m3g_remd_target_view(40, 5, C.byref(at)) == _l.M3G_OK and 0 < at.value < dyn.value and at.value % 256 == 0


def test_replica_exchange_argument_validation():
    from torch_m3gnet.model.build import build_model
    from torch_m3gnet.replica_exchange import ReplicaExchange

    model = build_model(5.0, 4.0, 3, 3, 95, 16, 1)
    rx = ReplicaExchange(model, [300.0, 400.0, 500.0])
    assert rx.shared and rx.exchange_interval == 100 and rx.friction == 0.01
    assert not ReplicaExchange(model, [[300.0, 400.0], [100.0, 200.0, 300.0]]).shared
    for bad in ([300.0], [], [300.0, 300.0], [400.0, 300.0], [0.0, 300.0], [-1.0, 300.0], [300.0, float("inf")], [300.0, float("nan")],
                [[300.0, 400.0], [300.0]], [[300.0, 400.0], [500.0, 400.0]], 300.0):
        with pytest.raises(ValueError):
            ReplicaExchange(model, bad)
    for interval in (0, -3, 2.5):
        with pytest.raises(ValueError):
            ReplicaExchange(model, [300.0, 400.0], exchange_interval=interval)
    with pytest.raises(ValueError):
        ReplicaExchange(model, [300.0, 400.0], timestep=0.0)
    with pytest.raises(ValueError):
        ReplicaExchange(model, [300.0, 400.0], friction=-0.1)
    with pytest.raises(TypeError):
        ReplicaExchange(model.model, [300.0, 400.0])
    # one ladder per structure, counted in run() before anything touches the device
    lat, pos, z = np.eye(3) * 5.0, np.zeros((1, 3)), np.array([29])
    with pytest.raises(ValueError, match="one ladder or one per structure"):
        ReplicaExchange(model, [[300.0, 400.0], [100.0, 200.0]]).run([lat] * 3, [pos] * 3, [z] * 3, 5)
