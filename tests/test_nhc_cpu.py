"""CPU checks of the Nose-Hoover chain NVT and MTK NPT ensembles: the numpy restatement (tests/nhc_reference.py, the yardstick of
tests/test_gpu_nhc.py) held to physics on a smoothly truncated Lennard-Jones fcc cell of 32 atoms -- second-order drift of the
conserved quantity, time reversal, the mean pressure and the canonical temperature fluctuation of a long NPT run, chains of different
length and substeps -- and the C ABI / MolecularDynamics refusing bad arguments before touching a device."""
import ctypes as C
import itertools
import re
from pathlib import Path

import numpy as np
import pytest

import nhc_reference as nr

ROOT = Path(__file__).resolve().parent.parent
CU = 63.546
EPS, SIGMA, R_ON, RC = 0.4, 2.3, 2.9, 3.4   # eV, A; RC < half the box (2 a ~ 7.2 A) and between the first two fcc shells
FCC_BASE = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])
SHIFTS = np.array(list(itertools.product((-2, -1, 0, 1, 2), repeat=3)), dtype=np.float64)
A_START = 3.63


def fcc(a, n=2):
    grid = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1).reshape(-1, 1, 3)
    return (grid + FCC_BASE[None]).reshape(-1, 3) * a, np.eye(3) * n * a


SKIN = 0.8


class SmoothLJ:
    """Energy, forces and pair-virial stresses (Voigt, W / V) of LJ times the quintic switch S(t) = 1 - 10 t^3 + 15 t^4 - 6 t^5,
    t = (r - R_ON) / (RC - R_ON): the value and the first two derivatives vanish at RC, and are continuous at R_ON.  The pairs within
    RC + SKIN (with their image shifts, over unwrapped positions) are listed once and listed again when an atom has moved SKIN / 2
    in the scaled frame, so the list always holds every pair within RC."""

    def __init__(self):
        self.frac0 = None

    def _build(self, frac, lattice):
        rij = (frac[None, :, None, :] + SHIFTS[None, None, :, :] - frac[:, None, None, :]) @ lattice
        r = np.sqrt((rij * rij).sum(-1))
        self.i, self.j, s = np.nonzero((r > 1e-9) & (r < RC + SKIN))
        self.shift, self.frac0 = SHIFTS[s], frac.copy()

    def __call__(self, pos, lattice):
        assert np.diag(lattice).min() > max(2 * RC, RC + SKIN) and np.abs(lattice - np.diag(np.diag(lattice))).max() < 1e-6
        frac = np.linalg.solve(lattice.T, pos.T).T
        if self.frac0 is None or np.abs((frac - self.frac0) @ lattice).max() > 0.5 * SKIN / np.sqrt(3.0):
            self._build(frac, lattice)
        vec = (frac[self.j] + self.shift - frac[self.i]) @ lattice
        rs = np.sqrt((vec * vec).sum(-1))
        keep = rs < RC
        i, rs, vec = self.i[keep], rs[keep], vec[keep]
        sr6 = (SIGMA / rs) ** 6
        phi = 4 * EPS * (sr6 * sr6 - sr6)
        dphi = 4 * EPS * (-12 * sr6 * sr6 + 6 * sr6) / rs
        t = np.clip((rs - R_ON) / (RC - R_ON), 0.0, 1.0)
        sw = 1 - t ** 3 * (10 - 15 * t + 6 * t * t)
        dsw = -30 * t * t * (1 - t) ** 2 / (RC - R_ON)
        du = (dphi * sw + phi * dsw) / rs   # (d u / d r) / r
        e = 0.5 * (phi * sw).sum()
        f = np.stack([np.bincount(i, du * vec[:, k], len(pos)) for k in range(3)], axis=1)
        w = -0.5 * np.einsum("p,pa,pb->ab", du, vec, vec)
        vol = abs(np.linalg.det(lattice))
        return e, f, np.array([w[0, 0], w[1, 1], w[2, 2], w[1, 2], w[2, 0], w[0, 1]]) / vol


def smooth_lj(pos, lattice):
    return SmoothLJ()(pos, lattice)


def test_smooth_lj_forces_and_virial_are_derivatives():
    rng = np.random.default_rng(1)
    pos, lat = fcc(A_START)
    pos = pos + rng.normal(0, 0.05, pos.shape)
    e, f, s = smooth_lj(pos, lat)
    h = 1e-5
    for i, k in [(0, 0), (5, 1), (17, 2)]:
        dp = np.zeros_like(pos)
        dp[i, k] = h
        fd = -(smooth_lj(pos + dp, lat)[0] - smooth_lj(pos - dp, lat)[0]) / (2 * h)
        assert abs(fd - f[i, k]) < 1e-6 * max(1.0, abs(f[i, k]))
    fd = -(smooth_lj(pos * (1 + h), lat * (1 + h))[0] - smooth_lj(pos * (1 - h), lat * (1 - h))[0]) / (2 * h)
    assert abs(fd - s[:3].sum() * abs(np.linalg.det(lat))) < 1e-5 * max(1.0, abs(fd))


def _start(seed=3, temperature=300.0):
    from torch_m3gnet.dynamics import maxwell_boltzmann

    pos, lat = fcc(A_START)
    pos = pos + np.random.default_rng(seed).normal(0, 0.02, pos.shape)
    m = np.full(len(pos), CU)
    return pos, lat, m, maxwell_boltzmann(m, temperature, seed)


def _run(ref, n_steps, record=False):
    """n_steps steps (n_steps + 1 calls, the last finish_only): H = e_pot + KE + extended at every full step."""
    h, rows, pot = [], [], SmoothLJ()
    for k in range(n_steps + 1):
        e, f, s = pot(ref.pos, ref.lattice)
        ref.step(f, s, finish_only=(k == n_steps))
        h.append(e + ref.obs[0] + ref.obs[4])
        if record:
            rows.append(ref.obs.copy())
    return np.array(h), np.array(rows)


def _ref(ensemble, dt, **kw):
    pos, lat, m, v = _start()
    args = dict(temperature=300.0, dt=dt, taut=50.0, taup=300.0, pressure=2e-3)
    args.update(kw)
    return nr.NhcReference(pos, lat, m, v, ensemble, **args)


@pytest.mark.parametrize("ensemble", ["nvt_nose_hoover", "npt_mtk"])
def test_restatement_conserved_quantity_error_is_second_order(ensemble):
    drift = []
    for dt in (1.0, 2.0, 4.0):
        h, _ = _run(_ref(ensemble, dt), int(400 / dt))
        drift.append(np.abs(h - h[0]).max())
    print(f"{ensemble}: drift of H over 400 fs at dt = 1, 2, 4 fs: {drift}")
    assert drift[0] > 0
    assert 3.0 <= drift[1] / drift[0] <= 5.0 and 3.0 <= drift[2] / drift[1] <= 5.0, drift


@pytest.mark.parametrize("ensemble", ["nvt_nose_hoover", "npt_mtk"])
def test_restatement_is_time_reversible(ensemble):
    ref = _ref(ensemble, 2.0)
    pos0, lat0 = ref.pos.copy(), ref.lattice.copy()
    _run(ref, 100)
    assert np.abs(ref.pos - pos0).max() > 0.05 and ref.n_steps == 100
    if ensemble == "npt_mtk":
        assert np.abs(ref.lattice - lat0).max() > 1e-4
    ref.reverse()
    _run(ref, 100)
    assert np.abs(ref.pos - pos0).max() < 1e-9 and np.abs(ref.lattice - lat0).max() < 1e-9


def _block_standard_error(x, block):
    """Standard error of mean(x) from the means of consecutive blocks of `block` samples."""
    b = x[:len(x) // block * block].reshape(-1, block).mean(1)
    return b.std(ddof=1) / np.sqrt(len(b))


def test_restatement_long_npt_run_samples_pressure_and_canonical_temperature():
    """20,000 retained steps of 4 fs after 1,000 discarded, at P_ext = 2e-3 eV/A^3 (0.32 GPa).  Blocks of 250 steps (1 ps): several
    periods of the thermostat (taut = 50 fs) and of the barostat (taup = 300 fs), so block means are close to independent and the
    80 of them give the standard error of either mean.  Gates: |<P> - P_ext| < 4 standard errors; var(T) / <T>^2, the mean of
    x_i = (T_i - <T>)^2 / <T>^2, within 3 standard errors of 2 / g (99.7 % of a normal estimator), and those 3 standard errors must
    themselves be below 11 % of 2 / g."""
    ref = _ref("npt_mtk", 4.0)
    _, rows = _run(ref, 21000, record=True)
    rows = rows[1000:21000]
    block = 250
    p, t = rows[:, 2], rows[:, 1]
    p_se = _block_standard_error(p, block)
    print(f"<P> = {p.mean():.6e} eV/A^3 against {ref.p0:.1e}: {abs(p.mean() - ref.p0) / p_se:.2f} standard errors of {p_se:.2e}")
    assert abs(p.mean() - ref.p0) < 4 * p_se
    x = (t - t.mean()) ** 2 / t.mean() ** 2
    x_se = _block_standard_error(x, block)
    want = 2.0 / ref.g
    print(f"var(T)/<T>^2 = {x.mean():.5f} against 2/g = {want:.5f}: standard error {x_se:.5f} ({x_se / want:.1%})")
    assert 3 * x_se < 0.11 * want
    assert abs(x.mean() - want) < 3 * x_se
    assert abs(t.mean() / (300.0 * ref.g / (3 * len(ref.m))) - 1.0) < 0.02


def test_restatement_nvt_mean_temperature():
    """The gate and the run shape of tests/test_gpu_nhc.py's 300 K test (2,000 steps of 2 fs from a perfect lattice, the mean of the
    last 1,500 within 5 % of t0 g / (3 n)): taut = 50 fs meets it here, on a third of the atoms."""
    from torch_m3gnet.dynamics import maxwell_boltzmann

    pos, lat = fcc(A_START)
    m = np.full(len(pos), CU)
    ref = nr.NhcReference(pos, lat, m, maxwell_boltzmann(m, 300.0, 5), "nvt_nose_hoover", temperature=300.0, dt=2.0, taut=50.0)
    _, rows = _run(ref, 2000, record=True)
    assert abs(rows[-1500:, 1].mean() / (300.0 * ref.g / (3 * len(m))) - 1.0) < 0.05


@pytest.mark.parametrize("ensemble", ["nvt_nose_hoover", "npt_mtk"])
def test_restatement_chain_length_and_substeps_change_the_trajectory_and_conserve(ensemble):
    """Conserving H means that its error is the integrator's own, O(dt^2): halving dt takes a quarter of it, to within [3, 5]."""
    runs = {}
    for key, kw in (("m3", {}), ("m1", dict(chain_length=1)), ("nc2", dict(chain_substeps=2))):
        ref = _ref(ensemble, 2.0, **kw)
        h2, _ = _run(ref, 200)
        h1, _ = _run(_ref(ensemble, 1.0, **kw), 400)
        d2, d1 = np.abs(h2 - h2[0]).max(), np.abs(h1 - h1[0]).max()
        assert d1 > 0 and 3.0 <= d2 / d1 <= 5.0, (key, d1, d2)
        runs[key] = ref.pos.copy()
    assert np.abs(runs["m1"] - runs["m3"]).max() > 1e-6 and np.abs(runs["nc2"] - runs["m3"]).max() > 1e-9


def test_restatement_flags_non_finite_forces_and_freezes():
    ref = _ref("npt_mtk", 1.0)
    e, f, s = smooth_lj(ref.pos, ref.lattice)
    ref.step(f, s)
    pos, lat, obs = ref.pos.copy(), ref.lattice.copy(), ref.obs.copy()
    bad = s.copy()
    bad[1] = np.inf
    ref.step(f, bad)
    ref.step(f, s)
    assert ref.flags & nr.ERROR and ref.n_steps == 1
    assert np.array_equal(ref.pos, pos) and np.array_equal(ref.lattice, lat) and np.array_equal(ref.obs, obs)


# ---- argument checks (no device needed: refused before any HIP call) ------------------------------------------------------------
def _params(**kw):
    from torch_m3gnet import _lib

    p = dict(ensemble=_lib.NHC_NPT_MTK, fix_com=1, chain_length=3, chain_substeps=1, dt=1.0, taut=100.0, pressure=0.0, taup=1000.0)
    p.update(kw)
    return _lib.M3GNhcParams(**p)


def _init(params, offsets=(0, 2), masses=(1.0, 1.0), temps=(300.0,), state_bytes=1 << 20):
    from torch_m3gnet import _lib

    lib = _lib.load_library()
    offs = np.array(offsets, dtype=np.int64)
    m = np.array(masses, dtype=np.float64)
    t = np.array(temps, dtype=np.float64)
    dummy = C.c_void_p(256)   # never dereferenced: the call returns at the checks
    return lib.m3g_nhc_init(C.byref(params), int(offs[-1]), len(offs) - 1, offs.ctypes.data, m.ctypes.data, t.ctypes.data, dummy, dummy,
                            state_bytes, None)


@pytest.mark.parametrize("bad,why", [(dict(ensemble=2), "ensemble"), (dict(ensemble=-1), "ensemble"), (dict(fix_com=2), "fix_com"),
                                     (dict(chain_length=0), "chain_length"), (dict(chain_length=9), "chain_length"),
                                     (dict(chain_substeps=0), "chain_substeps"), (dict(chain_substeps=9), "chain_substeps"),
                                     (dict(dt=0.0), "dt"), (dict(dt=float("nan")), "dt"), (dict(taut=0.0), "taut"),
                                     (dict(taup=-1.0), "taup"), (dict(pressure=float("nan")), "pressure")])
def test_c_abi_refuses_invalid_nhc_parameters(bad, why):
    from torch_m3gnet import _lib

    lib = _lib.load_library()
    assert _init(_params(**bad)) == _lib.M3G_ERR_VALUE
    assert why.encode() in lib.m3g_last_error()
    dummy = C.c_void_p(256)
    assert lib.m3g_nhc_step(C.byref(_params(**bad)), 2, 1, dummy, 1 << 20, dummy, dummy, dummy, dummy, dummy, 0, dummy, None) == _lib.M3G_ERR_VALUE
    assert why.encode() in lib.m3g_last_error()


def test_c_abi_refuses_bad_temperatures_single_atoms_sizes_and_a_missing_lattice():
    from torch_m3gnet import _lib

    lib = _lib.load_library()
    assert _init(_params(), temps=(0.0,)) == _lib.M3G_ERR_VALUE and b"temperature" in lib.m3g_last_error()
    assert _init(_params(), temps=(float("nan"),)) == _lib.M3G_ERR_VALUE
    assert _init(_params(), offsets=(0, 1, 3), masses=(1.0,) * 3, temps=(300.0,) * 2) == _lib.M3G_ERR_VALUE
    assert b"fix_com" in lib.m3g_last_error()
    assert _init(_params(), masses=(1.0, 0.0)) == _lib.M3G_ERR_VALUE
    assert _init(_params(), offsets=(0, 2, 2), masses=(1.0,) * 2, temps=(300.0,) * 2) == _lib.M3G_ERR_VALUE
    # valid parameters, taup unused in NVT, one atom without fix_com: past the checks, the state buffer is too small
    assert _init(_params(ensemble=_lib.NHC_NVT, taup=0.0, fix_com=0), offsets=(0, 1, 3), masses=(1.0,) * 3, temps=(300.0,) * 2,
                 state_bytes=1) == _lib.M3G_ERR_SIZE
    dummy = C.c_void_p(256)
    assert lib.m3g_nhc_step(C.byref(_params()), 4, 1, dummy, 1 << 20, dummy, None, dummy, dummy, dummy, 0, None, None) == _lib.M3G_ERR_VALUE
    assert b"stresses" in lib.m3g_last_error()
    assert lib.m3g_nhc_step(C.byref(_params()), 4, 1, dummy, 1 << 20, dummy, dummy, dummy, None, None, 0, None, None) == _lib.M3G_ERR_VALUE
    assert b"lattice" in lib.m3g_last_error()
    size, small = C.c_size_t(), C.c_size_t()
    assert lib.m3g_nhc_state_bytes(10000, 3, 8, C.byref(size)) == _lib.M3G_OK and size.value > 10000 * 4 * 8
    assert lib.m3g_nhc_state_bytes(10000, 3, 1, C.byref(small)) == _lib.M3G_OK and small.value <= size.value
    for n, s, m in ((2, 3, 3), (0, 1, 3), (4, 0, 3), (4, 1, 0), (4, 1, 9)):
        assert lib.m3g_nhc_state_bytes(n, s, m, C.byref(size)) == _lib.M3G_ERR_VALUE
    mass_at, vel_at = C.c_size_t(), C.c_size_t()
    assert lib.m3g_nhc_state_view(100, 2, 3, C.byref(mass_at), C.byref(vel_at)) == _lib.M3G_OK and 0 < mass_at.value < vel_at.value
    assert lib.m3g_nhc_state_view(100, 2, 0, C.byref(mass_at), C.byref(vel_at)) == _lib.M3G_ERR_VALUE


def test_molecular_dynamics_refuses_bad_nhc_arguments():
    import torch

    from torch_m3gnet.dynamics import MolecularDynamics, NhcState
    from torch_m3gnet.model.build import build_model
    from torch_m3gnet.trajectory import TrajectoryObservables

    model = build_model(5.0, 4.0, 3, 3, 95, 16, 1)
    for kw, why in ((dict(chain_length=0), "chain_length"), (dict(chain_length=9), "chain_length"), (dict(chain_length=2.5), "chain_length"),
                    (dict(chain_substeps=0), "chain_substeps"), (dict(chain_substeps=9), "chain_substeps"),
                    (dict(temperature=0.0), "temperature"), (dict(temperature=[300.0, 0.0]), "temperature"), (dict(taut=0.0), "taut"),
                    (dict(taup=-1.0), "taup")):
        for ensemble in ("nvt_nose_hoover", "npt_mtk"):
            with pytest.raises(ValueError, match=why):
                MolecularDynamics(model, ensemble=ensemble, **kw)
    npt = MolecularDynamics(model, ensemble="npt_mtk", temperature=300.0)   # no compressibility needed
    assert npt.fix_com is True and npt.chain_length == 3 and npt.chain_substeps == 1
    pos, lat = fcc(3.6)
    z = np.full(len(pos), 29)
    with pytest.raises(ValueError, match="fix_com"):   # one atom, no degrees of freedom left
        MolecularDynamics(model, ensemble="nvt_nose_hoover").run([lat], [pos[:1]], [z[:1]], steps=1)
    with pytest.raises(ValueError, match="npt_mtk"):
        npt.run([lat], [pos], [z], steps=1, observables=TrajectoryObservables())
    with pytest.raises(ValueError, match="lattice"):
        npt.run([None], [pos], [z], steps=1)
    x, v = torch.zeros(4, 3, dtype=torch.float64), torch.zeros(4, 3, dtype=torch.float64)
    with pytest.raises(ValueError, match="lattice"):
        NhcState(x, None, [0, 4], np.ones(4), v, [300.0], ensemble="npt_mtk")
    with pytest.raises(ValueError, match="ensemble"):
        NhcState(x, None, [0, 4], np.ones(4), v, [300.0], ensemble="nve")


def test_new_symbols_are_declared_bound_and_exported():
    from torch_m3gnet import _lib, dynamics

    header = (ROOT / "include" / "m3gnet_hip.h").read_text()
    lib = _lib.load_library()
    for name in ("m3g_nhc_state_bytes", "m3g_nhc_state_view", "m3g_nhc_init", "m3g_nhc_step", "m3g_nhc_read"):
        assert re.search(rf"\bint {name}\(", header) and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert "m3g_nhc_params" in header and C.sizeof(_lib.M3GNhcParams) == 4 * 4 + 4 * 8
    assert set(dynamics.ENSEMBLES) == {"nve", "nvt_berendsen", "nvt_langevin", "npt_berendsen"}
    assert set(dynamics.NHC_ENSEMBLES) == {"nvt_nose_hoover", "npt_mtk"}
    assert hasattr(dynamics, "NhcState") and hasattr(dynamics, "nhc_step")
