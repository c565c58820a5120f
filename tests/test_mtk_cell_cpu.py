"""CPU checks of the flexible-cell MTK NPT ensemble: the numpy restatement (tests/mtk_cell_reference.py, the yardstick of
tests/test_gpu_mtk_cell.py) held to physics on the smoothly truncated Lennard-Jones fcc cell of tests/test_nhc_cpu.py, here in
triclinic cells -- forces and the full virial tensor as derivatives, second-order drift of the conserved quantity, time reversal,
the mean pressure tensor and the canonical temperature fluctuation of long runs under both cell masks, chains of different length
and substeps, error freezing -- and the C ABI / MolecularDynamics refusing bad arguments before touching a device."""
import ctypes as C
import functools
import itertools
import re
from pathlib import Path

import numpy as np
import pytest

import mtk_cell_reference as mr

ROOT = Path(__file__).resolve().parent.parent
CU = 63.546
EPS, SIGMA, R_ON, RC = 0.4, 2.3, 2.9, 3.4   # eV, A: the potential of tests/test_nhc_cpu.py
FCC_BASE = np.array([[0, 0, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0.5, 0.5, 0]])
SHIFTS = np.array(list(itertools.product((-2, -1, 0, 1, 2), repeat=3)), dtype=np.float64)
A_START = 3.63
SKIN = 0.8
MASKS = ["full", "orthorhombic"]
P_EXT = 2e-3


def fcc(a, n=2):
    grid = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1).reshape(-1, 1, 3)
    return (grid + FCC_BASE[None]).reshape(-1, 3) * a, np.eye(3) * n * a


class SmoothLJ:
    """tests/test_nhc_cpu.py's SmoothLJ for any cell: energy, forces and pair-virial stresses (Voigt xx, yy, zz, yz, zx, xy, W / V)
    of LJ times the quintic switch.  The pairs within RC + SKIN (with their image shifts, over unwrapped positions) are listed once
    and listed again before atoms moving in the scaled frame and the strain of the cell since can together have brought an unlisted
    pair SKIN nearer."""

    def __init__(self):
        self.frac0 = None

    def _build(self, frac, lattice):
        heights = abs(np.linalg.det(lattice)) / np.linalg.norm(np.cross(lattice[[1, 2, 0]], lattice[[2, 0, 1]]), axis=1)
        assert heights.min() > RC + SKIN and np.abs(frac - 0.5).max() < 1.0   # the +-2 image shifts then cover RC + SKIN
        rij = (frac[None, :, None, :] + SHIFTS[None, None, :, :] - frac[:, None, None, :]) @ lattice
        r = np.sqrt((rij * rij).sum(-1))
        self.i, self.j, s = np.nonzero((r > 1e-9) & (r < RC + SKIN))
        self.shift, self.frac0, self.lat0 = SHIFTS[s], frac.copy(), lattice.copy()

    def __call__(self, pos, lattice):
        frac = np.linalg.solve(lattice.T, pos.T).T
        if self.frac0 is not None:   # an unlisted pair was RC + SKIN apart: the strain since takes (1 - smin) of that, two atoms 2 moved
            smin = np.linalg.svd(np.linalg.solve(self.lat0, lattice), compute_uv=False).min()
            moved = np.sqrt((((frac - self.frac0) @ lattice) ** 2).sum(1)).max()
        if self.frac0 is None or 2.0 * moved + max(0.0, 1.0 - smin) * (RC + SKIN) > SKIN:
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


def _triclinic(pos, lat, seed=11):
    """The cell and positions times I + D, D symmetric with |D_ab| <= 0.02."""
    d = np.random.default_rng(seed).uniform(-0.02, 0.02, (3, 3))
    d = np.triu(d) + np.triu(d, 1).T
    return pos @ (np.eye(3) + d), lat @ (np.eye(3) + d)


def _start(mask, seed=3, temperature=300.0, cubic=False):
    from torch_m3gnet.dynamics import maxwell_boltzmann

    pos, lat = fcc(A_START)
    pos = pos + np.random.default_rng(seed).normal(0, 0.02, pos.shape)
    if not cubic:
        if mask == "full":
            pos, lat = _triclinic(pos, lat)
        else:   # the same strain's diagonal: an orthorhombic cell of three different lengths
            d = np.diag(np.diag(_triclinic(np.eye(3), np.eye(3))[1]))
            pos, lat = pos @ d, lat @ d
    m = np.full(len(pos), CU)
    return pos, lat, m, maxwell_boltzmann(m, temperature, seed)


def _ref(mask, dt, cubic=False, **kw):
    pos, lat, m, v = _start(mask, cubic=cubic)
    args = dict(temperature=300.0, dt=dt, taut=50.0, taup=300.0, pressure=P_EXT)
    args.update(kw)
    return mr.MtkCellReference(pos, lat, m, v, mask, **args)


def _run(ref, n_steps, record=False):
    """n_steps steps (n_steps + 1 calls, the last finish_only): H = e_pot + KE + extended at every full step."""
    h, rows, lats, pot = [], [], [], SmoothLJ()
    for k in range(n_steps + 1):
        e, f, s = pot(ref.pos, ref.lattice)
        if record:
            lats.append(ref.lattice.copy())
        ref.step(f, s, finish_only=(k == n_steps))
        h.append(e + ref.obs[0] + ref.obs[4])
        if record:
            rows.append(ref.obs.copy())
    assert not ref.flags & mr.ERROR
    return np.array(h), np.array(rows), np.array(lats)


def test_smooth_lj_forces_and_full_virial_are_derivatives_in_a_triclinic_cell():
    pos, lat = fcc(A_START)
    pos = pos + np.random.default_rng(1).normal(0, 0.05, pos.shape)
    pos, lat = _triclinic(pos, lat)
    assert np.abs(lat - np.diag(np.diag(lat))).max() > 0.01
    e, f, s = smooth_lj(pos, lat)
    h = 1e-5
    for i, k in [(0, 0), (5, 1), (17, 2)]:
        dp = np.zeros_like(pos)
        dp[i, k] = h
        fd = -(smooth_lj(pos + dp, lat)[0] - smooth_lj(pos - dp, lat)[0]) / (2 * h)
        assert abs(fd - f[i, k]) < 1e-6 * max(1.0, abs(f[i, k]))
    w = mr.unpack(s) * abs(np.linalg.det(lat))
    for a, b in [(1, 1), (0, 1), (1, 2)]:   # one diagonal and two shear components of a symmetric strain
        strain = np.zeros((3, 3))
        strain[a, b] = strain[b, a] = 1.0
        up, down = np.eye(3) + h * strain, np.eye(3) - h * strain
        fd = -(smooth_lj(pos @ up, lat @ up)[0] - smooth_lj(pos @ down, lat @ down)[0]) / (2 * h)
        want = (w * strain).sum()
        assert abs(fd - want) < 1e-5 * max(1.0, abs(want)), (a, b, fd, want)


@pytest.mark.parametrize("mask", MASKS)
def test_restatement_conserved_quantity_error_is_second_order(mask):
    """400 fs at dt = 1 / 2 / 4 fs from the strained start.  Measured: full 3.16e-3 / 1.26e-2 / 4.62e-2 eV (ratios 4.00, 3.66);
    orthorhombic 2.65e-3 / 1.06e-2 / 3.98e-2 eV (4.00, 3.75)."""
    drift = []
    for dt in (1.0, 2.0, 4.0):
        h, _, _ = _run(_ref(mask, dt), int(400 / dt))
        drift.append(np.abs(h - h[0]).max())
    print(f"{mask}: drift of H over 400 fs at dt = 1, 2, 4 fs: {drift} (ratios {drift[1] / drift[0]:.2f}, {drift[2] / drift[1]:.2f})")
    assert drift[0] > 0
    assert 3.0 <= drift[1] / drift[0] <= 5.0 and 3.0 <= drift[2] / drift[1] <= 5.0, drift


@pytest.mark.parametrize("mask", MASKS)
def test_restatement_is_time_reversible(mask):
    ref = _ref(mask, 2.0)
    pos0, lat0 = ref.pos.copy(), ref.lattice.copy()
    _run(ref, 100)
    assert np.abs(ref.pos - pos0).max() > 0.05 and ref.n_steps == 100
    assert np.abs(ref.lattice - lat0).max() > 1e-4
    ref.reverse()
    _run(ref, 100)
    # measured: full 1.5e-14 A in positions and 6.0e-15 A in the cell, orthorhombic 8.4e-15 and 5.3e-15
    print(f"{mask}: back to {np.abs(ref.pos - pos0).max():.1e} A in positions, {np.abs(ref.lattice - lat0).max():.1e} A in the cell")
    assert np.abs(ref.pos - pos0).max() < 1e-9 and np.abs(ref.lattice - lat0).max() < 1e-9


def _block_standard_error(x, block):
    """Standard error of mean(x) from the means of consecutive blocks of `block` samples."""
    b = x[:len(x) // block * block].reshape(-1, block).mean(1)
    return b.std(ddof=1) / np.sqrt(len(b))


@functools.lru_cache(maxsize=None)
def _long_run(mask):
    """1,000 discarded and 20,000 retained steps of 4 fs from the cubic start at P_ext = 2e-3 eV/A^3: obs rows and cells."""
    ref = _ref(mask, 4.0, cubic=True)
    _, rows, lats = _run(ref, 21000, record=True)
    return ref, rows[1000:21000], lats[1000:21000], lats[0]


def _pressure_tensor_in_standard_errors(rows, components, target, block=250):
    out = []
    for j in components:
        x = rows[:, 6 + j]
        out.append(abs(x.mean() - target) / _block_standard_error(x, block))
    return out


def test_restatement_long_full_cell_run_samples_the_pressure_tensor_and_canonical_temperature():
    """Blocks of 250 steps (1 ps), as tests/test_nhc_cpu.py.  Gates: every diagonal mean of the pressure tensor within 4 standard
    errors of P_ext, every off-diagonal mean within 4 of 0; var(T) / <T>^2 within 3 standard errors of 2 / g, those 3 standard
    errors below 11 % of 2 / g.  Measured: diagonals 0.70, 1.09, 1.21 standard errors, off-diagonals 0.02, 0.04, 0.04;
    var(T) / <T>^2 0.02020 against 0.02151, 2.44 standard errors of 2.5 % (three of them 7.5 % of 2 / g)."""
    ref, rows, lats, lat0 = _long_run("full")
    diag = _pressure_tensor_in_standard_errors(rows, (0, 1, 2), ref.p0)
    off = _pressure_tensor_in_standard_errors(rows, (3, 4, 5), 0.0)
    print(f"full: pressure tensor means off by {diag} (diagonal) and {off} (off-diagonal) standard errors")
    assert max(diag) < 4.0 and max(off) < 4.0
    assert abs(rows[:, 2].mean() - rows[:, 6:9].mean()) < 1e-12
    t = rows[:, 1]
    x = (t - t.mean()) ** 2 / t.mean() ** 2
    x_se = _block_standard_error(x, 250)
    want = 2.0 / ref.g
    print(f"var(T)/<T>^2 = {x.mean():.5f} against 2/g = {want:.5f}: {abs(x.mean() - want) / x_se:.2f} standard errors of {x_se:.5f} "
          f"({x_se / want:.1%})")
    assert np.abs(lats - lat0)[:, [0, 0, 1], [1, 2, 2]].max() > 1e-3   # the shape moved
    assert abs(x.mean() - want) < 3 * x_se
    assert 3 * x_se < 0.11 * want


def test_restatement_long_orthorhombic_run_samples_the_diagonal_and_keeps_the_cell_along_the_axes():
    """Measured: the three diagonal means within 1.05, 0.93, 1.09 standard errors of P_ext."""
    ref, rows, lats, lat0 = _long_run("orthorhombic")
    diag = _pressure_tensor_in_standard_errors(rows, (0, 1, 2), ref.p0)
    print(f"orthorhombic: diagonal pressure means off by {diag} standard errors")
    assert max(diag) < 4.0
    off = lats - lats * np.eye(3)
    assert (off == 0.0).all() and (ref.lattice - np.diag(np.diag(ref.lattice)) == 0.0).all()
    assert np.ptp(np.diagonal(lats, axis1=1, axis2=2), axis=1).max() > 1e-3   # three lengths on their own


def test_restatement_sheared_cell_relaxes_towards_cubic():
    """The cubic-start run's time-averaged cell is cubic: the mean shear components are small against the diagonal's spread."""
    _, _, lats, _ = _long_run("full")
    mean = lats.mean(0)
    sym = 0.5 * (mean + mean.T)
    assert np.abs(sym - np.diag(np.diag(sym))).max() < 0.01 * sym[0, 0]
    assert np.ptp(np.diag(sym)) < 0.01 * sym[0, 0]


@pytest.mark.parametrize("mask", MASKS)
def test_restatement_chain_length_and_substeps_change_the_trajectory_and_conserve(mask):
    runs = {}
    for key, kw in (("m3", {}), ("m1", dict(chain_length=1)), ("nc2", dict(chain_substeps=2))):
        ref = _ref(mask, 2.0, **kw)
        h2, _, _ = _run(ref, 200)
        h1, _, _ = _run(_ref(mask, 1.0, **kw), 400)
        d2, d1 = np.abs(h2 - h2[0]).max(), np.abs(h1 - h1[0]).max()
        assert d1 > 0 and 3.0 <= d2 / d1 <= 5.0, (key, d1, d2)
        runs[key] = ref.pos.copy()
    assert np.abs(runs["m1"] - runs["m3"]).max() > 1e-6 and np.abs(runs["nc2"] - runs["m3"]).max() > 1e-9


def test_restatement_full_mask_reduces_to_the_isotropic_family_when_the_rate_is_isotropic():
    """tr G / 3 is the isotropic family's G_eps and W_g its W / 3: the first opening T(h) from rest gives tr vg / 3 = veps."""
    import nhc_reference as nr

    pos, lat, m, v = _start("full")
    _, f, s = smooth_lj(pos, lat)
    args = dict(temperature=300.0, dt=1.0, taut=50.0, taup=300.0, pressure=P_EXT)
    cell, iso = mr.MtkCellReference(pos, lat, m, v, "full", **args), nr.NhcReference(pos, lat, m, v, "npt_mtk", **args)
    cell.step(f, s)
    iso.step(f, s)
    assert abs(np.trace(cell.vg) / 3.0 - iso.veps) < 1e-12 * abs(iso.veps)
    assert np.allclose(cell.obs[:4], iso.obs[:4], rtol=1e-12, atol=0.0)


@pytest.mark.parametrize("mask", MASKS)
def test_restatement_flags_bad_stresses_and_freezes(mask):
    for bad_value in (np.inf, 1e3):   # non-finite; finite, and large enough to push |vg| dt past 0.05
        ref = _ref(mask, 1.0)
        e, f, s = smooth_lj(ref.pos, ref.lattice)
        ref.step(f, s)
        pos, lat, obs, row, v = ref.pos.copy(), ref.lattice.copy(), ref.obs.copy(), ref.chain_row(), ref.v.copy()
        bad = s.copy()
        bad[1] = bad_value
        ref.step(f, bad)
        assert ref.flags & mr.ERROR and ref.n_steps == 1, bad_value
        ref.step(f, s)
        assert ref.flags & mr.ERROR and ref.n_steps == 1
        assert np.array_equal(ref.pos, pos) and np.array_equal(ref.lattice, lat) and np.array_equal(ref.obs, obs)
        assert np.array_equal(ref.chain_row(), row) and np.array_equal(ref.v, v)


# ---- argument checks (no device needed: refused before any HIP call) ------------------------------------------------------------
def _params(**kw):
    from torch_m3gnet import _lib

    p = dict(cell_mask=_lib.MTK_CELL_FULL, fix_com=1, chain_length=3, chain_substeps=1, dt=1.0, taut=100.0, pressure=0.0, taup=1000.0)
    p.update(kw)
    return _lib.M3GMtkParams(**p)


def _init(params, offsets=(0, 2), masses=(1.0, 1.0), temps=(300.0,), state_bytes=1 << 20):
    from torch_m3gnet import _lib

    lib = _lib.load_library()
    offs = np.array(offsets, dtype=np.int64)
    m = np.array(masses, dtype=np.float64)
    t = np.array(temps, dtype=np.float64)
    dummy = C.c_void_p(256)   # never dereferenced: the call returns at the checks
    return lib.m3g_mtk_init(C.byref(params), int(offs[-1]), len(offs) - 1, offs.ctypes.data, m.ctypes.data, t.ctypes.data, dummy, dummy,
                            state_bytes, None)


@pytest.mark.parametrize("bad,why", [(dict(cell_mask=2), "cell_mask"), (dict(cell_mask=-1), "cell_mask"), (dict(fix_com=2), "fix_com"),
                                     (dict(chain_length=0), "chain_length"), (dict(chain_length=9), "chain_length"),
                                     (dict(chain_substeps=0), "chain_substeps"), (dict(chain_substeps=9), "chain_substeps"),
                                     (dict(dt=0.0), "dt"), (dict(dt=float("nan")), "dt"), (dict(taut=0.0), "taut"),
                                     (dict(taup=-1.0), "taup"), (dict(taup=0.0), "taup"), (dict(pressure=float("nan")), "pressure"),
                                     (dict(pressure=float("inf")), "pressure")])
def test_c_abi_refuses_invalid_mtk_parameters(bad, why):
    from torch_m3gnet import _lib

    lib = _lib.load_library()
    assert _init(_params(**bad)) == _lib.M3G_ERR_VALUE
    assert why.encode() in lib.m3g_last_error()
    dummy = C.c_void_p(256)
    assert lib.m3g_mtk_step(C.byref(_params(**bad)), 2, 1, dummy, 1 << 20, dummy, dummy, dummy, dummy, dummy, 0, dummy, None) == _lib.M3G_ERR_VALUE
    assert why.encode() in lib.m3g_last_error()


def test_c_abi_refuses_bad_temperatures_single_atoms_sizes_and_missing_stresses_or_lattice():
    from torch_m3gnet import _lib

    lib = _lib.load_library()
    assert _init(_params(), temps=(0.0,)) == _lib.M3G_ERR_VALUE and b"temperature" in lib.m3g_last_error()
    assert _init(_params(), temps=(float("nan"),)) == _lib.M3G_ERR_VALUE
    assert _init(_params(), offsets=(0, 1, 3), masses=(1.0,) * 3, temps=(300.0,) * 2) == _lib.M3G_ERR_VALUE
    assert b"fix_com" in lib.m3g_last_error()
    assert _init(_params(), masses=(1.0, 0.0)) == _lib.M3G_ERR_VALUE
    assert _init(_params(), offsets=(0, 2, 2), masses=(1.0,) * 2, temps=(300.0,) * 2) == _lib.M3G_ERR_VALUE
    # valid parameters, one atom without fix_com: past the checks, the state buffer is too small
    assert _init(_params(fix_com=0, cell_mask=_lib.MTK_CELL_ORTHORHOMBIC), offsets=(0, 1, 3), masses=(1.0,) * 3, temps=(300.0,) * 2,
                 state_bytes=1) == _lib.M3G_ERR_SIZE
    dummy = C.c_void_p(256)
    assert lib.m3g_mtk_step(C.byref(_params()), 4, 1, dummy, 1 << 20, dummy, None, dummy, dummy, dummy, 0, None, None) == _lib.M3G_ERR_VALUE
    assert b"stresses" in lib.m3g_last_error()
    assert lib.m3g_mtk_step(C.byref(_params()), 4, 1, dummy, 1 << 20, dummy, dummy, dummy, None, None, 0, None, None) == _lib.M3G_ERR_VALUE
    assert b"lattice" in lib.m3g_last_error()
    assert lib.m3g_mtk_step(C.byref(_params()), 4, 1, dummy, 1, dummy, dummy, dummy, dummy, None, 0, None, None) == _lib.M3G_ERR_SIZE
    size, small, nhc = C.c_size_t(), C.c_size_t(), C.c_size_t()
    assert lib.m3g_mtk_state_bytes(10000, 3, 8, C.byref(size)) == _lib.M3G_OK and size.value > 10000 * 4 * 8
    assert lib.m3g_mtk_state_bytes(10000, 3, 1, C.byref(small)) == _lib.M3G_OK and small.value <= size.value
    assert lib.m3g_nhc_state_bytes(10000, 3, 8, C.byref(nhc)) == _lib.M3G_OK and size.value > nhc.value   # 13 partials, 42 coefficients
    for n, s, m in ((2, 3, 3), (0, 1, 3), (4, 0, 3), (4, 1, 0), (4, 1, 9)):
        assert lib.m3g_mtk_state_bytes(n, s, m, C.byref(size)) == _lib.M3G_ERR_VALUE
    mass_at, vel_at = C.c_size_t(), C.c_size_t()
    assert lib.m3g_mtk_state_view(100, 2, 3, C.byref(mass_at), C.byref(vel_at)) == _lib.M3G_OK and 0 < mass_at.value < vel_at.value
    assert lib.m3g_mtk_state_view(100, 2, 0, C.byref(mass_at), C.byref(vel_at)) == _lib.M3G_ERR_VALUE
    assert lib.m3g_mtk_read(4, 1, 0, dummy, 1 << 20, None, None, None, None, None) == _lib.M3G_ERR_VALUE


def test_molecular_dynamics_refuses_bad_mtk_cell_arguments():
    import torch

    from torch_m3gnet.dynamics import MolecularDynamics, MtkCellState
    from torch_m3gnet.model.build import build_model
    from torch_m3gnet.trajectory import TrajectoryObservables

    model = build_model(5.0, 4.0, 3, 3, 95, 16, 1)
    for kw, why in ((dict(chain_length=0), "chain_length"), (dict(chain_length=9), "chain_length"), (dict(chain_substeps=0), "chain_substeps"),
                    (dict(temperature=0.0), "temperature"), (dict(taut=0.0), "taut"), (dict(taup=-1.0), "taup"),
                    (dict(pressure=float("nan")), "pressure"), (dict(cell_mask="cubic"), "cell_mask"), (dict(cell_mask=1), "cell_mask")):
        with pytest.raises(ValueError, match=why):
            MolecularDynamics(model, ensemble="npt_mtk_cell", **kw)
    with pytest.raises(ValueError, match="ensemble"):
        MolecularDynamics(model, ensemble="npt_mtk_full")
    md = MolecularDynamics(model, ensemble="npt_mtk_cell", temperature=300.0)   # no compressibility needed
    assert md.fix_com is True and md.chain_length == 3 and md.chain_substeps == 1 and md.cell_mask == "full"
    pos, lat = fcc(3.6)
    z = np.full(len(pos), 29)
    with pytest.raises(ValueError, match="fix_com"):   # one atom, no degrees of freedom left
        md.run([lat], [pos[:1]], [z[:1]], steps=1)
    with pytest.raises(ValueError, match="npt_mtk_cell"):
        md.run([lat], [pos], [z], steps=1, observables=TrajectoryObservables())
    with pytest.raises(ValueError, match="lattice"):
        md.run([None], [pos], [z], steps=1)
    sheared = lat.copy()
    sheared[0, 1] = 1e-6
    ortho = MolecularDynamics(model, ensemble="npt_mtk_cell", cell_mask="orthorhombic")
    with pytest.raises(ValueError, match="orthorhombic"):
        ortho.run([lat, sheared], [pos, pos], [z, z], steps=1)
    x, v = torch.zeros(4, 3, dtype=torch.float64), torch.zeros(4, 3, dtype=torch.float64)
    with pytest.raises(ValueError, match="lattice"):
        MtkCellState(x, None, [0, 4], np.ones(4), v, [300.0])
    with pytest.raises(ValueError, match="cell_mask"):
        MtkCellState(x, torch.eye(3, dtype=torch.float64)[None], [0, 4], np.ones(4), v, [300.0], cell_mask="diagonal")


def test_new_symbols_are_declared_bound_and_exported():
    from torch_m3gnet import _lib, dynamics

    header = (ROOT / "include" / "m3gnet_hip.h").read_text()
    lib = _lib.load_library()
    for name in ("m3g_mtk_state_bytes", "m3g_mtk_state_view", "m3g_mtk_init", "m3g_mtk_step", "m3g_mtk_read"):
        assert re.search(rf"\bint {name}\(", header) and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert "m3g_mtk_params" in header and C.sizeof(_lib.M3GMtkParams) == 48
    assert re.search(r"#define M3G_MTK_OBS 12\b", header) and _lib.MTK_OBS == 12
    assert set(dynamics.MTK_CELL_ENSEMBLES) == {"npt_mtk_cell"} and set(dynamics.CELL_MASKS) == {"full", "orthorhombic"}
    assert set(dynamics.ENSEMBLES) == {"nve", "nvt_berendsen", "nvt_langevin", "npt_berendsen"}   # the other families keep theirs
    assert set(dynamics.NHC_ENSEMBLES) == {"nvt_nose_hoover", "npt_mtk"}
    assert C.sizeof(_lib.M3GNhcParams) == 48
    assert hasattr(dynamics, "MtkCellState") and hasattr(dynamics, "mtk_cell_step")
