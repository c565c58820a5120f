"""Thermodynamic fluctuation observables accumulated on the device: heat capacity, compressibility and bulk modulus, thermal expansion,
finite-temperature elastic constants and the Green-Kubo shear and bulk viscosities of every structure of a batch (C ABI:
m3g_thermo_*, csrc/m3g_thermo.hip).  The per-structure companion of `trajectory.py`, `scattering.py` and `local_order.py`.

`MolecularDynamics.run(..., observables=ThermoObservables(...))` (alone, or in a list beside the other three kinds) samples the run on
the device while it integrates -- nothing but the final accumulators goes to the host -- and every result dict gains "thermo".
`ThermoState` / `thermo_sample` are the layer below and take any samples.

Definitions (the same ones are restated in include/m3gnet_hip.h and tests/thermo_reference.py).  Every sample forms the row
    x = (e_pot, ke, V, h = e_pot + ke + p_ext V, p = tr P / 3, eps_xx, eps_yy, eps_zz, eps_yz, eps_zx, eps_xy)
with V = |det L|, eps = (A A^T - 1) / 2 the Green-Lagrange strain against the reference cell L0 (A = L0^-1 L, rows = lattice vectors)
and P = stresses + K / V the pressure tensor in the pair-virial convention of the integrators (K_ab = sum m v_a v_b / kappa in eV, minus
the centre-of-mass term with `remove_com`; ke = tr K / 2), or ke and P as an integrator's own `obs` row states them ("npt_mtk",
"npt_mtk_cell": their finish kick carries the barostat, so only the integrator knows the synchronous kinetic energy).  The device
keeps the running mean and the Welford co-moments C_ij = sum (x_i - <x_i>)(x_j - <x_j>) of the row, so Cov = C / n_samples, and, with
n_lags > 0, per lag l the sums of u_c(t) u_c(t - l), u_c(t) and u_c(t - l) of u = (P_xx, P_yy, P_zz, P_yz, P_zx, P_xy, p) over a ring of
the last n_lags samples.  A sample that holds a non-finite value is skipped, flagged, and empties the ring.  With T = 2 <ke> / (g kB),
g = 3 n, or 3 n - 3 with `remove_com` or under a run that holds the total momentum at zero (`fix_com` of `MolecularDynamics`: the
integrators then have 3 n - 3 degrees of freedom, and 3 n would bias T, and with it every quantity below, by (n - 1) / n):
    heat_capacity      Var(e_pot + ke) / (kB T^2)                      "nvt_langevin", "nvt_nose_hoover" (C_v)
                       (g kB / 2) / (1 - 2 Var(ke) / (g kB^2 T^2))     "nve" (Lebowitz, Percus and Verlet, Phys. Rev. 153, 250 (1967))
                       Var(h) / (kB T^2)                               "npt_mtk", "npt_mtk_cell" (C_p)
    compressibility    Var(V) / (kB T <V>), bulk_modulus its inverse   "npt_mtk", "npt_mtk_cell"
    thermal_expansion  Cov(V, h) / (kB T^2 <V>)                        "npt_mtk", "npt_mtk_cell"
    elastic_constants  C = S^-1, S = <V> Cov(e) / (kB T), e the Voigt strain (eps_xx, eps_yy, eps_zz, 2 eps_yz, 2 eps_zx, 2 eps_xy)
                       (Parrinello and Rahman, J. Chem. Phys. 76, 2662 (1982))                       "npt_mtk_cell"
    shear ACF          (sum_a c_aa + 2 sum_{a<b} c_ab - 3 c_p) / 10, c_c(l) = <u_c u_c'> - <u_c><u_c'>  (Daivis and Evans, J. Chem. Phys.
                       100, 541 (1994)); bulk ACF c_p; eta(t) = <V> / (kB T) int_0^t ACF, viscosity its mean over `plateau_window`.
The Berendsen ensembles do not sample the fluctuations of any ensemble (the weak coupling suppresses those of ke and of V), so their
fluctuation quantities are None; their means are returned."""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np
import torch

from . import _cuda, _lib
from ._driver import EV_A3_TO_GPA, atom_offsets, boolean, check_tensor, integer, read_state, state_tensor
from .data.graph_gpu import _ptr, _stream

KB = 8.617333262e-5                 # eV/K
EV_FS_A3_TO_MPA_S = 0.1602176634    # 1 eV fs / A^3 = 1.602176634e-4 Pa s
ROW, TENSOR = _lib.THERMO_ROW, _lib.THERMO_TENSOR
COLUMNS = ("e_pot", "ke", "v", "h", "p", "eps_xx", "eps_yy", "eps_zz", "eps_yz", "eps_zx", "eps_xy")
CANONICAL = ("nvt_langevin", "nvt_nose_hoover")
ISOBARIC = ("npt_mtk", "npt_mtk_cell")


class ThermoState:
    """Accumulators of a batch on the device (m3g_thermo_init).  `offsets`: S + 1 atom offsets; `masses` [N] amu; `p_ext` [S] (eV/A^3):
    the external pressure of the enthalpy; `reference_cells` [S,3,3] (A): the L0 of the strain.  `n_lags` = 0 switches the stress
    correlations off."""

    def __init__(self, n_atoms: int, offsets: Sequence[int], masses, p_ext, reference_cells, n_lags: int = 0, remove_com: bool = False,
                 device="cuda"):
        self.offsets = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64))
        self.N, self.S = integer("n_atoms", n_atoms, 1), int(len(self.offsets) - 1)
        self.masses = np.ascontiguousarray(np.asarray(masses, dtype=np.float64).reshape(-1))
        if len(self.masses) != self.N:
            raise ValueError(f"expected {self.N} masses")
        self.p_ext = np.ascontiguousarray(np.broadcast_to(np.asarray(p_ext, dtype=np.float64), (self.S,)))
        self.reference_cells = np.ascontiguousarray(np.asarray(reference_cells, dtype=np.float64))
        if self.reference_cells.shape != (self.S, 3, 3):
            raise ValueError(f"reference_cells: expected [{self.S}, 3, 3]")
        self.lags = integer("n_lags", n_lags, 0)
        self.remove_com = boolean("remove_com", remove_com)
        self.sizes = _lib.M3GThermoSizes(self.N, self.S, self.lags)
        self.params = _lib.M3GThermoParams(1 if self.remove_com else 0)
        self.lib = _lib.load_library()
        self.device = torch.device(device)
        self.state = state_tensor(self.lib.m3g_thermo_state_bytes, C.byref(self.sizes), device=self.device)
        with _cuda.on_device(self.device):
            _lib.check(self.lib.m3g_thermo_init(C.byref(self.sizes), C.byref(self.params), self.offsets.ctypes.data, self.masses.ctypes.data,
                                                self.p_ext.ctypes.data, self.reference_cells.ctypes.data, _ptr(self.state),
                                                self.state.numel(), _stream()))

    def read(self) -> dict:
        """The raw accumulators, copied to the host (waits for the stream): mean [S, 11], comoments [S, 66] (upper triangle, row-major),
        lag_uu, lag_now, lag_old [S, n_lags, 7], lag_count [S, n_lags], n_samples, n_skipped, flags [S]."""
        S, G = self.S, self.lags
        return read_state(self.lib.m3g_thermo_read, (C.byref(self.sizes),), self.state,
                          (("mean", np.float64, (S, ROW)), ("comoments", np.float64, (S, _lib.THERMO_COMOMENTS)),
                           ("lag_uu", np.float64, (S, G, TENSOR)), ("lag_now", np.float64, (S, G, TENSOR)),
                           ("lag_old", np.float64, (S, G, TENSOR)), ("lag_count", np.int64, (S, G)), ("n_samples", np.int64, S),
                           ("n_skipped", np.int64, S), ("flags", np.int32, S)))

    def frame(self, lag: int = 0):
        """(row [S, 11], tensor [S, 7] or None without a ring) of the last sample, the tensor `lag` samples back (NaN for a structure
        whose ring holds no such entry), copied to the host (waits for the stream)."""
        row = np.empty((self.S, ROW))
        tensor = np.empty((self.S, TENSOR)) if self.lags else None
        with _cuda.on_device(self.device):
            _lib.check(self.lib.m3g_thermo_frame(C.byref(self.sizes), _ptr(self.state), self.state.numel(), int(lag), row.ctypes.data,
                                                 tensor.ctypes.data if tensor is not None else None, _stream()))
        return row, tensor


def _strided(name: str, x: torch.Tensor, rows: int, width: int):
    """(pointer, row stride in elements) of an fp64 device view of `rows` rows of `width` contiguous values (a column block of an
    integrator's `obs`)."""
    shape = (rows,) if width == 1 else (rows, width)
    if x.dtype != torch.float64 or tuple(x.shape) != shape or (width > 1 and x.stride(1) != 1) or x.stride(0) < width:
        raise ValueError(f"{name} must be a float64 view of {list(shape)} with contiguous rows")
    return x.data_ptr(), int(x.stride(0))


def thermo_sample(state: ThermoState, energies: torch.Tensor, stresses: torch.Tensor, lattice: torch.Tensor, vel: torch.Tensor | None = None,
                  forces: torch.Tensor | None = None, kick: float = 0.0, kinetic: torch.Tensor | None = None,
                  pressure_tensor: torch.Tensor | None = None) -> None:
    """One sample of the batch (m3g_thermo_sample): `energies` [S] and `stresses` [S,6] float32 (pair virial), `lattice` [S,3,3] fp64,
    and exactly one of `vel` [N,3] fp64 (with `forces` [N,3] float32 the sampled velocity is vel + kick * kappa * forces / m, as in
    `traj_sample`) and `kinetic`, a float64 view [S] of the kinetic energies (eV; any stride: a column of an integrator's `obs`), beside
    which `pressure_tensor` may be a view [S,6] (eV/A^3, Voigt xx, yy, zz, yz, zx, xy; rows contiguous, any row stride).  Queued on the
    current stream; no wait, capture-safe."""
    check_tensor("energies", energies, (state.S,), torch.float32)
    check_tensor("stresses", stresses, (state.S, 6), torch.float32)
    check_tensor("lattice", lattice, (state.S, 3, 3), torch.float64)
    if vel is not None:
        check_tensor("vel", vel, (state.N, 3), torch.float64)
    if forces is not None:
        check_tensor("forces", forces, (state.N, 3), torch.float32)
    k_ptr, k_stride = _strided("kinetic", kinetic, state.S, 1) if kinetic is not None else (None, 0)
    t_ptr, t_stride = _strided("pressure_tensor", pressure_tensor, state.S, 6) if pressure_tensor is not None else (None, 0)
    with _cuda.on_device(state.device):
        _lib.check(state.lib.m3g_thermo_sample(C.byref(state.sizes), C.byref(state.params), _ptr(state.state), state.state.numel(),
                                               _ptr(energies), _ptr(stresses), _ptr(lattice), _ptr(vel), _ptr(forces), float(kick), k_ptr,
                                               k_stride, t_ptr, t_stride, _stream()))


def decode_flags(flags: int) -> dict:
    """{"nonfinite"}: whether a sample of the structure held a non-finite value (it was then left out)."""
    return {"nonfinite": bool(int(flags) & _lib.THERMO_NONFINITE)}


# ---- host post-processing (numpy, one structure) ------------------------------------------------------------------------------------
def covariance(comoments, n_samples: int) -> np.ndarray:
    """The population covariance [11, 11] of the row from the 66 upper-triangle co-moments (NaN without samples)."""
    cov = np.zeros((ROW, ROW))
    cov[np.triu_indices(ROW)] = np.asarray(comoments, dtype=np.float64)
    cov = cov + np.triu(cov, 1).T
    with np.errstate(divide="ignore", invalid="ignore"):
        return cov / float(n_samples)


def thermo_from_moments(mean, comoments, n_samples: int, n_atoms: int, ensemble: str | None = None, remove_com: bool = False,
                        cell_mask: str = "full") -> dict:
    """Means and fluctuation quantities of one structure from its accumulators (module docstring).  Energies in eV, `t` in K, `p` in
    GPa, `v` in A^3; `mean` [11] and `covariance` [11, 11]: of the row itself, in its own units (eV, A^3, eV/A^3); heat_capacity in eV/K (and heat_capacity_kb: per atom in units of kB), compressibility in 1/GPa, bulk_modulus in
    GPa, thermal_expansion (volumetric) in 1/K, elastic_constants [6, 6] in GPa (Voigt; NaN outside the block the `cell_mask` lets
    fluctuate).  `remove_com`: the centre of mass carries no kinetic energy (removed by the sampler, or held by the run): g = 3 n - 3.
    What the ensemble does not define is None: everything but the means for the Berendsen ensembles, which sample no
    ensemble's fluctuations, and for `ensemble` None."""
    mean = np.asarray(mean, dtype=np.float64)
    cov = covariance(comoments, n_samples)
    g = 3.0 * n_atoms - (3.0 if remove_com else 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = 2.0 * mean[1] / (g * KB) if g > 0 else np.nan
        out = {"e_pot": mean[0], "ke": mean[1], "t": t, "v": mean[2], "h": mean[3], "p": mean[4] * EV_A3_TO_GPA, "strain": mean[5:].copy(),
               "mean": mean.copy(), "covariance": cov, "heat_capacity": None, "heat_capacity_kb": None, "compressibility": None, "bulk_modulus": None,
               "thermal_expansion": None, "elastic_constants": None}
        if ensemble in CANONICAL:
            out["heat_capacity"] = (cov[0, 0] + cov[1, 1] + 2.0 * cov[0, 1]) / (KB * t * t)
        elif ensemble == "nve":
            out["heat_capacity"] = 0.5 * g * KB / (1.0 - 2.0 * cov[1, 1] / (g * KB * KB * t * t))
        elif ensemble in ISOBARIC:
            out["heat_capacity"] = cov[3, 3] / (KB * t * t)
            kappa_t = cov[2, 2] / (KB * t * mean[2])   # A^3/eV
            out["compressibility"] = kappa_t / EV_A3_TO_GPA
            out["bulk_modulus"] = EV_A3_TO_GPA / kappa_t
            out["thermal_expansion"] = cov[2, 3] / (KB * t * t * mean[2])
        if out["heat_capacity"] is not None:
            out["heat_capacity_kb"] = out["heat_capacity"] / (n_atoms * KB)
        if ensemble == "npt_mtk_cell":
            voigt = np.array([1.0, 1.0, 1.0, 2.0, 2.0, 2.0])
            compliance = mean[2] * cov[5:, 5:] * np.outer(voigt, voigt) / (KB * t)   # A^3/eV
            active = np.arange(6 if cell_mask == "full" else 3)
            c = np.full((6, 6), np.nan)
            block = compliance[np.ix_(active, active)]
            if np.isfinite(block).all() and np.linalg.matrix_rank(block) == len(active):
                c[np.ix_(active, active)] = np.linalg.inv(block) * EV_A3_TO_GPA
            out["elastic_constants"] = c
    return out


def running_integral(y, dt: float) -> np.ndarray:
    """The running trapezoid integral of `y` sampled every `dt` along the last axis (0 at the first point)."""
    y = np.asarray(y, dtype=np.float64)
    out = np.zeros_like(y)
    out[..., 1:] = np.cumsum(0.5 * (y[..., 1:] + y[..., :-1]) * dt, axis=-1)
    return out


def stress_correlations(lag_uu, lag_now, lag_old, lag_count, mean_volume: float, temperature: float, dt: float,
                        plateau_window=(0.5, 1.0)) -> dict:
    """The Green-Kubo analysis of one structure from its lag sums [n_lags, 7] (module docstring); `dt`: the time between two samples
    (fs).  time (fs), tensor_mean [7] (eV/A^3: the mean of u over the samples), tensor_acf [n_lags, 7], shear_acf, bulk_acf (eV^2/A^6), eta_shear, eta_bulk (running integrals, mPa s),
    viscosity_shear, viscosity_bulk (mPa s): the mean of the running integral over `plateau_window` (fractions of the longest lag;
    NaN while a lag in it has no sample)."""
    k = np.asarray(lag_count, dtype=np.float64)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.asarray(lag_uu, dtype=np.float64) / k - (np.asarray(lag_now, dtype=np.float64) / k) * (np.asarray(lag_old, dtype=np.float64) / k)
        shear = (c[:, 0] + c[:, 1] + c[:, 2] + 2.0 * (c[:, 3] + c[:, 4] + c[:, 5]) - 3.0 * c[:, 6]) / 10.0
        bulk = c[:, 6]
        scale = mean_volume / (KB * temperature) * EV_FS_A3_TO_MPA_S
        eta_s, eta_b = scale * running_integral(shear, dt), scale * running_integral(bulk, dt)
    G = len(shear)
    time = np.arange(G) * dt
    lo, hi = plateau_window[0] * time[-1], plateau_window[1] * time[-1]
    window = (time >= lo) & (time <= hi)
    with np.errstate(divide="ignore", invalid="ignore"):
        tensor_mean = np.asarray(lag_now, dtype=np.float64)[0] / k[0]
    return {"time": time, "lag_count": np.asarray(lag_count).copy(), "tensor_mean": tensor_mean, "tensor_acf": c, "shear_acf": shear, "bulk_acf": bulk,
            "eta_shear": eta_s, "eta_bulk": eta_b, "viscosity_shear": float(eta_s[window].mean()), "viscosity_bulk": float(eta_b[window].mean())}


class ThermoObservables:
    """What `MolecularDynamics.run(..., observables=...)` accumulates per structure.  `n_lags` (0: no stress correlations): the
    correlations reach n_lags - 1 samples back; `sample_interval`: MD steps between two samples; `remove_com`: the kinetic tensor
    without its centre-of-mass term, and g = 3 n - 3 in the temperature (also under a run with `fix_com`, which is the default of
    every ensemble but Langevin); `plateau_window`: the part of the lag range (fractions of the
    longest lag) the viscosities are averaged over; `reference_cells`: the cells [S, 3, 3] the strain is measured from (None: the
    starting cells).  Each result dict of the run gains "thermo"."""

    def __init__(self, n_lags: int = 0, sample_interval: int = 1, remove_com: bool = False, plateau_window=(0.5, 1.0), reference_cells=None):
        self.n_lags = integer("n_lags", n_lags, 0)
        if self.n_lags > _lib.THERMO_MAX_LAGS:
            raise ValueError(f"n_lags must be at most {_lib.THERMO_MAX_LAGS}")
        self.sample_interval = integer("sample_interval", sample_interval, 1)
        self.remove_com = boolean("remove_com", remove_com)
        lo, hi = (float(x) for x in plateau_window)
        if not 0.0 <= lo < hi <= 1.0:
            raise ValueError(f"plateau_window must be 0 <= low < high <= 1; got {plateau_window}")
        self.plateau_window = (lo, hi)
        self.reference_cells = None if reference_cells is None else np.asarray(reference_cells, dtype=np.float64)

    def begin(self, lattices, atomic_numbers, masses, device, p_ext=0.0, ensemble: str | None = None, cell_mask: str = "full",
              fix_com: bool = False) -> ThermoState:
        """The device state for these structures.  `p_ext` (eV/A^3, one value or one per structure): the pressure of the run, 0 for
        NVE / NVT; `ensemble` and `cell_mask` decide what `results` derives; `fix_com`: the run holds the total momentum at zero, so
        g = 3 n - 3 whatever `remove_com`.  They stay on the state, not on this object."""
        S = len(atomic_numbers)
        cells = np.stack([np.asarray(L, dtype=np.float64) for L in lattices]) if self.reference_cells is None else self.reference_cells
        if cells.shape != (S, 3, 3):
            raise ValueError(f"reference_cells: expected [{S}, 3, 3]; got {list(cells.shape)}")
        if self.n_lags > 0 and ensemble == "npt_mtk":
            raise ValueError("ThermoObservables(n_lags > 0) is not supported with npt_mtk: its integrator states no pressure tensor")
        offsets = atom_offsets(atomic_numbers)
        state = ThermoState(int(offsets[-1]), offsets, np.concatenate(masses), p_ext, cells, self.n_lags, self.remove_com, device=device)
        state.ensemble, state.cell_mask, state.com_fixed = ensemble, cell_mask, self.remove_com or boolean("fix_com", fix_com)
        return state

    def results(self, state: ThermoState, timestep: float) -> list:
        """One thermo dict per structure from the accumulators of a state `begin` returned (waits for the stream): n_samples,
        n_skipped, flags, the keys of `thermo_from_moments` and, with n_lags > 0, those of `stress_correlations`."""
        acc = state.read()
        out = []
        for s in range(state.S):
            n = int(state.offsets[s + 1] - state.offsets[s])
            res = {"n_samples": int(acc["n_samples"][s]), "n_skipped": int(acc["n_skipped"][s]), "flags": decode_flags(acc["flags"][s])}
            res.update(thermo_from_moments(acc["mean"][s], acc["comoments"][s], res["n_samples"], n, state.ensemble, state.com_fixed,
                                           state.cell_mask))
            if state.lags:
                res.update(stress_correlations(acc["lag_uu"][s], acc["lag_now"][s], acc["lag_old"][s], acc["lag_count"][s], res["v"],
                                               res["t"], self.sample_interval * timestep, self.plateau_window))
            out.append(res)
        return out
