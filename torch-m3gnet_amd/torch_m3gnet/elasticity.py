"""Batched finite-strain elastic constants and equations of state on the device (C ABI: m3g_el_*, csrc/m3g_elastic.hip).

The usual way to get C_ij or E(V) from an M3GNet potential is matcalc's `ElasticityCalc` / `EOSCalc` (pymatgen's
`DeformedStructureSet`) over an ASE calculator: deform a cell, build a graph, evaluate, copy the stress back, 25 times per structure,
then fit in numpy.  `Elasticity.run` and `EquationOfState.run` take a batch of structures instead.  Every deformed copy of every
structure is one row block of a single fp64 `pos` written, with the deformed cells, by one launch (`el_deform`); the copies are
evaluated through the path `Relaxer` uses (`VerletGraph.step` with the pair-virial engine), in sub-batches of copies of one structure,
at most `max_atoms` atoms, optionally relaxing the ions of every copy with the cell fixed (the device FIRE of `torch_m3gnet.relax`);
the fits of the whole batch are one launch each (`el_fit_elastic`, `el_fit_eos`).

Semantics (include/m3gnet_hip.h, "batched finite-strain elastic constants and equation of state"): rows of a lattice are lattice
vectors, a deformation acts on the right (`L' = L D`, `r' = r D`, `D = I + eps`); Voigt order xx, yy, zz, yz, zx, xy; the engine's
pair-virial `stresses` are -(1/V) dE/d eps, so the Cauchy stress (tension positive) is `sigma = -stresses` and everything here is
stated in sigma.  Elastic constants: one Voigt strain component at a time (engineering shear), C_raw[i, j] the slope of the
least-squares line of sigma_i over the magnitudes of component j and the undeformed point.  Equation of state: isotropic linear
strains, third-order Birch-Murnaghan as a linear least-squares cubic in (V / V_ref)^(-2/3) - 1."""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np
import torch

from . import _cuda, _lib
from ._driver import (EV_A3_TO_GPA, Driver, boolean, check_tensor, gpu_device, integer, positive, state_tensor, structure_arrays,
                      sub_batches)
from .data import MaterialGraphKey as K
from .data.graph_gpu import _ptr, _stream
from .data.md import VerletGraph
from .nn.modules import Gradient
from .relax import FireState, fire_loop

NORM_STRAINS = (-0.01, -0.005, 0.005, 0.01)    # matcalc's ElasticityCalc defaults
SHEAR_STRAINS = (-0.06, -0.03, 0.03, 0.06)
EOS_STRAINS = tuple(np.linspace(-0.05, 0.05, 11).tolist())


def _magnitudes(name: str, values, min_distinct: int) -> list:
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    if len(v) == 0 or not np.isfinite(v).all() or (v == 0.0).any() or (np.abs(v) >= _lib.EL_MAX_STRAIN).any():
        raise ValueError(f"{name} must be a non-empty list of finite non-zero magnitudes below {_lib.EL_MAX_STRAIN} in size; got {values}")
    if len(np.unique(v)) < min_distinct:
        raise ValueError(f"{name} must hold at least {min_distinct} distinct magnitudes; got {values}")
    return v.tolist()


def elastic_deformations(norm_strains=NORM_STRAINS, shear_strains=SHEAR_STRAINS):
    """(components, magnitudes) of the elastic strain set: components 0, 1, 2 at every normal magnitude, then 3, 4, 5 at every
    (engineering) shear magnitude."""
    norm, shear = _magnitudes("norm_strains", norm_strains, 2), _magnitudes("shear_strains", shear_strains, 2)
    comp = [j for j in range(3) for _ in norm] + [j for j in range(3, 6) for _ in shear]
    return np.array(comp, dtype=np.int32), np.array(norm * 3 + shear * 3, dtype=np.float64)


def eos_deformations(strains=EOS_STRAINS):
    """(components, magnitudes) of the isotropic strain set: the linear strains but for 0, which is the undeformed copy."""
    v = np.asarray(strains, dtype=np.float64).reshape(-1)
    if not np.isfinite(v).all():
        raise ValueError(f"strains must be finite; got {strains}")
    v = v[np.abs(v) > 1e-14]   # (linspace through zero leaves a rounding residue there)
    mag = _magnitudes("strains", v, 1)
    if 1 + len(np.unique(mag)) < 5:
        raise ValueError("an equation of state needs at least 5 distinct volumes (the undeformed cell counted)")
    return np.full(len(mag), _lib.EL_VOLUMETRIC, dtype=np.int32), np.array(mag, dtype=np.float64)


class ElasticState:
    """The deformed copies of a batch of structures on the device (m3g_el_init).  `lattices` [S] of [3,3] (rows = lattice vectors),
    `positions` [S] of [n_s,3] (Cartesian, A), `components` [M] (Voigt component 0..5 of each deformation, or `_lib.EL_VOLUMETRIC`
    for every one: an equation of state), `magnitudes` [M].  Holds `pos` [rows, 3] and `lat` [copies, 3, 3] float64 (written by
    `el_deform`), `rows_elastic` [S, EL_ROW] / `rows_eos` [S, EL_EOS_ROW] float64 and `nonfinite` / `error` [S] int32 (written by the
    fits).  Copy c of structure s: rows `row_offsets[s] + c n_s ...`, cell `(1 + M) s + c`."""

    def __init__(self, lattices, positions, components, magnitudes, device="cuda"):
        self.S = len(lattices)
        if len(positions) != self.S or self.S == 0:
            raise ValueError("lattices and positions must hold one entry per structure (at least one)")
        self.lattices = np.ascontiguousarray(np.stack([np.asarray(L, dtype=np.float64).reshape(3, 3) for L in lattices]))
        self.positions = np.ascontiguousarray(np.concatenate([np.asarray(p, dtype=np.float64).reshape(-1, 3) for p in positions]))
        self.n_atoms = np.array([len(np.asarray(p).reshape(-1, 3)) for p in positions], dtype=np.int64)
        self.components = np.ascontiguousarray(np.asarray(components, dtype=np.int32).reshape(-1))
        self.magnitudes = np.ascontiguousarray(np.asarray(magnitudes, dtype=np.float64).reshape(-1))
        self.M = len(self.components)
        if len(self.magnitudes) != self.M or not 1 <= self.M <= _lib.EL_MAX_DEFORM:
            raise ValueError(f"components and magnitudes must hold the same number of deformations, 1 to {_lib.EL_MAX_DEFORM}")
        self.mode = _lib.EL_MODE_EOS if (self.components == _lib.EL_VOLUMETRIC).all() else _lib.EL_MODE_ELASTIC
        self._check_arguments()   # (what m3g_el_init checks, before any buffer is made on the device)
        self.offsets = np.concatenate([[0], np.cumsum(self.n_atoms)]).astype(np.int64)
        self.row_offsets = (1 + self.M) * self.offsets
        self.sizes = _lib.M3GElSizes(self.S, int(self.offsets[-1]), self.M, self.mode)
        self.rows, self.copies = int(self.row_offsets[-1]), (1 + self.M) * self.S
        self.device = gpu_device(device, "ElasticState")
        self.lib = _lib.load_library()
        self.state = state_tensor(self.lib.m3g_el_state_bytes, C.byref(self.sizes), device=self.device)
        self.pos = torch.zeros(self.rows, 3, dtype=torch.float64, device=self.device)
        self.lat = torch.zeros(self.copies, 3, 3, dtype=torch.float64, device=self.device)
        self.rows_elastic = torch.full((self.S, _lib.EL_ROW), float("nan"), dtype=torch.float64, device=self.device)
        self.rows_eos = torch.full((self.S, _lib.EL_EOS_ROW), float("nan"), dtype=torch.float64, device=self.device)
        self.nonfinite = torch.zeros(self.S, dtype=torch.int32, device=self.device)
        self.error = torch.zeros(self.S, dtype=torch.int32, device=self.device)
        with _cuda.on_device(self.device):
            _lib.check(self.lib.m3g_el_init(C.byref(self.sizes), self.offsets.ctypes.data, self.lattices.ctypes.data,
                                            self.positions.ctypes.data, self.components.ctypes.data, self.magnitudes.ctypes.data,
                                            _ptr(self.state), self.state.numel(), _stream()))

    def _check_arguments(self) -> None:
        if (self.n_atoms < 1).any():
            raise ValueError("every structure must hold an atom")
        if not (np.isfinite(self.lattices).all() and np.isfinite(self.positions).all()):
            raise ValueError("non-finite lattice or positions")
        if (np.abs(np.linalg.det(self.lattices)) < 1e-12).any():
            raise ValueError("singular lattice")
        d, c = self.magnitudes, self.components
        if not np.isfinite(d).all() or (d == 0.0).any() or (np.abs(d) >= _lib.EL_MAX_STRAIN).any():
            raise ValueError(f"magnitudes must be finite, non-zero and below {_lib.EL_MAX_STRAIN} in size")
        if self.mode == _lib.EL_MODE_EOS:
            if 1 + len(np.unique(d)) < 5:
                raise ValueError("an equation of state needs at least 5 distinct volumes (the undeformed cell counted)")
        else:
            if ((c < 0) | (c > 5)).any():
                raise ValueError(f"components must be Voigt indices 0..5, or {_lib.EL_VOLUMETRIC} for every deformation")
            if any(len(np.unique(d[c == j])) < 2 for j in range(6)):
                raise ValueError("every Voigt component needs at least two distinct magnitudes")


def el_deform(state: ElasticState):
    """Positions of every row and cells of every copy of the deformed batch (m3g_el_deform), written to and returned as
    (`state.pos`, `state.lat`).  Queued on the current stream; no wait, capture-safe."""
    with _cuda.on_device(state.device):
        _lib.check(state.lib.m3g_el_deform(C.byref(state.sizes), _ptr(state.state), state.state.numel(), _ptr(state.pos), _ptr(state.lat),
                                           _stream()))
    return state.pos, state.lat


def el_fit_elastic(state: ElasticState, stresses: torch.Tensor) -> torch.Tensor:
    """Elastic tensors and moduli of every structure (m3g_el_fit_elastic) from the engine's pair-virial `stresses` [copies, 6] float32
    of the deformed batch: written to and returned as `state.rows_elastic` (layout: M3G_EL_ROW_*); `state.nonfinite` too.  Queued on
    the current stream; no wait, capture-safe."""
    check_tensor("stresses", stresses, (state.copies, 6), torch.float32, state.pos.device)
    with _cuda.on_device(state.device):
        _lib.check(state.lib.m3g_el_fit_elastic(C.byref(state.sizes), _ptr(state.state), state.state.numel(), _ptr(stresses),
                                                _ptr(state.rows_elastic), _ptr(state.nonfinite), _stream()))
    return state.rows_elastic


def el_fit_eos(state: ElasticState, energies: torch.Tensor) -> torch.Tensor:
    """Birch-Murnaghan fits of every structure (m3g_el_fit_eos) from the total `energies` [copies] float32 of the deformed batch:
    written to and returned as `state.rows_eos` (v0, e0, b0, b0', rms residual, v_ref, t0, points); `state.error` too.  Queued on the
    current stream; no wait, capture-safe."""
    check_tensor("energies", energies, (state.copies,), torch.float32, state.pos.device)
    with _cuda.on_device(state.device):
        _lib.check(state.lib.m3g_el_fit_eos(C.byref(state.sizes), _ptr(state.state), state.state.numel(), _ptr(energies),
                                            _ptr(state.rows_eos), _ptr(state.error), _stream()))
    return state.rows_eos


class ElasticResult:
    """Elastic constants of one structure at the given cell, eV/A^3 (`*_gpa`: GPa).  `C_raw` [6,6] (C_raw[i, j] = d sigma_i / d eps_j,
    Voigt order xx yy zz yz zx xy, engineering shear), `C` its symmetric part, `compliance` = C^-1, `asymmetry` = max |C_raw -
    C_raw^T|, `residual_stress` [6] (sigma of the undeformed cell), `fit_residual` (largest residual of the 36 lines), `k_voigt`,
    `k_reuss`, `k_hill`, `g_voigt`, `g_reuss`, `g_hill`, `youngs_modulus`, `poisson_ratio` (from the Hill values),
    `universal_anisotropy`, `eigenvalues` [6] of C and `stable` (all > 0); `sigma` [1 + M, 6] (the Cauchy stress of every copy, minus the engine's `stresses`), `energies`
    [1 + M], `n_unconverged` (copies whose ions did not reach fmax), `converged`, `error` (a non-finite stress, or a copy whose
    relaxation failed: the tensor is NaN in the first case).

    This is the stress-strain tensor pymatgen / matcalc report.  It equals the thermodynamic second derivative of the energy with
    respect to strain only at zero `residual_stress`."""

    def __init__(self, row: np.ndarray, nonfinite: int, sigma: np.ndarray, energies: np.ndarray, n_unconverged: int, fire_error: bool):
        self.C_raw, self.C, self.compliance = (row[a:a + 36].reshape(6, 6).copy() for a in (0, 36, 72))
        self.residual_stress, self.eigenvalues = row[108:114].copy(), row[114:120].copy()
        (self.asymmetry, self.fit_residual, self.k_voigt, self.k_reuss, self.k_hill, self.g_voigt, self.g_reuss, self.g_hill,
         self.youngs_modulus, self.poisson_ratio, self.universal_anisotropy) = (float(x) for x in row[120:131])
        self.stable = bool(row[131] == 1.0)
        self.sigma, self.energies = sigma, energies
        self.n_unconverged = int(n_unconverged)
        self.converged = self.n_unconverged == 0
        self.error = bool(nonfinite != 0 or fire_error)
        for name in ("C_raw", "C", "residual_stress", "eigenvalues", "k_voigt", "k_reuss", "k_hill", "g_voigt", "g_reuss", "g_hill",
                     "youngs_modulus"):
            setattr(self, name + "_gpa", getattr(self, name) * EV_A3_TO_GPA)


class EosResult:
    """Third-order Birch-Murnaghan equation of state of one structure: `v0` (A^3), `e0` (eV), `b0` (eV/A^3; `b0_gpa`), `b0_prime`,
    `rms_residual` (eV), `volumes` / `energies` [1 + M] (copy 0 first), `error` (`no_minimum`: the fitted curve has no minimum inside
    the sampled volumes; `nonfinite`: an energy is not finite), `n_unconverged` / `converged` as in `ElasticResult`."""

    def __init__(self, row: np.ndarray, error: int, volumes: np.ndarray, energies: np.ndarray, n_unconverged: int, fire_error: bool):
        self.v0, self.e0, self.b0, self.b0_prime, self.rms_residual = (float(x) for x in row[:5])
        self.b0_gpa = self.b0 * EV_A3_TO_GPA
        self.volumes, self.energies = volumes, energies
        self.error_bits = int(error)
        self.no_minimum, self.nonfinite = bool(error & _lib.EL_EOS_NO_MINIMUM), bool(error & _lib.EL_EOS_NONFINITE)
        self.n_unconverged = int(n_unconverged)
        self.converged = self.n_unconverged == 0
        self.error = bool(error != 0 or fire_error)


class _StrainDriver(Driver):
    """What `Elasticity` and `EquationOfState` share: the arguments and the evaluation of the deformed batch."""

    def __init__(self, model: Gradient, relax_atoms: bool, fmax: float, steps: int, max_atoms: int, skin: float, device):
        super().__init__(model, skin, device)
        self.relax_atoms, self.fmax = boolean("relax_atoms", relax_atoms), positive("fmax", fmax)
        self.steps, self.max_atoms = integer("steps", steps, 0), integer("max_atoms", max_atoms, 1)

    def _evaluate(self, st: ElasticState, z: Sequence[np.ndarray]):
        """Energies [copies], pair-virial stresses [copies, 6] (float32, device) and FIRE flags [copies] (host) of the deformed batch
        at `st.pos` / `st.lat`; with `relax_atoms` the ions of every copy are relaxed in place in `st.pos` first."""
        model, dev = self.model, self.device
        cfg = model.engine.cfg
        host_lat = st.lat.cpu().numpy()   # (waits for el_deform: the candidate search needs the deformed cells on the host)
        energies = torch.empty(st.copies, dtype=torch.float32, device=st.pos.device)
        stresses = torch.empty(st.copies, 6, dtype=torch.float32, device=st.pos.device)
        flags = np.full(st.copies, _lib.FIRE_CONVERGED, dtype=np.int32)
        n_copies = 1 + st.M
        for s in range(st.S):   # the copies in row order, structure by structure (`sub_batches`, as Phonons.run)
            n = int(st.n_atoms[s])
            for c0, nc in sub_batches(n_copies, n, self.max_atoms):
                k0 = n_copies * s + c0
                r0 = int(st.row_offsets[s]) + c0 * n
                pos = st.pos[r0:r0 + nc * n]
                vg = VerletGraph(list(host_lat[k0:k0 + nc]), [z[s]] * nc, cfg.cutoff, cfg.threebody_cutoff, skin=self.skin, device=dev)
                if not self.relax_atoms:
                    out = vg.step(model, pos)
                else:   # the fixed-cell loop of Relaxer.relax over the copies of this sub-batch
                    fire = FireState(pos, vg.lattice.clone(), np.arange(nc + 1) * n, relax_cell=False, fmax=self.fmax)
                    out = fire_loop(vg, model, fire, self.steps)
                    flags[k0:k0 + nc] = fire.read()["flags"]
                vg.raise_on_step_errors("elasticity")
                energies[k0:k0 + nc] = out[K.TOTAL_ENERGY].reshape(-1)
                stresses[k0:k0 + nc] = out[K.STRESSES]
        return energies, stresses, flags

    def _prepare(self, lattices, positions, atomic_numbers, components, magnitudes):
        lat, pos, z = structure_arrays(lattices, positions, atomic_numbers)
        st = ElasticState(lat, pos, components, magnitudes, device=self.device)
        el_deform(st)
        energies, stresses, flags = self._evaluate(st, z)
        flags = flags.reshape(st.S, 1 + st.M)
        unconverged = ((flags & _lib.FIRE_CONVERGED) == 0).sum(axis=1)
        fire_error = ((flags & _lib.FIRE_ERROR) != 0).any(axis=1)
        return st, energies, stresses, unconverged, fire_error


class Elasticity(_StrainDriver):
    """Batched elastic constants under an M3GNet potential.

    `model`: the `Gradient` returned by `build_model` (evaluated, like `Relaxer`'s, through a pair-virial engine made from its
    `Sequential`).  `norm_strains` / `shear_strains`: magnitudes of the normal and (engineering) shear strains, each applied to its
    three Voigt components (defaults: matcalc's).  `relax_atoms`: relax the ions of every deformed copy with the cell fixed (FIRE to
    `fmax` eV/A within `steps`; the default 0.01 is tighter than a structure search's because a strain derivative needs it) or keep
    them clamped.  `max_atoms`: atoms per engine sub-batch (whole copies of one structure; a copy larger than it is evaluated alone).
    A structure's results are bitwise the same alone or in any batch for a given `max_atoms`; a different `max_atoms` can change the
    engine's sub-batches and so the last bits of its stresses.  The structures should be relaxed first: see `ElasticResult`."""

    def __init__(self, model: Gradient, norm_strains=NORM_STRAINS, shear_strains=SHEAR_STRAINS, relax_atoms: bool = True, fmax: float = 0.01,
                 steps: int = 500, max_atoms: int = 200_000, skin: float = 0.5, device="cuda"):
        super().__init__(model, relax_atoms, fmax, steps, max_atoms, skin, device)
        self.components, self.magnitudes = elastic_deformations(norm_strains, shear_strains)

    def run(self, lattices: Sequence, positions: Sequence, atomic_numbers: Sequence) -> list:
        """Elastic constants of every structure (lattices [3,3] rows = lattice vectors, positions [n_s,3] Cartesian, atomic_numbers
        [n_s]).  Returns one `ElasticResult` per structure.  A copy whose ions do not converge is counted in `n_unconverged`: the
        fit is still made from the stresses where it stopped."""
        st, energies, stresses, unconverged, fire_error = self._prepare(lattices, positions, atomic_numbers, self.components, self.magnitudes)
        rows = el_fit_elastic(st, stresses).cpu().numpy()
        bad = st.nonfinite.cpu().numpy()
        sigma = -stresses.double().cpu().numpy().reshape(st.S, 1 + st.M, 6)
        e = energies.double().cpu().numpy().reshape(st.S, 1 + st.M)
        self.state = st   # (the deformed batch, kept for inspection)
        return [ElasticResult(rows[s], int(bad[s]), sigma[s], e[s], unconverged[s], bool(fire_error[s])) for s in range(st.S)]


class EquationOfState(_StrainDriver):
    """Batched third-order Birch-Murnaghan equations of state under an M3GNet potential.  `strains`: linear strains of the isotropic
    deformations (default 11 points over +-5 %; 0 is the undeformed copy and is not repeated).  The other arguments: see
    `Elasticity`.  Where a model's energy is not smooth as a neighbour shell crosses its cutoff, keep the strains inside the range in
    which none does: a curve through such a step is no equation of state (`rms_residual` shows it)."""

    def __init__(self, model: Gradient, strains=EOS_STRAINS, relax_atoms: bool = True, fmax: float = 0.01, steps: int = 500,
                 max_atoms: int = 200_000, skin: float = 0.5, device="cuda"):
        super().__init__(model, relax_atoms, fmax, steps, max_atoms, skin, device)
        self.components, self.magnitudes = eos_deformations(strains)

    def run(self, lattices: Sequence, positions: Sequence, atomic_numbers: Sequence) -> list:
        """Equation of state of every structure.  Returns one `EosResult` per structure."""
        st, energies, _, unconverged, fire_error = self._prepare(lattices, positions, atomic_numbers, self.components, self.magnitudes)
        rows = el_fit_eos(st, energies).cpu().numpy()
        err = st.error.cpu().numpy()
        vol = np.abs(np.linalg.det(st.lat.cpu().numpy())).reshape(st.S, 1 + st.M)
        e = energies.double().cpu().numpy().reshape(st.S, 1 + st.M)
        self.state = st
        return [EosResult(rows[s], int(err[s]), vol[s], e[s], unconverged[s], bool(fire_error[s])) for s in range(st.S)]
