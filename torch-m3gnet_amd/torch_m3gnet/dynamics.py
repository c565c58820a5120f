"""Batched molecular dynamics on the device: NVE, NVT (Berendsen, Langevin) and isotropic NPT Berendsen (C ABI: m3g_dyn_*,
csrc/m3g_dynamics.hip), and the deterministic, time-reversible ensembles with a conserved quantity, Nose-Hoover chain NVT and
isotropic Martyna-Tobias-Klein NPT (C ABI: m3g_nhc_*, csrc/m3g_nhc.hip), and the flexible-cell Martyna-Tobias-Klein NPT whose cell
changes shape as well as size (C ABI: m3g_mtk_*, csrc/m3g_mtk.hip).

The m3gnet package the reference stands in for runs MD through `MolecularDynamics` (ASE's VelocityVerlet "nve", NVTBerendsen "nvt",
NPTBerendsen "npt_berendsen") on one structure at a time.  `MolecularDynamics.run` takes a whole batch: every structure is integrated
on its own, with its own target temperature and its own random stream, and its numbers are bitwise the same alone or in any batch.
Per step the energies, forces and (pair-virial) stresses come from `VerletGraph.step` -- whose skin-test verdict is the loop's only
wait -- and the integrator of the whole batch is three kernel launches (`dyn_step`); the host copies observables only on log steps.
NPT moves the cells at every step, so the candidates are searched again at every step (`VerletGraph.set_lattice`), as in the
variable-cell `Relaxer`.  The two deterministic ensembles run the same loop over an `NhcState` / `nhc_step` pair shaped like
`DynState` / `dyn_step`, and the flexible-cell one over `MtkCellState` / `mtk_cell_step`.

Units: A, fs, amu, eV; velocities in A/fs; `MolecularDynamics` takes the pressure in GPa and the compressibility in 1/GPa (ASE's
NPTBerendsen convention), the C ABI in eV/A^3 and A^3/eV."""
from __future__ import annotations

import math
from typing import Sequence

import numpy as np
import torch

from . import _lib
from ._driver import (EV_A3_TO_GPA, Driver, IntegratorState, MdBatch, MdLog, integer, md_loop, md_results, non_negative, per_structure,
                      positive, state_tensor, structure_arrays, structure_masses, structure_seeds)
from .data import MaterialGraphKey as K
from .nn.modules import Gradient
from .local_order import LocalOrderObservables, lo_sample
from .scattering import ScatteringObservables, sq_sample
from .thermo import ThermoObservables, thermo_sample
from .trajectory import TrajectoryObservables, traj_sample

KAPPA = 9.648533215665e-3    # A/fs^2 per eV/(A amu)
KB = 8.617333262e-5          # eV/K
EV_PER_A3_IN_GPA = EV_A3_TO_GPA
ENSEMBLES = {"nve": _lib.DYN_NVE, "nvt_berendsen": _lib.DYN_NVT_BERENDSEN, "nvt_langevin": _lib.DYN_NVT_LANGEVIN,
             "npt_berendsen": _lib.DYN_NPT_BERENDSEN}
NHC_ENSEMBLES = {"nvt_nose_hoover": _lib.NHC_NVT, "npt_mtk": _lib.NHC_NPT_MTK}   # the m3g_nhc_* family
CELL_MASKS = {"full": _lib.MTK_CELL_FULL, "orthorhombic": _lib.MTK_CELL_ORTHORHOMBIC}
MTK_CELL_ENSEMBLES = {"npt_mtk_cell": CELL_MASKS}   # the m3g_mtk_* family: one ensemble, its `cell_mask` values


def maxwell_boltzmann(masses, temperature: float, seed: int = 0) -> np.ndarray:
    """Velocities [n, 3] (A/fs, host numpy) of one structure drawn from the Maxwell-Boltzmann distribution at `temperature` (K), seeded,
    with zero total momentum and rescaled to exactly `temperature` (3n degrees of freedom, as ASE's get_temperature).  A single atom,
    or T = 0, gets zero velocity."""
    m = np.asarray(masses, dtype=np.float64).reshape(-1)
    temperature = float(temperature)
    if not (math.isfinite(temperature) and temperature >= 0.0) or not (np.isfinite(m).all() and (m > 0).all()):
        raise ValueError("maxwell_boltzmann needs a finite temperature >= 0 and finite masses > 0")
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(len(m), 3)) * np.sqrt(KB * temperature * KAPPA / m)[:, None]
    v -= (m[:, None] * v).sum(0) / m.sum()
    t_now = (m * (v * v).sum(1)).sum() / KAPPA / (3.0 * len(m) * KB)
    if temperature == 0.0 or t_now == 0.0:
        return np.zeros_like(v)
    return v * np.sqrt(temperature / t_now)


class DynState(IntegratorState):
    """MD state of a batch on the device (m3g_dyn_init): masses, velocities (fp64), target temperatures, seeds, flags and step counts.
    `pos` ([N,3] fp64, unwrapped) and `lattice` ([S,3,3] fp64, may be None except in NPT) are the caller's tensors: `dyn_step` moves
    them IN PLACE (and `lattice32`, their fp32 copy).  The `velocities` ARGUMENT [N,3] fp64 device holds the starting velocities: copied.  `offsets`: S + 1 atom offsets, strictly
    increasing.  Parameters in the C ABI's units: dt, taut, taup in fs, friction in 1/fs, pressure in eV/A^3, compressibility in
    A^3/eV.  `obs` [S,4] (KE eV, T K, P eV/A^3, V A^3) is written by every `dyn_step`.  The `velocities` ATTRIBUTE is not the
    argument: it is a live [N,3] fp64 view into the state buffer, the integrator's own velocities on the device (between two
    `dyn_step` calls the half-step velocities of the step under way), which every `dyn_step` changes."""
    FAMILY, OBS, CELLS, SECOND = "dyn", 4, True, ("stresses", (6,), None)

    def __init__(self, pos: torch.Tensor, lattice: torch.Tensor | None, offsets: Sequence[int], masses, velocities: torch.Tensor,
                 temperatures, seeds, ensemble: str = "nve", dt: float = 1.0, taut: float = 100.0, friction: float = 0.01,
                 pressure: float = 0.0, taup: float = 1000.0, compressibility: float = 1.0, fix_com: bool = False):
        if ensemble not in ENSEMBLES:
            raise ValueError(f"unknown ensemble {ensemble!r}; expected one of {sorted(ENSEMBLES)}")
        self.ensemble = ensemble
        self.params = _lib.M3GDynParams(ensemble=ENSEMBLES[ensemble], fix_com=1 if fix_com else 0, dt=dt, taut=taut, friction=friction,
                                        pressure=pressure, taup=taup, compressibility=compressibility)
        self._layout(pos, lattice, offsets)
        if ensemble == "npt_berendsen" and lattice is None:
            raise ValueError("NPT needs the lattice")
        self._rows("velocities", velocities)
        if not self._host_arrays(masses, temperatures, seeds):
            raise ValueError(f"expected {self.N} masses and {self.S} seeds")
        self._allocate(state_tensor, self.N, self.S)
        self._init(self.temperatures, self.seeds, velocities)

    def _fields(self):
        """`read()`: flags / n_steps [S] and the velocities [N, 3], copied to the host (waits for the stream)."""
        return ("flags", np.int32, self.S), ("n_steps", np.int64, self.S), ("v", np.float64, (self.N, 3))


def dyn_step(state: DynState, forces: torch.Tensor, stresses: torch.Tensor | None = None, finish_only: bool = False) -> None:
    """One MD call of the batch (m3g_dyn_step) at `forces` [N,3] and `stresses` [S,6] (float32, pair-virial convention; required in
    NPT) evaluated at `state.pos`: finish the step that ends here, write `state.obs`, start the next one (not with `finish_only`).
    Queued on the current stream; no wait, capture-safe."""
    state.step(forces, finish_only, stresses)


def langevin_warm_up(batch: MdBatch, masses: list, temperature: float, seeds, equilibration: int, **common) -> DynState:
    """`equilibration` Langevin steps of `batch` from Maxwell-Boltzmann velocities (`masses`: [n_s] per structure; `common`: dt and
    friction): the `DynState`, ended on full-step velocities, which seed the run proper (`velocities=warm.velocities`: copied on the
    device)."""
    vel = [maxwell_boltzmann(ms, temperature, int(sd)) for ms, sd in zip(masses, seeds)]
    warm = DynState(batch.pos, batch.lattice, batch.offsets, np.concatenate(masses), torch.tensor(np.concatenate(vel), device=batch.device),
                    temperature, seeds, ensemble="nvt_langevin", **common)
    md_loop(batch, warm, equilibration)
    return warm


class NhcState(IntegratorState):
    """State of a Nose-Hoover chain NVT ("nvt_nose_hoover") or MTK NPT ("npt_mtk") batch on the device (m3g_nhc_init), shaped like
    `DynState`: `pos` [N,3] fp64 and `lattice` [S,3,3] fp64 (may be None in NVT) are the caller's tensors, moved IN PLACE by `nhc_step`
    (with `lattice32`, the fp32 copy of the cells); the `velocities` argument is copied, the `velocities` attribute is the live
    [N,3] fp64 view of the integrator's own.  dt, taut, taup in fs, pressure in eV/A^3; `chain_length` thermostats per chain (1 .. 8)
    and `chain_substeps` equal parts of every chain half-step (1 .. 8).  Every temperature must be > 0: the chain masses are
    proportional to it.  `obs` [S,6] (KE eV, T K, P eV/A^3, V A^3, extended eV, 0) is written by every `nhc_step`; T = 2 KE / (3 n kB)
    as in the other ensembles, so its canonical mean is T0 g / (3 n) with g = 3 n - 3 under `fix_com`.  E_pot + KE + extended is
    the conserved quantity."""
    FAMILY, OBS, CELLS, SECOND = "nhc", _lib.NHC_OBS, True, ("stresses", (6,), None)

    def __init__(self, pos: torch.Tensor, lattice: torch.Tensor | None, offsets: Sequence[int], masses, velocities: torch.Tensor,
                 temperatures, ensemble: str = "nvt_nose_hoover", dt: float = 1.0, taut: float = 100.0, pressure: float = 0.0,
                 taup: float = 1000.0, chain_length: int = 3, chain_substeps: int = 1, fix_com: bool = True):
        if ensemble not in NHC_ENSEMBLES:
            raise ValueError(f"unknown ensemble {ensemble!r}; expected one of {sorted(NHC_ENSEMBLES)}")
        self.ensemble = ensemble
        self.chain_length = chain_count("chain_length", chain_length)
        self.params = _lib.M3GNhcParams(ensemble=NHC_ENSEMBLES[ensemble], fix_com=1 if fix_com else 0, chain_length=self.chain_length,
                                        chain_substeps=chain_count("chain_substeps", chain_substeps), dt=dt, taut=taut, pressure=pressure,
                                        taup=taup)
        self._layout(pos, lattice, offsets)
        if ensemble == "npt_mtk" and lattice is None:
            raise ValueError("NPT needs the lattice")
        self._rows("velocities", velocities)
        if not self._host_arrays(masses, temperatures):
            raise ValueError(f"expected {self.N} masses")
        self._allocate(state_tensor, self.N, self.S, self.chain_length)
        self._init(self.temperatures, velocities)

    def _fields(self):
        """`read()`: flags / n_steps [S], the velocities [N, 3] and the chain rows [S, 4 M + 1] (xi, vxi, xib, vxib of the M
        thermostats, then veps), copied to the host (waits for the stream)."""
        return (("flags", np.int32, self.S), ("n_steps", np.int64, self.S), ("v", np.float64, (self.N, 3)),
                ("chain", np.float64, (self.S, 4 * self.chain_length + 1)))


def nhc_step(state: NhcState, forces: torch.Tensor, stresses: torch.Tensor | None = None, finish_only: bool = False) -> None:
    """One MD call of the batch (m3g_nhc_step), the arguments of `dyn_step`: finish the step that ends at these forces, write
    `state.obs`, start the next one (not with `finish_only`).  Three launches, queued on the current stream; no wait, capture-safe."""
    state.step(forces, finish_only, stresses)


class MtkCellState(IntegratorState):
    """State of a flexible-cell MTK NPT ("npt_mtk_cell") batch on the device (m3g_mtk_init), shaped like `NhcState`: `pos` [N,3] fp64
    and `lattice` [S,3,3] fp64 (triclinic cells welcome) are the caller's tensors, moved IN PLACE by `mtk_cell_step` (with `lattice32`,
    the fp32 copy of the cells); the `velocities` argument is copied, the `velocities` attribute is the live [N,3] fp64 view of the
    integrator's own.  `cell_mask`: "full" (all six components of the symmetric cell rate move) or "orthorhombic" (its diagonal
    only: for cells whose vectors lie along the axes).  dt, taut, taup in fs, pressure (hydrostatic) in eV/A^3; chains as `NhcState`.
    `obs` [S,12] (KE eV, T K, P eV/A^3, V A^3, extended eV, 0, then the pressure tensor in Voigt order xx, yy, zz, yz, zx, xy) is
    written by every `mtk_cell_step`; E_pot + KE + extended is the conserved quantity.  A structure whose cell rate times dt passes
    0.05 is flagged like one with non-finite forces or stresses, and frozen."""
    FAMILY, OBS, CELLS, SECOND = "mtk", _lib.MTK_OBS, True, ("stresses", (6,), "npt_mtk_cell needs the stresses")

    def __init__(self, pos: torch.Tensor, lattice: torch.Tensor, offsets: Sequence[int], masses, velocities: torch.Tensor, temperatures,
                 cell_mask: str = "full", dt: float = 1.0, taut: float = 100.0, pressure: float = 0.0, taup: float = 1000.0,
                 chain_length: int = 3, chain_substeps: int = 1, fix_com: bool = True):
        self.cell_mask = cell_mask_name(cell_mask)
        self.ensemble = "npt_mtk_cell"
        self.chain_length = chain_count("chain_length", chain_length)
        self.params = _lib.M3GMtkParams(cell_mask=CELL_MASKS[self.cell_mask], fix_com=1 if fix_com else 0, chain_length=self.chain_length,
                                        chain_substeps=chain_count("chain_substeps", chain_substeps), dt=dt, taut=taut, pressure=pressure,
                                        taup=taup)
        if lattice is None:
            raise ValueError("NPT needs the lattice")
        self._layout(pos, lattice, offsets)
        self._rows("velocities", velocities)
        if not self._host_arrays(masses, temperatures):
            raise ValueError(f"expected {self.N} masses")
        self._allocate(state_tensor, self.N, self.S, self.chain_length)
        self._init(self.temperatures, velocities)

    def _fields(self):
        """`read()`: flags / n_steps [S], the velocities [N, 3] and the chain rows [S, 4 M + 6] (xi, vxi, xib, vxib of the M
        thermostats, then the six components of the cell rate vg), copied to the host (waits for the stream)."""
        return (("flags", np.int32, self.S), ("n_steps", np.int64, self.S), ("v", np.float64, (self.N, 3)),
                ("chain", np.float64, (self.S, 4 * self.chain_length + 6)))


def mtk_cell_step(state: MtkCellState, forces: torch.Tensor, stresses: torch.Tensor, finish_only: bool = False) -> None:
    """One MD call of the batch (m3g_mtk_step), the arguments of `nhc_step` (the stresses are required): finish the step that ends
    at these forces, write `state.obs`, start the next one (not with `finish_only`).  Three launches, queued on the current stream;
    no wait, capture-safe."""
    state.step(forces, finish_only, stresses)


def cell_mask_name(x) -> str:
    """`cell_mask`: "full" or "orthorhombic"."""
    if not isinstance(x, str) or x not in CELL_MASKS:
        raise ValueError(f"unknown cell_mask {x!r}; expected one of {sorted(CELL_MASKS)}")
    return x


def chain_count(name: str, x) -> int:
    """`chain_length` / `chain_substeps`: an integer in 1 .. 8."""
    if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or not 1 <= x <= _lib.NHC_MAX_CHAIN:
        raise ValueError(f"{name} must be an integer in 1 .. {_lib.NHC_MAX_CHAIN}; got {x!r}")
    return int(x)


def _split_observables(observables):
    """(TrajectoryObservables or None, ScatteringObservables or None) of the `observables` argument of `MolecularDynamics.run`: one
    object, or a list / tuple holding at most one of each kind."""
    found = {TrajectoryObservables: None, ScatteringObservables: None}
    items = observables if isinstance(observables, (list, tuple)) else () if observables is None else (observables,)
    for item in items:
        kind = next((k for k in found if isinstance(item, k)), None)
        if kind is None or found[kind] is not None:
            raise TypeError("observables must be a TrajectoryObservables, a ScatteringObservables, or a list holding at most one of each; "
                            f"got {'a second ' if kind else ''}{type(item).__name__}")
        found[kind] = item
    return found[TrajectoryObservables], found[ScatteringObservables]


def _take_local_order(observables):
    """(LocalOrderObservables or None, what is left of the `observables` argument for `_split_observables`): at most one of them, alone
    or anywhere in the list / tuple."""
    if isinstance(observables, LocalOrderObservables):
        return observables, None
    if not isinstance(observables, (list, tuple)):
        return None, observables
    mine = [item for item in observables if isinstance(item, LocalOrderObservables)]
    if len(mine) > 1:
        raise TypeError("observables must hold at most one of each kind; got a second LocalOrderObservables")
    return (mine[0] if mine else None), [item for item in observables if not isinstance(item, LocalOrderObservables)]


def _take_thermo(observables):
    """(ThermoObservables or None, what is left of the `observables` argument for `_take_local_order`): at most one of them, alone or
    anywhere in the list / tuple."""
    if isinstance(observables, ThermoObservables):
        return observables, None
    if not isinstance(observables, (list, tuple)):
        return None, observables
    mine = [item for item in observables if isinstance(item, ThermoObservables)]
    if len(mine) > 1:
        raise TypeError("observables must hold at most one of each kind; got a second ThermoObservables")
    return (mine[0] if mine else None), [item for item in observables if not isinstance(item, ThermoObservables)]


class MolecularDynamics(Driver):
    """Batched counterpart of m3gnet's `MolecularDynamics`.

    `model`: the `Gradient` returned by `build_model`; the run evaluates a `pair_virial=True` engine made from its `Sequential` (the
    pressure needs the strain derivative).  ensemble: "nvt_langevin" (BAOAB with `friction`, 1/fs), "nve", "nvt_berendsen" (`taut`, fs)
    "npt_berendsen" (`taut`, `taup`, `pressure` in GPa, `compressibility` in 1/GPa -- required), "nvt_nose_hoover" (a Nose-Hoover
    chain of `chain_length` thermostats of period `taut`, every chain half-step in `chain_substeps` equal parts) or "npt_mtk" (the
    isotropic Martyna-Tobias-Klein barostat of period `taup` at `pressure`, with a chain on the particles and one on the barostat; no
    compressibility), or "npt_mtk_cell" (the fully flexible Martyna-Tobias-Klein barostat: the same parameters as "npt_mtk" and
    `cell_mask`, "full" -- the cell changes shape as well as size, all six components of its symmetric rate move -- or
    "orthorhombic" -- its three lengths move independently, for cells whose vectors lie along the axes; the pressure is hydrostatic
    only; a symmetric rate does not forbid a slow rigid rotation of the cell, which the physics does not see).  The last three are deterministic and time-reversible, sample the canonical and the isothermal-isobaric
    ensemble, need every temperature > 0, and their log gains `conserved` (eV): e_pot + ke + the thermostat and barostat terms,
    constant up to the O(timestep^2) error of the integrator ("npt_mtk_cell" also `pressure_tensor` [6], GPa in Voigt order xx, yy,
    zz, yz, zx, xy, and `lattice` [3,3] per logged step).  Their `t` is 2 KE / (3 n kB) like the others', so its canonical mean
    is temperature * g / (3 n) with g = 3 n - 3 under `fix_com`.  `temperature`: K, one value or one per structure (the target of
    the thermostats and the temperature of the starting velocities).  `fix_com` (zero the total momentum at every step) defaults to
    True where the ensemble allows it (not with Langevin).  `seed`: an integer, or one per structure."""

    def __init__(self, model: Gradient, ensemble: str = "nvt_langevin", timestep: float = 1.0, temperature=300.0, taut: float | None = None,
                 friction: float = 0.01, pressure: float = 0.0, taup: float | None = None, compressibility: float | None = None,
                 fix_com: bool | None = None, skin: float = 0.5, seed=0, device="cuda", chain_length: int = 3, chain_substeps: int = 1,
                 cell_mask: str = "full"):
        super().__init__(model, skin, device)
        known = sorted(ENSEMBLES) + sorted(NHC_ENSEMBLES) + sorted(MTK_CELL_ENSEMBLES)
        if not isinstance(ensemble, str) or ensemble not in known:
            raise ValueError(f"unknown ensemble {ensemble!r}; expected one of {known}")
        self.ensemble = ensemble
        self.cell_mask = cell_mask_name(cell_mask)
        self.chain_length, self.chain_substeps = chain_count("chain_length", chain_length), chain_count("chain_substeps", chain_substeps)
        self.timestep = positive("timestep", timestep)
        self.taut = positive("taut", 100.0 * self.timestep if taut is None else taut)
        self.taup = positive("taup", 1000.0 * self.timestep if taup is None else taup)
        self.friction = non_negative("friction", friction)
        self.pressure = float(pressure)
        if not math.isfinite(self.pressure):
            raise ValueError(f"pressure must be finite; got {self.pressure}")
        if ensemble == "npt_berendsen":
            if compressibility is None:
                raise ValueError("npt_berendsen needs the compressibility (1/GPa)")
            compressibility = positive("compressibility", compressibility)
        self.compressibility = compressibility
        if fix_com is None:
            fix_com = ensemble != "nvt_langevin"
        if fix_com and ensemble == "nvt_langevin":
            raise ValueError("fix_com is not supported with the Langevin thermostat")
        self.fix_com = bool(fix_com)
        t = np.asarray(temperature, dtype=np.float64)
        if t.ndim > 1 or not (np.isfinite(t).all() and (t >= 0).all()):
            raise ValueError("temperature must be one finite value >= 0 (K) or one per structure")
        if (ensemble in NHC_ENSEMBLES or ensemble in MTK_CELL_ENSEMBLES) and not (t > 0).all():
            raise ValueError(f"{ensemble} needs every temperature > 0 (the thermostat masses are proportional to it)")
        self.temperature = t
        self.seed = seed

    def _params(self) -> dict:
        if self.ensemble in MTK_CELL_ENSEMBLES:
            return dict(cell_mask=self.cell_mask, dt=self.timestep, taut=self.taut, pressure=self.pressure / EV_PER_A3_IN_GPA, taup=self.taup,
                        chain_length=self.chain_length, chain_substeps=self.chain_substeps, fix_com=self.fix_com)
        if self.ensemble in NHC_ENSEMBLES:
            return dict(ensemble=self.ensemble, dt=self.timestep, taut=self.taut, pressure=self.pressure / EV_PER_A3_IN_GPA, taup=self.taup,
                        chain_length=self.chain_length, chain_substeps=self.chain_substeps, fix_com=self.fix_com)
        beta = 1.0 if self.compressibility is None else self.compressibility * EV_PER_A3_IN_GPA   # 1/GPa -> A^3/eV
        return dict(ensemble=self.ensemble, dt=self.timestep, taut=self.taut, friction=self.friction,
                    pressure=self.pressure / EV_PER_A3_IN_GPA, taup=self.taup, compressibility=beta, fix_com=self.fix_com)

    def run(self, lattices: Sequence, positions: Sequence, atomic_numbers: Sequence, steps: int, velocities: Sequence | None = None,
            masses: Sequence | None = None, loginterval: int = 10, observables=None) -> list:
        """Integrate every structure (lattices: [3,3] rows = lattice vectors, positions: [n_s,3] Cartesian, atomic_numbers: [n_s])
        for `steps` steps.  velocities: [n_s,3] A/fs per structure (default: Maxwell-Boltzmann at the temperature, zero momentum);
        masses: [n_s] amu per structure (default: standard atomic weights).  Returns one dict per structure: positions (unwrapped),
        velocities, lattice, total_energy, forces, stresses (pair virial) at the final step, n_steps, error (its forces became
        non-finite: it was stopped where it stood), and `log`: arrays step, e_pot, ke (eV), t (K), p (GPa), v (A^3) (and `conserved`,
        eV, with "nvt_nose_hoover", "npt_mtk" and "npt_mtk_cell"; the last also pressure_tensor and lattice) every `loginterval` steps and at the last one.  observables: a `TrajectoryObservables`, a `ScatteringObservables`, a `LocalOrderObservables`, a `ThermoObservables`, or a list / tuple
        holding at most one of each; the trajectory is then sampled on the
        device before the integrator call of every `sample_interval`-th step (positions, forces and velocities are synchronous only
        there: the sampler completes the half-step velocities with the finish kick itself) and every dict gains "observables"
        (trajectory), "scattering", "local_order" and / or "thermo".
        With "nvt_nose_hoover" the sampler's own v + dt/2 a is the state between the closing kick and the closing thermostat
        half-step: a point on the trajectory of the cyclically permuted splitting, as good a sample of the same dynamics (so the
        kinetic energy a `ThermoObservables` sees there is not the logged `ke`, which is taken after that half-step).  With
        "npt_mtk" and "npt_mtk_cell" the closing kick is not the plain one (it carries the barostat's friction), so those two kinds
        raise ValueError; a `LocalOrderObservables` reads positions and cells only (the current ones, before the integrator call
        of every `sample_interval`-th step) and runs with every ensemble.  A `ThermoObservables` runs with every ensemble too: with "npt_mtk" and
        "npt_mtk_cell" it reads the kinetic energy (and, "npt_mtk_cell", the pressure tensor) from the integrator's own observables
        after the integrator call, beside the cell, energies and stresses of the same step; "npt_mtk" states no pressure tensor,
        so `ThermoObservables(n_lags > 0)` raises ValueError there.  "npt_mtk_cell" with `cell_mask` "orthorhombic" needs every lattice diagonal to 1e-9 of its largest entry.
        As in the other NPT ensembles the cells go to the host and the candidates are searched again at every step."""
        thermo, observables = _take_thermo(observables)
        if thermo is not None and thermo.n_lags > 0 and self.ensemble == "npt_mtk":
            raise ValueError("ThermoObservables(n_lags > 0) is not supported with npt_mtk: its integrator states no pressure tensor")
        local, observables = _take_local_order(observables)
        observables, scattering = _split_observables(observables)
        if (observables is not None or scattering is not None) and self.ensemble in ("npt_mtk", "npt_mtk_cell"):
            raise ValueError(f"observables are not supported with {self.ensemble}: its finish kick is not the sampler's v + dt/2 a")
        steps, loginterval = integer("steps", steps, 0), integer("loginterval", loginterval, 1)
        lat, pos, z = structure_arrays(lattices, positions, atomic_numbers)
        S = len(z)
        cell = self.ensemble in MTK_CELL_ENSEMBLES
        nhc = self.ensemble in NHC_ENSEMBLES or cell   # (the deterministic ensembles: a conserved quantity, temperatures > 0)
        if cell and self.cell_mask == "orthorhombic":
            for s, L in enumerate(lat):
                if np.abs(L - np.diag(np.diag(L))).max() > 1e-9 * np.abs(L).max():
                    raise ValueError(f"structure {s}: cell_mask 'orthorhombic' needs a diagonal lattice (cell vectors along the axes)")
        if nhc and self.fix_com and min(len(a) for a in z) == 1:
            raise ValueError(f"{self.ensemble} with fix_com needs more than one atom per structure (g = 3 n - 3 degrees of freedom)")
        temps = per_structure("temperature", self.temperature, S)
        seeds = structure_seeds(self.seed, S)
        m = structure_masses(masses, z)
        if velocities is None:
            vel = [maxwell_boltzmann(ms, t, int(sd)) for ms, t, sd in zip(m, temps, seeds)]
        else:
            if len(velocities) != S:
                raise ValueError("velocities: expected one array per structure")
            vel = [np.asarray(v, dtype=np.float64) for v in velocities]
            for s, (v, a) in enumerate(zip(vel, z)):
                if v.shape != (len(a), 3) or not np.isfinite(v).all():
                    raise ValueError(f"structure {s}: velocities must be a finite [{len(a)}, 3] array")
        batch = MdBatch(self.model, lat, pos, z, [(0, S)], self.skin, self.device)
        (vg,), pos_t, lat64 = batch.graphs, batch.pos, batch.lattice   # (the NPT launches write the scaled cells into lat64)
        npt = self.ensemble in ("npt_berendsen", "npt_mtk", "npt_mtk_cell")
        vel_t = torch.tensor(np.concatenate(vel), device=vg.device)
        keys = () if nhc else (seeds,)   # (the deterministic ensembles draw nothing)
        dyn = (MtkCellState if cell else NhcState if nhc else DynState)(pos_t, lat64, batch.offsets, np.concatenate(m), vel_t, temps, *keys,
                                                                        **self._params())
        traj = observables.begin(lat, z, m, vg.device) if observables is not None else None
        sq = scattering.begin(lat, z, m, vg.device) if scattering is not None else None
        lo = local.begin(lat, z, m, vg.device) if local is not None else None
        mtk = self.ensemble in ("npt_mtk", "npt_mtk_cell")   # (the kinetic part comes from the integrator's own obs row)
        th = thermo.begin(lat, z, m, vg.device, self.pressure / EV_PER_A3_IN_GPA if npt else 0.0, self.ensemble,
                          self.cell_mask, self.fix_com) if thermo is not None else None
        th_cell = torch.empty_like(lat64) if th is not None and mtk else None
        log, cells = MdLog(conserved=nhc, cell=cell), []

        def before(k, out, logged):
            if traj is not None and k % observables.sample_interval == 0:
                traj_sample(traj, pos_t, lat64, dyn.velocities, out[K.FORCES], 0.0 if k == 0 else 0.5 * self.timestep)
            if sq is not None and k % scattering.sample_interval == 0:
                sq_sample(sq, pos_t, lat64, dyn.velocities, out[K.FORCES], 0.0 if k == 0 else 0.5 * self.timestep)
            if lo is not None and k % local.sample_interval == 0:
                lo_sample(lo, pos_t, lat64)
            if th is not None and k % thermo.sample_interval == 0:
                if mtk:
                    th_cell.copy_(lat64)   # (the cell of the sample: the integrator call moves it on)
                else:
                    thermo_sample(th, out[K.TOTAL_ENERGY], out[K.STRESSES], lat64, dyn.velocities, out[K.FORCES],
                                  0.0 if k == 0 else 0.5 * self.timestep)
            if cell and logged:
                cells.append(lat64.clone())   # (the cell of the observables: the integrator call moves it on)

        def after(k, out):
            if th is not None and mtk and k % thermo.sample_interval == 0:   # ke (and the pressure tensor) as the integrator states them
                thermo_sample(th, out[K.TOTAL_ENERGY], out[K.STRESSES], th_cell, kinetic=dyn.obs[:, 0],
                              pressure_tensor=dyn.obs[:, 6:12] if cell else None)
            if npt and k < steps:
                vg.set_lattice(list(lat64.cpu().numpy()))   # (waits: the candidate search in the new cells needs them on the host)

        out = md_loop(batch, dyn, steps, before=before, after=after, loginterval=loginterval,
                      log=lambda k, out: log.append(k, out[K.TOTAL_ENERGY], dyn.obs, cells.pop() if cell else None))
        res = md_results(batch, dyn, out, log, "molecular dynamics")
        if traj is not None:
            for r, obs in zip(res, observables.results(traj, self.timestep)):
                r["observables"] = obs
        if sq is not None:
            for r, obs in zip(res, scattering.results(sq, self.timestep)):
                r["scattering"] = obs
        if lo is not None:
            for r, obs in zip(res, local.results(lo, self.timestep)):
                r["local_order"] = obs
        if th is not None:
            for r, obs in zip(res, thermo.results(th, self.timestep)):
                r["thermo"] = obs
        return res
