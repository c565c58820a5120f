"""Batched reverse non-equilibrium molecular dynamics (rNEMD) on the device (C ABI: m3g_rnemd_*, csrc/m3g_rnemd.hip), over the NVE
integrator of `dynamics`: thermal conductivity (Mueller-Plathe, J. Chem. Phys. 106, 6082 (1997)) and shear viscosity (Mueller-Plathe,
Phys. Rev. E 59, 4894 (1999)), with the unequal-mass exchange of Nieto-Draghi and Avalos (Mol. Phys. 101, 2303 (2003)); LAMMPS has the
method as fix thermal/conductivity and fix viscosity.

The flux is imposed and the gradient measured: every structure is cut into `n_slabs` slabs along lattice direction `axis`; every
`swap_interval` steps the hottest atoms of slab 0 and the coldest of slab n_slabs / 2 exchange their velocities ("heat"), or the atoms
moving fastest along +flow_axis in slab 0 and slowest in slab n_slabs / 2 exchange that component ("momentum").  The exchange conserves
the energy and the momentum of the structure, so the run is plain NVE; slab 0 becomes the cold (sink) slab, the middle slab the hot
(source) one, and the known amount transferred, through both halves of the periodic cell, over the measured slope of the temperature
(velocity) profile between them is the conductivity (viscosity).  No heat flux per atom is needed, which a message-passing,
three-body potential does not define without ambiguity.  Positions never move in an exchange, so the Verlet lists stay valid, and an
exchange is two kernel launches on the stream of the run (`rnemd_exchange`): the host waits for nothing new.

Units as in `dynamics`: A, fs, amu, eV, K."""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np
import torch

from . import _cuda, _lib
from ._driver import (Driver, MdBatch, MdLog, check_tensor, integer, md_loop, md_results, non_negative, positive, read_state, state_tensor,
                      structure_arrays, structure_masses, structure_seeds)
from .data.graph_gpu import _ptr, _stream
from .dynamics import KAPPA, KB, DynState, langevin_warm_up
from .nn.modules import Gradient

KINDS = {"heat": _lib.RNEMD_HEAT, "momentum": _lib.RNEMD_MOMENTUM}
EV_PER_FS_A_K_IN_W_PER_M_K = 1.602176634e6     # eV / (fs A K) in W / (m K)
AMU_PER_A_FS_IN_PA_S = 1.66053906660e-2        # amu / (A fs) in Pa s


def _choice(name: str, x, least: int, most: int) -> int:
    if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or not least <= x <= most:
        raise ValueError(f"{name} must be an integer in {least} .. {most}; got {x!r}")
    return int(x)


def rnemd_params(kind: str, axis: int, n_slabs: int, n_swaps: int, flow_axis: int | None = None) -> _lib.M3GRnemdParams:
    """The checked m3g_rnemd_params: `kind` "heat" or "momentum"; `axis` the lattice direction the slabs are stacked along; `n_slabs`
    even, 2 .. 64; `n_swaps` pairs per exchange, 1 .. 8; `flow_axis` the Cartesian component exchanged by "momentum" (default
    (axis + 1) % 3; not `axis`), unused by "heat"."""
    if not isinstance(kind, str) or kind not in KINDS:
        raise ValueError(f"unknown kind {kind!r}; expected one of {sorted(KINDS)}")
    axis = _choice("axis", axis, 0, 2)
    flow_axis = _choice("flow_axis", (axis + 1) % 3 if flow_axis is None else flow_axis, 0, 2)
    if kind == "momentum" and flow_axis == axis:
        raise ValueError("momentum: flow_axis must differ from axis (the momentum exchanged is perpendicular to the slab normal)")
    n_slabs = _choice("n_slabs", n_slabs, 2, _lib.RNEMD_MAX_SLABS)
    if n_slabs % 2:
        raise ValueError(f"n_slabs must be even; got {n_slabs}")
    return _lib.M3GRnemdParams(kind=KINDS[kind], axis=axis, flow_axis=flow_axis, n_slabs=n_slabs,
                               n_swaps=_choice("n_swaps", n_swaps, 1, _lib.RNEMD_MAX_SWAPS), reserved=0)


class RnemdState:
    """rNEMD state of a batch on the device (m3g_rnemd_init): the slab normal of every structure, the `active` mask ([N] booleans,
    default all: inactive rows are never exchanged but are sampled), the counters and the slab accumulators.  `offsets`: S + 1 atom
    offsets; `lattices`: [S,3,3], rows = lattice vectors (fixed for the run: NVE); the rest as `rnemd_params`."""

    def __init__(self, offsets: Sequence[int], lattices, kind: str, axis: int, n_slabs: int, n_swaps: int, flow_axis: int | None = None,
                 active=None, device="cuda"):
        self.kind = kind
        self.params = rnemd_params(kind, axis, n_slabs, n_swaps, flow_axis)
        self.offsets = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64).reshape(-1))
        self.S = len(self.offsets) - 1
        if self.S < 1:
            raise ValueError("offsets must hold S + 1 >= 2 entries")
        self.N = int(self.offsets[-1])
        self.lattices = np.ascontiguousarray(np.asarray(lattices, dtype=np.float64))
        if self.lattices.shape != (self.S, 3, 3):
            raise ValueError(f"lattices must be [{self.S}, 3, 3]; got {self.lattices.shape}")
        self.active = None if active is None else np.ascontiguousarray(np.asarray(active).reshape(-1) != 0).astype(np.uint8)
        if self.active is not None and len(self.active) != self.N:
            raise ValueError(f"active: expected {self.N} entries; got {len(self.active)}")
        self.device = torch.device(device)
        self.lib = _lib.load_library()
        self.state = state_tensor(self.lib.m3g_rnemd_state_bytes, self.N, self.S, self.params.n_slabs, device=self.device)
        with _cuda.on_device(self.device):
            _lib.check(self.lib.m3g_rnemd_init(C.byref(self.params), self.N, self.S, self.offsets.ctypes.data, self.lattices.ctypes.data,
                                               None if self.active is None else self.active.ctypes.data, _ptr(self.state),
                                               self.state.numel(), _stream()))

    def read(self) -> dict:
        """n_calls, n_exchanged (int64 [S]), transferred (fp64 [S]: eV for "heat", amu A/fs for "momentum"), n_samples (int64 [S]),
        last_pairs (int32 [S, n_swaps, 2]: the rows, relative to the structure, the last swapping call exchanged, slab-0 row first,
        -1 where none), count (int64 [S, n_slabs]) and sums (fp64 [S, n_slabs, 5]: sum m, m vx, m vy, m vz, m |v|^2), copied to the
        host (waits for the stream)."""
        S, nb, ns = self.S, self.params.n_slabs, self.params.n_swaps
        return read_state(self.lib.m3g_rnemd_read, (C.byref(self.params), self.N, S), self.state,
                          (("n_calls", np.int64, S), ("n_exchanged", np.int64, S), ("transferred", np.float64, S),
                           ("n_samples", np.int64, S), ("last_pairs", np.int32, (S, ns, 2)), ("count", np.int64, (S, nb)),
                           ("sums", np.float64, (S, nb, 5))))


def rnemd_exchange(state: RnemdState, dyn: DynState, pos: torch.Tensor, swap: bool = True, sample: bool = True) -> None:
    """One call of every structure (m3g_rnemd_exchange) on the velocities of `dyn` -- which must be at a synchronous point: call
    `dyn_step(finish_only=True)` first -- at the positions `pos` [N,3] fp64 (unwrapped).  `sample`: the slab counts and sums of the
    velocities BEFORE the exchange join the accumulators; `swap`: the exchange itself.  A structure flagged STARTED or ERROR is left
    untouched and not sampled.  Two launches queued on the current stream; no wait, capture-safe."""
    if dyn.S != state.S or dyn.N != state.N:
        raise ValueError(f"the dynamics state holds {dyn.S} structures of {dyn.N} atoms, the rNEMD state {state.S} of {state.N}")
    check_tensor("pos", pos, (state.N, 3), torch.float64, dyn.device)
    with _cuda.on_device(dyn.device):
        _lib.check(state.lib.m3g_rnemd_exchange(C.byref(state.params), dyn.N, dyn.S, _ptr(state.state), state.state.numel(), _ptr(dyn.state),
                                                dyn.state.numel(), _ptr(pos), 1 if swap else 0, 1 if sample else 0, _stream()))


def slab_geometry(lattice, axis: int, n_slabs: int):
    """(slab centres [n_slabs] in A along the slab normal, cross-section A in A^2) of a cell cut along lattice direction `axis`: the
    slabs are (b + 1/2) h / n_slabs, h = V / A the height of the cell, A = |a_j x a_k| the face the other two vectors span."""
    L = np.asarray(lattice, dtype=np.float64)
    j, k = [q for q in range(3) if q != axis]
    area = float(np.linalg.norm(np.cross(L[j], L[k])))
    height = abs(float(np.linalg.det(L))) / area
    return (np.arange(n_slabs) + 0.5) * height / n_slabs, area


def transport_coefficients(kind: str, lattice, axis: int, flow_axis: int, count, sums, transferred: float, time: float) -> dict:
    """The host post-processing of one structure: `count` [n_slabs] and `sums` [n_slabs, 5] as `RnemdState.read`, `transferred` (eV or
    amu A/fs) during `time` (fs).  Returns slab_centres (A), temperature_profile (K: sum m|v|^2 / (3 kB kappa count)),
    velocity_profile ([n_slabs, 3], A/fs: sum m v / sum m), counts, flux (transferred / (2 A time): both halves of the periodic cell
    carry it), gradient_sides ([2]: the least-squares slope of the temperature ("heat") or flow_axis velocity ("momentum") profile over
    the slabs strictly between 0 and n_slabs / 2, and over those beyond n_slabs / 2), gradient (the mean of their magnitudes) and
    thermal_conductivity (W / (m K)) or viscosity (Pa s) = flux / gradient.  Empty slabs give NaN."""
    count, sums = np.asarray(count, dtype=np.int64), np.asarray(sums, dtype=np.float64)
    n = len(count)
    centres, area = slab_geometry(lattice, axis, n)
    with np.errstate(invalid="ignore", divide="ignore"):
        t_prof = sums[:, 4] / (3.0 * KB * KAPPA * count)
        v_prof = sums[:, 1:4] / sums[:, :1]
        prof = t_prof if kind == "heat" else v_prof[:, flow_axis]
        sides = np.array([np.polyfit(centres[lo:hi], prof[lo:hi], 1)[0] if hi - lo >= 2 and np.isfinite(prof[lo:hi]).all() else np.nan
                          for lo, hi in ((1, n // 2), (n // 2 + 1, n))])
        flux = transferred / (2.0 * area * time) if time > 0 else float("nan")
        gradient = float(np.abs(sides).mean())
        coefficient = flux / gradient
    name, unit = ("thermal_conductivity", EV_PER_FS_A_K_IN_W_PER_M_K) if kind == "heat" else ("viscosity", AMU_PER_A_FS_IN_PA_S)
    return {"slab_centres": centres, "temperature_profile": t_prof, "velocity_profile": v_prof, "counts": count.copy(), "flux": float(flux),
            "gradient_sides": sides, "gradient": gradient, name: float(coefficient * unit)}


class ReverseNEMD(Driver):
    """Thermal conductivity (`kind` "heat") or shear viscosity ("momentum") of a batch of structures by reverse non-equilibrium MD.

    `model`: the `Gradient` returned by `build_model`.  Every structure is first equilibrated with the Langevin thermostat (BAOAB,
    `friction` in 1/fs) at `temperature` (K, one value), then run in NVE with an exchange of `n_swaps` pairs every `swap_interval`
    steps between slab 0 and slab n_slabs / 2 of `n_slabs` (even, 6 .. 64) slabs along lattice direction `axis`; the slab sums are
    sampled every `sample_interval` steps.  `flow_axis`: the Cartesian velocity component "momentum" exchanges (default
    (axis + 1) % 3).  `timestep` in fs; `seed`: an integer, or one per structure.

    All structures of a run share one engine batch, and the engine's fp32 rounding depends on the composition of its batch (as
    `ReplicaExchange` states): only the m3g_rnemd_* kernels are bitwise the same for a structure alone or in any batch, not the whole
    run, which agrees with the run alone to the engine's rounding, amplified by the dynamics.

    The conductivity of a cell of finite length along `axis` depends on that length (phonons with a mean free path beyond it are
    cut off): run several lengths and extrapolate 1 / kappa against 1 / L -- that is the caller's job, as is checking that the
    profile is linear between the exchange slabs (a `swap_interval` too short drives the response out of the linear regime)."""

    def __init__(self, model: Gradient, kind: str = "heat", temperature: float = 300.0, timestep: float = 1.0, axis: int = 2,
                 n_slabs: int = 20, n_swaps: int = 1, swap_interval: int = 100, sample_interval: int = 10, flow_axis: int | None = None,
                 friction: float = 0.01, skin: float = 0.5, seed=0, device="cuda"):
        super().__init__(model, skin, device)
        self.kind = kind
        self.params = rnemd_params(kind, axis, n_slabs, n_swaps, flow_axis)
        if self.params.n_slabs < 6:
            raise ValueError(f"n_slabs must be at least 6 (two slabs between the exchange slabs on either side); got {n_slabs}")
        self.temperature = positive("temperature", temperature)
        self.timestep = positive("timestep", timestep)
        self.friction = non_negative("friction", friction)
        self.swap_interval = integer("swap_interval", swap_interval, 1)
        self.sample_interval = integer("sample_interval", sample_interval, 1)
        self.seed = seed

    def run(self, lattices: Sequence, positions: Sequence, atomic_numbers: Sequence, steps: int, equilibration: int = 0, discard: int = 0,
            masses: Sequence | None = None, loginterval: int = 10, blocks: int = 1) -> list:
        """`equilibration` Langevin steps from Maxwell-Boltzmann velocities, then `steps` NVE steps from the full-step velocities the
        thermostatted run ended with (copied on the device).  At every NVE step 0 < k < steps that is a multiple of `swap_interval`
        or of `sample_interval` the integrator is brought to a synchronous point and `rnemd_exchange` called; samples and the
        transferred amount count from step `discard` on (the profile needs time to become stationary).  Arguments otherwise as
        `MolecularDynamics.run`.  Returns one dict per structure: that of `MolecularDynamics.run` for the NVE phase (its log holds
        the NVE steps), the entries of `transport_coefficients` over the steps from `discard` on, `transferred` (since `discard`;
        eV or amu A/fs), `n_exchanged` (pairs exchanged in the whole NVE phase), `n_calls` (exchange calls), and of every exchange
        call `kinetic_energy_at_exchange` [n_calls, 2] (eV, before and after) and `momentum_at_exchange` [n_calls, 2, 3] (amu A/fs).
        `blocks`: the steps from `discard` on are cut into that many equal parts and the accumulators read at the end of each (one
        wait per block), returned as `block_counts` [blocks, n_slabs] and `block_sums` [blocks, n_slabs, 5]: block averages of the
        profile, for error bars."""
        steps, loginterval, blocks = integer("steps", steps, 0), integer("loginterval", loginterval, 1), integer("blocks", blocks, 1)
        equilibration, discard = integer("equilibration", equilibration, 0), integer("discard", discard, 0)
        if discard > steps:
            raise ValueError(f"discard ({discard}) must not exceed steps ({steps})")
        lat, pos, z = structure_arrays(lattices, positions, atomic_numbers)
        S = len(z)
        seeds = structure_seeds(self.seed, S)
        m = structure_masses(masses, z)
        batch = MdBatch(self.model, lat, pos, z, [(0, S)], self.skin, self.device)
        dev, pos_t, offsets, spans = batch.device, batch.pos, batch.offsets, batch.atoms
        common = dict(dt=self.timestep, friction=self.friction)
        warm = langevin_warm_up(batch, m, self.temperature, seeds, equilibration, **common)
        m_all = np.concatenate(m)
        dyn = DynState(pos_t, batch.lattice, offsets, m_all, warm.velocities, self.temperature, seeds, ensemble="nve", **common)
        rn = RnemdState(offsets, np.stack(lat), self.kind, self.params.axis, self.params.n_slabs, self.params.n_swaps,
                        flow_axis=self.params.flow_axis, device=dev)
        mass_t = torch.tensor(m_all, device=dev)[:, None]
        momentum = lambda: torch.stack([(mass_t[a:b] * dyn.velocities[a:b]).sum(0) for a, b in spans])
        ke, mom = [], []
        base = np.zeros(S)
        ends = {discard + (steps - discard) * (j + 1) // blocks for j in range(blocks - 1)} - {discard}   # where a block ends, but the last
        marks = [(np.zeros((S, self.params.n_slabs), dtype=np.int64), np.zeros((S, self.params.n_slabs, 5)))]
        swap = lambda k: 0 < k < steps and k % self.swap_interval == 0
        sample = lambda k: 0 < k < steps and k % self.sample_interval == 0 and k >= discard

        def reads(k, out, logged):
            nonlocal base
            if k == discard and k > 0:
                base = rn.read()["transferred"]   # (waits, once: what was transferred before `discard` does not count)
            if k in ends:   # (waits: the samples of step k itself belong to the next block)
                now = rn.read()
                marks.append((now["count"], now["sums"]))

        def exchange(k, out):
            ke.append([dyn.obs[:, 0].clone()])
            mom.append([momentum()])
            rnemd_exchange(rn, dyn, pos_t, swap=swap(k), sample=sample(k))
            mom[-1].append(momentum())   # (before the next step's kick changes it)
            return lambda: ke[-1].append(dyn.obs[:, 0].clone())

        log = MdLog()
        out = md_loop(batch, dyn, steps, before=reads, sync_at=lambda k: swap(k) or sample(k), at_sync=exchange, log=log.of(dyn),
                      loginterval=loginterval)
        runs = md_results(batch, dyn, out, log, "reverse non-equilibrium molecular dynamics")
        ex = rn.read()
        ke_host = torch.stack([torch.stack(pair) for pair in ke]).cpu().numpy() if ke else np.zeros((0, 2, S))
        mom_host = torch.stack([torch.stack(pair) for pair in mom]).cpu().numpy() if mom else np.zeros((0, 2, S, 3))
        marks.append((ex["count"], ex["sums"]))
        time = (steps - discard) * self.timestep
        res = []
        for s, r in enumerate(runs):
            moved = float(ex["transferred"][s] - base[s])
            r.update(transport_coefficients(self.kind, lat[s], self.params.axis, self.params.flow_axis, ex["count"][s], ex["sums"][s], moved,
                                            time))
            r.update(transferred=moved, n_exchanged=int(ex["n_exchanged"][s]), n_calls=int(ex["n_calls"][s]),
                     n_samples=int(ex["n_samples"][s]), kinetic_energy_at_exchange=ke_host[:, :, s].copy(),
                     momentum_at_exchange=mom_host[:, :, s].copy(),
                     block_counts=np.stack([b[0][s] - a[0][s] for a, b in zip(marks, marks[1:])]),
                     block_sums=np.stack([b[1][s] - a[1][s] for a, b in zip(marks, marks[1:])]))
            res.append(r)
        return res
