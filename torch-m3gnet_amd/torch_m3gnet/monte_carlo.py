"""Batched canonical atom-swap Monte Carlo on the device (C ABI: m3g_mc_*, csrc/m3g_mc.hip), alone on a fixed lattice or interleaved
with the Langevin integrator of `dynamics` (hybrid MC/MD, the scheme of LAMMPS' fix atom/swap): which arrangement of the species on
the sites has the lowest free energy -- ordering, segregation, cation disorder, short-range order.

A trial exchanges the occupants of two sites of one structure: two entries of `atom_types` and, in a hybrid run, their masses and
velocities.  Positions never move, so the Verlet candidates, the neighbour and triplet lists and the topology of `VerletGraph` all stay
valid, and the engine reads the species through the same device pointer at every call: a trial costs one engine evaluation (without
forces in pure Monte Carlo) plus `mc_propose` (one launch) and `mc_decide` (one or two), all queued on the stream of the run -- the
host waits for nothing new.  One engine call evaluates the trial of every structure of the batch; every structure has its own random
stream, and the Monte Carlo arithmetic of a structure is bitwise the same alone or in any batch.

Units as in `dynamics`: A, fs, amu, eV, K."""
from __future__ import annotations

from typing import Sequence

import numpy as np
import torch

from . import _cuda, _lib
from ._driver import (Driver, MdBatch, boolean, check_tensor, integer, md_loop, non_negative, per_structure, positive, read_state,
                      state_tensor, structure_arrays, structure_masses, structure_seeds)
from .data import MaterialGraphKey as K
from .data.graph_gpu import _ptr, _stream
from .dynamics import KB, DynState, maxwell_boltzmann
from .nn.modules import Gradient


class McState:
    """Swap Monte Carlo state of a batch on the device (m3g_mc_init): per structure the temperature, seed, flags (M3G_MC_*), proposal
    counter, pending pair, attempts / accepts / non-finite trials and the statistics of the current energy; per row the site mask; and
    the chunk table of the batch.  `offsets`: S + 1 atom offsets; `temperatures` (K, > 0) and `seeds`: [S]; `active`: [N] (truthy = the
    row takes part)."""

    def __init__(self, offsets: Sequence[int], temperatures, seeds, active, device="cuda"):
        self.offsets = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64).reshape(-1))
        self.S = len(self.offsets) - 1
        if self.S < 1:
            raise ValueError("offsets must hold S + 1 >= 2 entries")
        self.N = int(self.offsets[-1])
        self.temperatures = np.ascontiguousarray(np.broadcast_to(np.asarray(temperatures, dtype=np.float64), (self.S,)))
        self.seeds = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64).reshape(-1))
        self.active = np.ascontiguousarray(np.asarray(active).reshape(-1) != 0).astype(np.uint8)
        if len(self.seeds) != self.S or len(self.active) != self.N:
            raise ValueError(f"expected {self.S} seeds and {self.N} site-mask entries; got {len(self.seeds)} and {len(self.active)}")
        self.device = torch.device(device)
        self.lib = _lib.load_library()
        self.state = state_tensor(self.lib.m3g_mc_state_bytes, self.N, self.S, device=self.device)
        self.device = self.state.device   # (with its index: what the tensors of a call are compared against)
        with _cuda.on_device(self.device):
            _lib.check(self.lib.m3g_mc_init(self.N, self.S, self.offsets.ctypes.data, self.temperatures.ctypes.data, self.seeds.ctypes.data,
                                            self.active.ctypes.data, _ptr(self.state), self.state.numel(), _stream()))

    def read(self) -> dict:
        """flags (int32), n_proposals, attempts, accepts, nonfinite, count (int64), mean, m2 (fp64) [S] and the last attempted pair
        [S, 2] (int32, rows relative to the structure), copied to the host (waits for the stream)."""
        S = self.S
        return read_state(self.lib.m3g_mc_read, (self.N, S), self.state,
                          (("flags", np.int32, S), ("n_proposals", np.int64, S), ("attempts", np.int64, S), ("accepts", np.int64, S),
                           ("nonfinite", np.int64, S), ("count", np.int64, S), ("mean", np.float64, S), ("m2", np.float64, S),
                           ("pair", np.int32, (S, 2))))


def _dyn_args(state: McState, dyn: DynState | None):
    if dyn is None:
        return None, 0
    if dyn.N != state.N or dyn.S != state.S:
        raise ValueError(f"the dynamics state holds {dyn.S} structures of {dyn.N} atoms, the Monte Carlo state {state.S} of {state.N}")
    return _ptr(dyn.state), dyn.state.numel()


def mc_propose(state: McState, atom_types: torch.Tensor, energies: torch.Tensor, dyn: DynState | None = None) -> None:
    """One swap proposal of every structure (m3g_mc_propose): `atom_types` [N] int64 -- the tensor the engine reads -- is exchanged in
    place, and with `dyn` the masses and velocities of the two rows travel along (`dyn` must be at a synchronous point: call
    `dyn_step(finish_only=True)` first).  `energies` [S] float32: the current ones.  One launch queued on the current stream; no wait,
    capture-safe."""
    check_tensor("atom_types", atom_types, (state.N,), torch.int64, state.device)
    check_tensor("energies", energies, (state.S,), torch.float32, state.device)
    dyn_ptr, dyn_bytes = _dyn_args(state, dyn)
    with _cuda.on_device(state.device):
        _lib.check(state.lib.m3g_mc_propose(state.N, state.S, _ptr(state.state), state.state.numel(), _ptr(atom_types), dyn_ptr, dyn_bytes,
                                            _ptr(energies), _stream()))


def mc_decide(state: McState, atom_types: torch.Tensor, trial_energies: torch.Tensor, energies: torch.Tensor,
              trial_forces: torch.Tensor | None = None, forces: torch.Tensor | None = None, trial_stresses: torch.Tensor | None = None,
              stresses: torch.Tensor | None = None, dyn: DynState | None = None, history: torch.Tensor | None = None) -> None:
    """The Metropolis verdict of every pending proposal (m3g_mc_decide) at `trial_energies` [S] float32: a rejected pair is exchanged
    back, an accepted structure's `energies` entry -- and its rows of `forces` [N,3] / `stresses` [S,6], when given with their trial
    partners -- take the trial values in place.  `history`: [rows, S, 3] int32 or None; row a receives (i, j, verdict) of call a < rows.
    Two launches (one without forces and stresses) queued on the current stream; no wait, capture-safe."""
    check_tensor("atom_types", atom_types, (state.N,), torch.int64, state.device)
    check_tensor("trial_energies", trial_energies, (state.S,), torch.float32, state.device)
    check_tensor("energies", energies, (state.S,), torch.float32, state.device)
    if (trial_forces is None) != (forces is None) or (trial_stresses is None) != (stresses is None):
        raise ValueError("trial and current forces (stresses) must be given together")
    for name, x, shape in (("trial_forces", trial_forces, (state.N, 3)), ("forces", forces, (state.N, 3)),
                           ("trial_stresses", trial_stresses, (state.S, 6)), ("stresses", stresses, (state.S, 6))):
        if x is not None:
            check_tensor(name, x, shape, torch.float32, state.device)
    if history is not None:
        check_tensor("history", history, ("rows", state.S, 3), torch.int32, state.device)
    dyn_ptr, dyn_bytes = _dyn_args(state, dyn)
    with _cuda.on_device(state.device):
        _lib.check(state.lib.m3g_mc_decide(state.N, state.S, _ptr(state.state), state.state.numel(), _ptr(atom_types), dyn_ptr, dyn_bytes,
                                           _ptr(trial_energies), _ptr(trial_forces), _ptr(trial_stresses), _ptr(energies), _ptr(forces),
                                           _ptr(stresses), _ptr(history), 0 if history is None else history.size(0), _stream()))


class SwapMonteCarlo(Driver):
    """Canonical atom-swap Monte Carlo of a batch of structures: pure lattice Monte Carlo (`md_steps` = 0: positions fixed, one
    energy-only engine evaluation per trial) or hybrid MC/MD (`md_steps` > 0: a swap trial after every `md_steps` steps of Langevin
    BAOAB dynamics at the same temperatures; masses and velocities travel with the atoms).

    `model`: the `Gradient` returned by `build_model`.  `temperature` (K, > 0) and `seed`: one value or one per structure; the seeds
    derive as in `MolecularDynamics` (`structure_seeds`), and a structure's swap stream and Langevin noise use different Philox key
    words of its own seed, so a structure draws the same alone or beside others.  `species`: the atomic numbers that take part
    (default: all); `run(sites=...)` takes an explicit mask per structure instead.  `timestep` in fs, `friction` in 1/fs.
    `structure_batches`: True evaluates every structure as an engine batch of its own -- the engine's fp32 rounding depends on the
    composition of its batch (as in `ReplicaExchange(ladder_batches=...)`), so only then is a structure's whole run bitwise the same
    alone or beside others, at one engine call per structure and trial; False, the DEFAULT here because throughput is the point,
    evaluates all structures in one engine call per trial (a structure then agrees with its run alone to the engine's rounding, which
    may flip a verdict that is nearly tied).  The proposals and verdicts run in one state of all structures either way."""

    def __init__(self, model: Gradient, temperature, species=None, md_steps: int = 0, timestep: float = 1.0, friction: float = 0.01,
                 skin: float = 0.5, seed=0, device="cuda", structure_batches: bool = False):
        super().__init__(model, skin, device)
        self.structure_batches = boolean("structure_batches", structure_batches)
        self.md_steps = integer("md_steps", md_steps, 0)
        self.timestep = positive("timestep", timestep)
        self.friction = non_negative("friction", friction)
        t = np.asarray(temperature, dtype=np.float64)
        if t.ndim > 1 or t.size == 0 or not (np.isfinite(t).all() and (t > 0).all()):
            raise ValueError("temperature must be one finite value > 0 (K) or one per structure")
        self.temperature = t
        if species is not None:
            species = np.asarray(species).reshape(-1)
            if len(species) == 0 or not np.issubdtype(species.dtype, np.integer) or (species < 1).any():
                raise ValueError("species must be a non-empty sequence of atomic numbers")
        self.species = species
        self.seed = seed

    def _mask(self, z: list, sites) -> np.ndarray:
        if sites is not None:
            if self.species is not None:
                raise ValueError("give either species (at construction) or sites (to run), not both")
            if len(sites) != len(z):
                raise ValueError("sites: expected one mask per structure")
            masks = [np.asarray(m).reshape(-1) != 0 for m in sites]
            for s, (m, a) in enumerate(zip(masks, z)):
                if len(m) != len(a):
                    raise ValueError(f"structure {s}: sites must hold {len(a)} entries")
            return np.concatenate(masks)
        if self.species is None:
            return np.ones(sum(len(a) for a in z), dtype=bool)
        return np.concatenate([np.isin(a, self.species) for a in z])

    def run(self, lattices: Sequence, positions: Sequence, atomic_numbers: Sequence, trials: int, sites: Sequence | None = None,
            masses: Sequence | None = None, loginterval: int = 10) -> list:
        """`trials` swap trials of every structure (structure arguments as `MolecularDynamics.run`; sites: one [n_s] mask per structure;
        masses: [n_s] amu per structure, default the standard atomic weights of the species -- they travel with the atoms either way;
        hybrid runs start from Maxwell-Boltzmann velocities).  Returns one dict per structure: the final atomic_numbers, positions,
        lattice and total_energy (the tracked current energy); velocities (hybrid only); attempts, acceptance, nonfinite (trials whose
        energy was not finite: rejected); mean_energy (eV) and heat_capacity (eV/K, var(E) / (kB T^2)) of the potential energy after
        every verdict; `energy`: its trace every `loginterval` trials and at the last one, with `energy_at` the trial numbers;
        trial_energy [trials]: the engine's energy of every trial configuration, accepted or not; swaps [trials, 3] (row i, row j,
        verdict; -1 for a trial not attempted); error (hybrid: its forces became non-finite)."""
        trials, loginterval = integer("trials", trials, 0), integer("loginterval", loginterval, 1)
        lat, pos, z = structure_arrays(lattices, positions, atomic_numbers)
        S = len(z)
        temps = per_structure("temperature", self.temperature, S)
        active = self._mask(z, sites)
        seeds = structure_seeds(self.seed, S)
        hybrid = self.md_steps > 0
        m = structure_masses(masses, z)
        groups = [(s, s + 1) for s in range(S)] if self.structure_batches else [(0, S)]
        ev = MdBatch(self.model, lat, pos, z, groups, self.skin, self.device, whole=False)   # (two sets of buffers of its own, below)
        dev, offsets, pos_t, lat64 = ev.device, ev.offsets, ev.pos, ev.lattice
        types = torch.tensor(np.concatenate(z) - 1, dtype=torch.int64, device=dev)   # the one array the swaps write and every engine reads
        for vg, (a, b) in zip(ev.graphs, ev.rows):
            vg.use_atom_types(types[a:b])

        def evaluate(into: dict) -> dict:
            return ev.evaluate(pos_t, into, forces=hybrid)

        cur, trial = ev.buffers(hybrid), ev.buffers(hybrid)
        mc = McState(offsets, temps, seeds, active, device=dev)
        dyn = None
        if hybrid:
            vel = [maxwell_boltzmann(ms, t, int(sd)) for ms, t, sd in zip(m, temps, seeds)]
            dyn = DynState(pos_t, lat64, offsets, np.concatenate(m), torch.tensor(np.concatenate(vel), device=dev), temps, seeds,
                           ensemble="nvt_langevin", dt=self.timestep, friction=self.friction)
        history = torch.full((max(trials, 1), S, 3), -1, dtype=torch.int32, device=dev)
        trial_log = torch.full((max(trials, 1), S), float("nan"), dtype=torch.float32, device=dev)
        trace, trace_at = [], []

        def one_trial(t: int) -> None:
            mc_propose(mc, types, cur[K.TOTAL_ENERGY], dyn)
            evaluate(trial)
            trial_log[t].copy_(trial[K.TOTAL_ENERGY])
            mc_decide(mc, types, trial[K.TOTAL_ENERGY], cur[K.TOTAL_ENERGY], trial[K.FORCES], cur[K.FORCES], trial[K.STRESSES],
                      cur[K.STRESSES], dyn, history)
            if t % loginterval == 0 or t == trials - 1:   # (host copies on log trials only)
                trace.append(cur[K.TOTAL_ENERGY].double().cpu().numpy())
                trace_at.append(t)

        if not hybrid:
            evaluate(cur)
            for t in range(trials):
                one_trial(t)
        else:   # a trial at every `md_steps`-th synchronous point, the last step's too; the restart takes the CURRENT forces
            md_loop(ev, dyn, trials * self.md_steps, into=cur, sync_at=lambda k: k > 0 and k % self.md_steps == 0,
                    at_sync=lambda k, out: one_trial(k // self.md_steps - 1))
        ev.raise_on_step_errors("swap Monte Carlo")
        st = mc.read()
        dst = dyn.read() if hybrid else None
        e = cur[K.TOTAL_ENERGY].double().cpu().numpy()
        z_end, p_host, l_host = types.cpu().numpy() + 1, pos_t.cpu().numpy(), lat64.cpu().numpy()
        hist, e_trial = history[:trials].cpu().numpy(), trial_log[:trials].double().cpu().numpy()
        trace = np.stack(trace, axis=1) if trace else np.empty((S, 0))
        res = []
        for s in range(S):
            a, b = int(offsets[s]), int(offsets[s + 1])
            n, att = int(st["count"][s]), int(st["attempts"][s])
            r = {"atomic_numbers": z_end[a:b].copy(), "positions": p_host[a:b].copy(), "lattice": l_host[s].copy(),
                 "total_energy": float(e[s]), "attempts": att, "acceptance": st["accepts"][s] / att if att else float("nan"),
                 "nonfinite": int(st["nonfinite"][s]), "mean_energy": float(st["mean"][s]) if n else float("nan"),
                 "heat_capacity": float(st["m2"][s] / n / (KB * temps[s] ** 2)) if n else float("nan"), "energy": trace[s].copy(),
                 "energy_at": np.array(trace_at, dtype=np.int64), "trial_energy": e_trial[:, s].copy(), "swaps": hist[:, s].copy(),
                 "error": bool(dst["flags"][s] & _lib.DYN_ERROR) if hybrid else False}
            if hybrid:
                r["velocities"] = dst["v"][a:b].copy()
            res.append(r)
        return res


def short_range_order(lattice, positions, atomic_numbers, r_shell: float) -> dict:
    """Warren-Cowley parameters of one structure (host, numpy): {(a, b): alpha_ab} for every ordered pair of the species present,
    alpha_ab = 1 - n_ab / (n_a Z_a c_b), with n_ab the ordered pairs (centre of species a, neighbour of species b) over all periodic
    images at a distance 0 < r < `r_shell`, n_a the atoms of species a, Z_a = sum_b n_ab / n_a their mean coordination and c_b the
    concentration of b.  0: random; < 0: a and b attract; > 0: they avoid each other (nan where species a has no neighbour)."""
    L = np.asarray(lattice, dtype=np.float64).reshape(3, 3)
    x = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
    z = np.asarray(atomic_numbers).reshape(-1)
    r_shell = positive("r_shell", r_shell)
    if len(z) != len(x) or len(z) == 0:
        raise ValueError("positions and atomic_numbers must hold one entry per atom (at least one)")
    widths = abs(np.linalg.det(L)) / np.array([np.linalg.norm(np.cross(L[(k + 1) % 3], L[(k + 2) % 3])) for k in range(3)])
    reach = [int(np.ceil(r_shell / w)) for w in widths]   # images within r_shell along every lattice direction
    shifts = np.stack(np.meshgrid(*[np.arange(-n, n + 1) for n in reach], indexing="ij"), -1).reshape(-1, 3) @ L
    kinds = np.unique(z)
    idx = np.searchsorted(kinds, z)
    counts = np.zeros((len(kinds), len(kinds)))
    for sh in shifts:
        d = np.linalg.norm(x[None, :, :] + sh[None, None, :] - x[:, None, :], axis=-1)
        near = (d < r_shell) & (d > 1e-9)
        np.add.at(counts, (idx[:, None].repeat(len(z), 1)[near], idx[None, :].repeat(len(z), 0)[near]), 1.0)
    n_a = np.bincount(idx, minlength=len(kinds)).astype(np.float64)
    conc = n_a / len(z)
    out = {}
    with np.errstate(invalid="ignore", divide="ignore"):
        for a, za in enumerate(kinds):
            for b, zb in enumerate(kinds):
                out[int(za), int(zb)] = float(1.0 - counts[a, b] / (counts[a].sum() * conc[b]))
    return out
