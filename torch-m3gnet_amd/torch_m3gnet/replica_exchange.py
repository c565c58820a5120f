"""Batched replica-exchange molecular dynamics (parallel tempering; Sugita and Okamoto, Chem. Phys. Lett. 314, 141 (1999)) on the
device (C ABI: m3g_remd_*, csrc/m3g_remd.hip), over the Langevin integrator of `dynamics`.

Every input structure becomes a LADDER: R copies in one engine batch, copy k starting at temperature T_k of an ascending sequence.
Every `exchange_interval` steps the neighbouring pairs (k, k+1) of alternating parity attempt to swap their TEMPERATURES with the
Metropolis probability min(1, exp((1/kB T_k - 1/kB T_{k+1}) (E_i - E_j))); an accepted pair gets the other's thermostat target and its
velocities scaled by sqrt(T_new / T_old).  Positions never move between the rows of the batch, so the Verlet lists stay valid, and
the exchange is two kernel launches on the stream of the run (`remd_exchange`): the host waits for nothing new.  All ladders of a run
exchange in the same two launches, each with its own random stream; a ladder's numbers are bitwise the same alone or in any batch.

Units as in `dynamics`: A, fs, amu, eV, K."""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np
import torch

from . import _cuda, _lib
from ._driver import (Driver, MdBatch, MdLog, boolean, check_tensor, derived_keys, integer, md_loop, md_results, non_negative, positive,
                      read_state, state_tensor, structure_arrays, structure_masses)
from .data import MaterialGraphKey as K
from .data.graph_gpu import _ptr, _stream
from .dynamics import KB, DynState, maxwell_boltzmann
from .nn.modules import Gradient


def ladder_temperatures(temperatures) -> np.ndarray:
    """One ladder's temperatures as a checked fp64 array: at least two, finite, > 0, strictly ascending."""
    t = np.asarray(temperatures, dtype=np.float64)
    if t.ndim != 1 or len(t) < 2:
        raise ValueError("a temperature ladder needs at least 2 temperatures")
    if not (np.isfinite(t).all() and (t > 0).all()):
        raise ValueError("ladder temperatures must be finite and > 0 (K)")
    if not (np.diff(t) > 0).all():
        raise ValueError("ladder temperatures must be strictly ascending")
    return t


class RemdState:
    """Replica-exchange state of a batch on the device (m3g_remd_init): per replica the temperature index it holds, its velocity scale
    and round trips; per ladder and index the holder and the energy statistics; per pair attempts and accepts; per ladder the attempt
    counter.  `ladder_offsets`: G + 1 replica offsets (every ladder at least 2 replicas); `temperatures`: [S], replica order; `seeds`:
    [G]."""

    def __init__(self, ladder_offsets: Sequence[int], temperatures, seeds, device="cuda"):
        self.offsets = np.ascontiguousarray(np.asarray(ladder_offsets, dtype=np.int64).reshape(-1))
        self.temperatures = np.ascontiguousarray(np.asarray(temperatures, dtype=np.float64).reshape(-1))
        self.seeds = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64).reshape(-1))
        self.G, self.S = len(self.offsets) - 1, len(self.temperatures)
        if self.G < 1 or len(self.seeds) != self.G:
            raise ValueError(f"expected G + 1 >= 2 ladder offsets and one seed per ladder; got {len(self.offsets)} and {len(self.seeds)}")
        self.device = torch.device(device)
        self.lib = _lib.load_library()
        self.state = state_tensor(self.lib.m3g_remd_state_bytes, self.S, self.G, device=self.device)
        with _cuda.on_device(self.device):
            _lib.check(self.lib.m3g_remd_init(self.S, self.G, self.offsets.ctypes.data, self.temperatures.ctypes.data, self.seeds.ctypes.data,
                                              _ptr(self.state), self.state.numel(), _stream()))

    def read(self) -> dict:
        """held / holder (int32 [S]), attempts / accepts (int64 [S], row o_g + k = pair (k, k+1)), count / mean / m2 of the energy at
        every index [S], round_trips [S] and the ladders' attempt counters [G], copied to the host (waits for the stream)."""
        S = self.S
        return read_state(self.lib.m3g_remd_read, (S, self.G), self.state,
                          (("held", np.int32, S), ("holder", np.int32, S), ("attempts", np.int64, S), ("accepts", np.int64, S),
                           ("count", np.int64, S), ("mean", np.float64, S), ("m2", np.float64, S), ("round_trips", np.int64, S),
                           ("n_attempts", np.int64, self.G)))


def remd_exchange(state: RemdState, dyn: DynState, energies: torch.Tensor, history: torch.Tensor | None = None) -> None:
    """One exchange attempt of every ladder (m3g_remd_exchange) at `energies` [S] float32, on the replicas of `dyn` -- which must be at
    a synchronous point: call `dyn_step(finish_only=True)` first.  `history`: [rows, S] int32 or None; row a receives the held
    indices after attempt a < rows.  Two launches queued on the current stream; no wait, capture-safe."""
    if dyn.S != state.S:
        raise ValueError(f"the dynamics state holds {dyn.S} structures, the replica-exchange state {state.S}")
    check_tensor("energies", energies, (state.S,), torch.float32, dyn.device)
    if history is not None:
        check_tensor("history", history, ("rows", state.S), torch.int32, dyn.device)
    with _cuda.on_device(dyn.device):
        _lib.check(state.lib.m3g_remd_exchange(dyn.N, dyn.S, state.G, _ptr(state.state), state.state.numel(), _ptr(dyn.state),
                                               dyn.state.numel(), _ptr(energies), _ptr(history), 0 if history is None else history.size(0),
                                               _stream()))


def target_temperatures(dyn: DynState) -> torch.Tensor:
    """Live [S] fp64 view of the thermostat targets inside the state buffer of `dyn` (the array an exchange writes)."""
    at = C.c_size_t()
    _lib.check(dyn.lib.m3g_remd_target_view(dyn.N, dyn.S, C.byref(at)))
    return dyn.state[at.value:at.value + 8 * dyn.S].view(torch.float64)


class ReplicaExchange(Driver):
    """Replica-exchange MD of a batch of structures, Langevin thermostat (BAOAB) only: Berendsen is not canonical and an exchange at
    constant pressure needs a PV term in the acceptance.

    `model`: the `Gradient` returned by `build_model`.  `temperatures`: one strictly ascending sequence (K) shared by all ladders, or
    one such sequence per input structure.  `friction` in 1/fs, `timestep` in fs; an exchange is attempted every `exchange_interval`
    steps.  `ladder_batches`: True evaluates every ladder as an engine batch of its own -- the engine's fp32 rounding depends on the
    composition of its batch (as in `Phonons` / `Elasticity`), so only then are a ladder's numbers bitwise the same alone or beside
    other ladders, at one engine call per ladder and step; False evaluates all replicas in one engine batch (one call per step; a
    ladder then agrees with its run alone to the engine's rounding, which the dynamics amplify).  The integrator and the exchange
    run on one state of all replicas either way.  `seed`: an integer, or one per input structure (as in `MolecularDynamics`): the Langevin keys of a ladder's copies and the
    key of its exchange stream derive from the ladder's own seed, so a ladder runs the same alone or beside others."""

    def __init__(self, model: Gradient, temperatures, timestep: float = 1.0, friction: float = 0.01, exchange_interval: int = 100,
                 skin: float = 0.5, seed=0, device="cuda", ladder_batches: bool = True):
        super().__init__(model, skin, device)
        self.ladder_batches = boolean("ladder_batches", ladder_batches)
        self.timestep = positive("timestep", timestep)
        self.friction = non_negative("friction", friction)
        self.exchange_interval = integer("exchange_interval", exchange_interval, 1)
        self.seed = seed
        several = isinstance(temperatures, (list, tuple, np.ndarray)) and len(temperatures) > 0 and np.ndim(temperatures[0]) == 1
        if several:   # one ladder per input structure
            self.temperatures, self.shared = [ladder_temperatures(t) for t in temperatures], False
        else:
            self.temperatures, self.shared = [ladder_temperatures(temperatures)], True

    def run(self, lattices: Sequence, positions: Sequence, atomic_numbers: Sequence, steps: int, masses: Sequence | None = None,
            loginterval: int = 10) -> list:
        """Run every structure's ladder for `steps` steps (arguments as `MolecularDynamics.run`; starting velocities are
        Maxwell-Boltzmann at each copy's own temperature).  Returns one dict per input structure: temperatures [R]; attempts and
        acceptance [R-1] (pair k, k+1); mean_energy [R] (eV) and heat_capacity [R] (eV/K, var(E) / (kB T^2)) of the potential energy
        sampled at the exchange attempts; round_trips [R] (per copy); temperature_index [n_attempts + 1, R] (the index every copy
        holds: the start, then one row per attempt); kinetic_temperature [n_attempts, 2, R] (every copy's instantaneous T before and
        after each attempt: an accepted copy's changes by T_new / T_old); error; and `replicas`: R dicts as `MolecularDynamics.run`
        returns per structure, in the order of the temperature held at the end (each with the `temperature` it holds, the
        `target_temperature` of its thermostat on the device and the number `replica` of the copy)."""
        steps, loginterval = integer("steps", steps, 0), integer("loginterval", loginterval, 1)
        lat, pos, z = structure_arrays(lattices, positions, atomic_numbers)
        G = len(z)
        if not self.shared and len(self.temperatures) != G:
            raise ValueError(f"temperatures: expected one ladder or one per structure ({G}); got {len(self.temperatures)}")
        ladders = self.temperatures * G if self.shared else self.temperatures
        m = structure_masses(masses, z)
        owner = np.concatenate([np.full(len(t), g) for g, t in enumerate(ladders)])   # the input structure of every replica
        l_off = np.concatenate([[0], np.cumsum([len(t) for t in ladders])])
        temps = np.concatenate(ladders)
        S = len(owner)
        # a ladder's keys derive from its own seed only: R Langevin keys of its replicas, then the key of its exchange stream
        keys = derived_keys(self.seed, G, [len(t) + 1 for t in ladders])
        seeds, ladder_seeds = np.concatenate([k[:-1] for k in keys]), np.array([k[-1] for k in keys], dtype=np.uint64)
        lat_r, pos_r, z_r, m_r = ([x[g] for g in owner] for x in (lat, pos, z, m))
        vel = [maxwell_boltzmann(ms, t, int(sd)) for ms, t, sd in zip(m_r, temps, seeds)]
        # the ladders of every engine batch (see `ladder_batches`), as spans of replicas
        groups = [(g, g + 1) for g in range(G)] if self.ladder_batches else [(0, G)]
        ev = MdBatch(self.model, lat_r, pos_r, z_r, [(int(l_off[first]), int(l_off[last])) for first, last in groups], self.skin, self.device)
        dev = ev.device
        dyn = DynState(ev.pos, ev.lattice, ev.offsets, np.concatenate(m_r), torch.tensor(np.concatenate(vel), device=dev), temps, seeds,
                       ensemble="nvt_langevin", dt=self.timestep, friction=self.friction)
        remd = RemdState(l_off, temps, ladder_seeds, device=dev)
        n_attempts = (steps - 1) // self.exchange_interval if steps > 0 else 0
        history = torch.full((max(n_attempts, 1), S), -1, dtype=torch.int32, device=dev)
        t_kin = torch.full((max(n_attempts, 1), 2, S), float("nan"), dtype=torch.float64, device=dev)   # T before / after every attempt

        def exchange(k, out):
            a = k // self.exchange_interval - 1
            t_kin[a, 0].copy_(dyn.obs[:, 1])
            remd_exchange(remd, dyn, out[K.TOTAL_ENERGY], history)
            return lambda: t_kin[a, 1].copy_(dyn.obs[:, 1])

        log = MdLog()
        out = md_loop(ev, dyn, steps, sync_at=lambda k: 0 < k < steps and k % self.exchange_interval == 0, at_sync=exchange, log=log.of(dyn),
                      loginterval=loginterval)
        runs = md_results(ev, dyn, out, log, "replica-exchange molecular dynamics")
        ex, hist = remd.read(), history[:n_attempts].cpu().numpy()
        t_host, target = t_kin[:n_attempts].cpu().numpy(), target_temperatures(dyn).cpu().numpy()
        res = []
        for g, t in enumerate(ladders):
            lo, hi = int(l_off[g]), int(l_off[g + 1])
            R = hi - lo
            replicas = []
            for idx in range(R):   # in the order of the temperature held at the end
                s = int(ex["holder"][lo + idx])
                replicas.append(dict(runs[s], temperature=float(t[idx]), target_temperature=float(target[s]), replica=s - lo))
            count = ex["count"][lo:hi]
            attempts = ex["attempts"][lo:hi - 1]
            with np.errstate(invalid="ignore", divide="ignore"):
                var = ex["m2"][lo:hi] / count
                acceptance = ex["accepts"][lo:hi - 1] / attempts
            res.append({"temperatures": t.copy(), "attempts": attempts.copy(), "acceptance": acceptance,
                        "mean_energy": np.where(count > 0, ex["mean"][lo:hi], np.nan), "heat_capacity": var / (KB * t * t),
                        "round_trips": ex["round_trips"][lo:hi].copy(),
                        "temperature_index": np.concatenate([np.arange(R, dtype=np.int32)[None], hist[:, lo:hi]]),
                        "kinetic_temperature": t_host[:, :, lo:hi].copy(),
                        "error": any(r["error"] for r in replicas), "replicas": replicas})
        return res
