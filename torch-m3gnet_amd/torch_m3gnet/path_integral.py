"""Batched path-integral molecular dynamics on the device (C ABI: m3g_pimd_*, csrc/m3g_pimd.hip): nuclear quantum effects -- zero-point
motion, isotope effects, anything well below the Debye temperature -- by ring polymers under the PILE-L thermostat (Ceriotti,
Parrinello, Markland, Manolopoulos, J. Chem. Phys. 133, 124104 (2010)), integrated BAOAB (Liu, Li, Liu, J. Chem. Phys. 145, 024103
(2016)).

Every input structure becomes a RING of P = `n_beads` copies ("beads") in one engine batch; bead j of ring g is structure g P + j.
The ring at target temperature T samples H_P = sum_j [KE_j + 1/2 sum_i m_i w_P^2 |q_i,j - q_i,j+1|^2 + V(q_j)] with w_P = P kB T / hbar
at temperature P T, so every bead feels the engine's full force.  Per step the forces of all beads come from `VerletGraph.step` and
the integrator of the whole batch -- kick, transform to the ring's normal modes, exact free-ring evolution, Langevin thermostat,
transform back -- is three kernel launches (`pimd_step`).  P = 1 with thermostat "none" is classical NVE.

Not here: constant-pressure path integrals, ring-polymer contraction, PIGLET / GLE thermostats, the Suzuki-Chin factorisation,
exchange statistics, and `TrajectoryObservables` on beads.

Units as in `dynamics`: A, fs, amu, eV, K; velocities in A/fs."""
from __future__ import annotations

from typing import Sequence

import numpy as np
import torch

from . import _lib
from ._driver import (Driver, IntegratorState, MdBatch, boolean, derived_keys, integer, md_loop, non_negative, per_structure, positive,
                      replicated, state_tensor, structure_arrays, structure_masses)
from .data import MaterialGraphKey as K
from .dynamics import maxwell_boltzmann
from .nn.modules import Gradient

HBAR = 0.6582119569   # eV fs
THERMOSTATS = {"none": _lib.PIMD_NONE, "pile_l": _lib.PIMD_PILE_L}


def bead_count(x) -> int:
    """`n_beads`: an integer in 1 .. 64."""
    if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or not 1 <= x <= _lib.PIMD_MAX_BEADS:
        raise ValueError(f"n_beads must be an integer in 1 .. {_lib.PIMD_MAX_BEADS}; got {x!r}")
    return int(x)


def thermostat_name(x) -> str:
    """`thermostat`: "none" or "pile_l"."""
    if not isinstance(x, str) or x not in THERMOSTATS:
        raise ValueError(f"unknown thermostat {x!r}; expected one of {sorted(THERMOSTATS)}")
    return x


class PimdState(IntegratorState):
    """State of a batch of ring polymers on the device (m3g_pimd_init), shaped like `NhcState`: `pos` [N,3] fp64 (unwrapped) is the
    caller's tensor, moved IN PLACE by `pimd_step`; the `velocities` argument [N,3] fp64 is copied, the `velocities` attribute is the
    live view of the integrator's own.  `offsets`: S + 1 atom offsets of the S = R P structures, ring by ring (bead j of ring g is
    structure g P + j; all beads of a ring hold the same atoms, so the same `masses`).  `temperatures` and `seeds`: one per RING (or
    one temperature for all).  dt in fs, `centroid_friction` in 1/fs.  `obs` [R,8] (KE of all beads eV, T = 2 KE / (3 n P^2 kB) K,
    E_spring, K_prim, K_cv, heat, 0, 0) is written by every `pimd_step`."""
    FAMILY, OBS = "pimd", _lib.PIMD_OBS

    def __init__(self, pos: torch.Tensor, offsets: Sequence[int], masses, velocities: torch.Tensor, temperatures, seeds, n_beads: int,
                 thermostat: str = "pile_l", dt: float = 0.5, centroid_friction: float = 0.01, pile_lambda: float = 0.5):
        self.n_beads, self.thermostat = bead_count(n_beads), thermostat_name(thermostat)
        self.params = _lib.M3GPimdParams(thermostat=THERMOSTATS[self.thermostat], n_beads=self.n_beads, dt=dt,
                                         centroid_friction=centroid_friction, pile_lambda=pile_lambda)
        self._layout(pos, None, offsets)
        if self.S % self.n_beads:
            raise ValueError(f"the batch holds {self.S} structures, which is not a multiple of n_beads = {self.n_beads}")
        self.R = self.S // self.n_beads
        self._rows("velocities", velocities)
        if not self._host_arrays(masses, temperatures, seeds, units=self.R):
            raise ValueError(f"expected {self.N} masses and {self.R} seeds (one per ring)")
        self._allocate(state_tensor, self.N, self.S, self.n_beads, units=self.R)
        self._init(self.temperatures, self.seeds, velocities)

    def _fields(self):
        """`read()`: flags / n_steps / heat [R] and the velocities [N, 3], copied to the host (waits for the stream)."""
        return (("flags", np.int32, self.R), ("n_steps", np.int64, self.R), ("heat", np.float64, self.R),
                ("v", np.float64, (self.N, 3)))


def pimd_step(state: PimdState, forces: torch.Tensor, finish_only: bool = False) -> None:
    """One call of the batch (m3g_pimd_step) at `forces` [N,3] float32 evaluated at `state.pos`: finish the step that ends here, write
    `state.obs`, start the next one (not with `finish_only`).  Three launches, queued on the current stream; no wait, capture-safe."""
    state.step(forces, finish_only)


LOG_KEYS = ("time", "temperature", "ring_kinetic", "spring_energy", "potential", "kinetic_primitive", "kinetic_centroid_virial",
            "conserved")


class PathIntegralMD(Driver):
    """Path-integral MD of a batch of structures: every structure a ring polymer of `n_beads` beads (1 .. 64, odd or even).

    `model`: the `Gradient` returned by `build_model`.  `temperature`: K, > 0, one value or one per structure (the physical
    temperature T: the beads move at P T).  `timestep` in fs.  thermostat: "pile_l" (white-noise Langevin in the ring's normal modes:
    `centroid_friction` in 1/fs on the centroid, 2 `pile_lambda` w_k on mode k; `centroid_friction` = 0 is thermostatted ring-polymer
    MD) or "none" (microcanonical ring-polymer MD).  `ring_batches`: True evaluates every ring as an engine batch of its own -- the
    engine's fp32 rounding depends on the composition of its batch (as `ReplicaExchange.ladder_batches`), so only then are a ring's
    numbers bitwise the same alone or beside other rings, at one engine call per ring and step; False evaluates all beads of all
    rings in one engine batch.  `seed`: an integer, or one per structure: the starting velocities of a ring's beads and the key of
    its thermostat derive from the ring's own seed."""

    def __init__(self, model: Gradient, n_beads: int, temperature=300.0, timestep: float = 0.5, thermostat: str = "pile_l",
                 centroid_friction: float = 0.01, pile_lambda: float = 0.5, skin: float = 0.5, seed=0, device="cuda",
                 ring_batches: bool = True):
        super().__init__(model, skin, device)
        self.n_beads, self.thermostat = bead_count(n_beads), thermostat_name(thermostat)
        self.timestep = positive("timestep", timestep)
        self.centroid_friction = non_negative("centroid_friction", centroid_friction)
        self.pile_lambda = non_negative("pile_lambda", pile_lambda)
        self.ring_batches = boolean("ring_batches", ring_batches)
        t = np.asarray(temperature, dtype=np.float64)
        if t.ndim > 1 or not (np.isfinite(t).all() and (t > 0).all()):
            raise ValueError("temperature must be one finite value > 0 (K) or one per structure")
        self.temperature = t
        self.seed = seed

    def run(self, lattices: Sequence, positions: Sequence, atomic_numbers: Sequence, steps: int, masses: Sequence | None = None,
            loginterval: int = 10) -> list:
        """Run every structure's ring for `steps` steps.  lattices: [3,3] rows = lattice vectors; atomic_numbers: [n]; positions[i]:
        [n,3] -- every bead starts there, with Maxwell-Boltzmann velocities at P T per bead -- or [P,n,3] to continue a ring (the
        velocities are drawn anew); masses: [n] amu per structure (default: standard atomic weights).  Returns one dict per input
        structure: `log` (arrays, one entry every `loginterval` steps and at the last one: time fs, temperature K = 2 KE_ring / (3 n P^2
        kB), ring_kinetic, spring_energy, potential = the mean of the beads' energies, kinetic_primitive, kinetic_centroid_virial and
        conserved = sum_j E_j + KE_ring + E_spring - the heat the thermostat added, all eV), the final positions and velocities
        [P,n,3] (unwrapped), centroid [n,3], n_steps and error (a force of one of its beads became non-finite: the ring was stopped
        where it stood)."""
        steps, loginterval = integer("steps", steps, 0), integer("loginterval", loginterval, 1)
        P = self.n_beads
        if not (len(lattices) == len(positions) == len(atomic_numbers)) or len(lattices) == 0:
            raise ValueError("lattices, positions and atomic_numbers must hold one entry per structure (at least one)")
        G = len(lattices)
        lat_r, pos_r, z_r = [], [], []
        for g, (L, p, a) in enumerate(zip(lattices, positions, atomic_numbers)):
            p = np.asarray(p, dtype=np.float64)
            if p.ndim == 2:
                p = np.broadcast_to(p, (P,) + p.shape)
            if p.ndim != 3 or p.shape[0] != P:
                raise ValueError(f"structure {g}: positions must be [n, 3] or [n_beads = {P}, n, 3]; got {p.shape}")
            lat_r += [L] * P
            pos_r += list(p)
            z_r += [a] * P
        lat_r, pos_r, z_r = structure_arrays(lat_r, pos_r, z_r)
        temps = per_structure("temperature", self.temperature, G)
        m = structure_masses(masses, z_r[::P])
        # a ring's keys derive from its own seed only: P velocity seeds of its beads, then the key of its thermostat
        keys = derived_keys(self.seed, G, P + 1)
        vel = [maxwell_boltzmann(m[g], P * temps[g], int(keys[g][j])) for g in range(G) for j in range(P)]
        groups = [(g * P, (g + 1) * P) for g in range(G)] if self.ring_batches else [(0, G * P)]
        ev = MdBatch(self.model, lat_r, pos_r, z_r, groups, self.skin, self.device, cells=False)
        pos_t, offsets = ev.pos, ev.offsets
        state = PimdState(pos_t, offsets, np.concatenate(replicated(m, P)), torch.tensor(np.concatenate(vel), device=ev.device), temps,
                          np.array([k[-1] for k in keys], dtype=np.uint64), P, thermostat=self.thermostat, dt=self.timestep,
                          centroid_friction=self.centroid_friction, pile_lambda=self.pile_lambda)
        rows = {key: [] for key in LOG_KEYS}

        def log(k, out):
            obs = state.obs.cpu().numpy()
            e_sum = out[K.TOTAL_ENERGY].double().cpu().numpy().reshape(G, P).sum(1)
            rows["time"].append(np.full(G, k * self.timestep))
            for key, col in (("ring_kinetic", 0), ("temperature", 1), ("spring_energy", 2), ("kinetic_primitive", 3),
                             ("kinetic_centroid_virial", 4)):
                rows[key].append(obs[:, col])
            rows["potential"].append(e_sum / P)
            rows["conserved"].append(e_sum + obs[:, 0] + obs[:, 2] - obs[:, 5])

        md_loop(ev, state, steps, None, log=log, loginterval=loginterval)
        ev.raise_on_step_errors("path-integral molecular dynamics")
        st = state.read()
        p_host = pos_t.cpu().numpy()
        logs = {key: np.stack(val, axis=1) for key, val in rows.items()}   # [G, n_log]
        res = []
        for g in range(G):
            a, b = int(offsets[g * P]), int(offsets[(g + 1) * P])
            beads = p_host[a:b].reshape(P, -1, 3)
            res.append({"positions": beads.copy(), "velocities": st["v"][a:b].reshape(P, -1, 3).copy(), "centroid": beads.mean(0),
                        "n_steps": int(st["n_steps"][g]), "error": bool(st["flags"][g] & _lib.DYN_ERROR),
                        "log": {key: val[g].copy() for key, val in logs.items()}})
        return res
