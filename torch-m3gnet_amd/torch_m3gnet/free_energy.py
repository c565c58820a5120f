"""Batched anharmonic Helmholtz free energies of crystals on the device (C ABI: m3g_ti_*, csrc/m3g_ti.hip): Frenkel-Ladd thermodynamic
integration to an Einstein crystal (Frenkel, Ladd, J. Chem. Phys. 81, 3188 (1984)), by non-equilibrium switching (`FreeEnergy.switch`;
Freitas, Asta, de Koning, Comput. Mater. Sci. 112, 333 (2016), the method of LAMMPS' fix ti/spring) or by equilibrium sampling at the
Gauss-Legendre nodes of the coupling (`FreeEnergy.integrate`).

Every structure moves under H(lambda) = KE + lambda E_model(x) + (1 - lambda) U_s(x), U_s = 1/2 sum_i k_i |x_i - r0_i|^2 about its
starting sites r0, by BAOAB Langevin dynamics whose centre of mass is held exactly -- without that, <dH/dlambda> diverges
logarithmically towards the model's end, where nothing ties the crystal to the sites.  dH/dlambda = E_model - U_s; its integral over
lambda from 0 to 1 is F_model - F_Einstein(centre of mass held), and `einstein_free_energy` supplies the closed forms of the Einstein
crystal and of the constraint.  Per step the forces and energies of the whole batch come from `VerletGraph.step` and the integrator --
mixing the two forces, the constraint, the thermostat, the switching work and the running statistics of dH/dlambda -- is three kernel
launches (`ti_step`).

Not here: constant pressure (the cell is fixed: relax or equilibrate it first and pass its volume), liquids (no Uhlenbeck-Ford
reference), reversible-scaling temperature sweeps, and quantum corrections (classical nuclei: see `path_integral`).

Units as in `dynamics`: A, fs, amu, eV, K; spring constants in eV/A^2."""
from __future__ import annotations

import math
from typing import Sequence

import numpy as np
import torch

from . import _cuda, _lib
from ._driver import (Driver, IntegratorState, MdBatch, boolean, derived_keys, integer, md_loop, non_negative, positive, replicated,
                      state_tensor, structure_arrays, structure_masses)
from .data import MaterialGraphKey as K
from .data.graph_gpu import _ptr, _stream
from .dynamics import KAPPA, KB, maxwell_boltzmann
from .nn.modules import Gradient
from .path_integral import HBAR

SCHEDULES = {"linear": _lib.TI_LINEAR, "smooth": _lib.TI_SMOOTH}


def schedule_name(x) -> str:
    """`schedule`: "linear" or "smooth"."""
    if not isinstance(x, str) or x not in SCHEDULES:
        raise ValueError(f"unknown schedule {x!r}; expected one of {sorted(SCHEDULES)}")
    return x


def einstein_free_energy(masses, spring_constants, temperature: float, volume: float, n_cells: int | None = None) -> dict:
    """The closed forms of one Einstein crystal (host, fp64): `masses` [n] amu, `spring_constants` [n] eV/A^2 (one value: for all),
    `temperature` K, `volume` A^3, `n_cells` the number of primitive cells in the cell (default: n, right for a monatomic Bravais
    crystal).  Returns f_einstein = -kB T sum_i 3 ln(kB T / (hbar w_i)), w_i = sqrt(kappa k_i / m_i), the classical free energy of the
    3 n oscillators, and f_com = 3/2 kB T ln(2 pi s^2) + kB T ln(n_cells / V), s^2 = kB T sum_i (m_i / M)^2 / k_i, what holding the
    centre of mass of that crystal takes out and the crystal's freedom to sit anywhere in a primitive cell puts back (for equal
    masses and springs kB T ln[(n / V) (2 pi kB T / (n k))^(3/2)], eq. 24 of Freitas et al.); both eV for the whole cell."""
    m = np.asarray(masses, dtype=np.float64).reshape(-1)
    k = np.ascontiguousarray(np.broadcast_to(np.asarray(spring_constants, dtype=np.float64), m.shape))
    kt = KB * positive("temperature", temperature)
    volume = positive("volume", volume)
    if len(m) == 0 or not (np.isfinite(m).all() and (m > 0).all()):
        raise ValueError("masses must be finite values > 0 (at least one)")
    if not (np.isfinite(k).all() and (k > 0).all()):
        raise ValueError("spring_constants must be finite values > 0")
    n_cells = len(m) if n_cells is None else integer("n_cells", n_cells, 1)
    omega = np.sqrt(KAPPA * k / m)
    s2 = kt * ((m / m.sum()) ** 2 / k).sum()
    return {"f_einstein": float(-kt * (3.0 * np.log(kt / (HBAR * omega))).sum()),
            "f_com": float(1.5 * kt * math.log(2.0 * math.pi * s2) + kt * math.log(n_cells / volume))}


class TiState(IntegratorState):
    """State of a thermodynamic-integration batch on the device (m3g_ti_init), shaped like `PimdState`: `pos` [N,3] fp64 (unwrapped)
    is the caller's tensor, moved IN PLACE by `ti_step`; the `velocities` and `reference` arguments [N,3] fp64 are copied, the
    `velocities` attribute is the live view of the integrator's own.  `offsets`: S + 1 atom offsets (two atoms per structure at
    least); `masses`, `springs` [N] (amu, eV/A^2 >= 0, not all of a structure's zero); `temperatures` and `seeds`: one per structure
    (or one temperature for all).  dt in fs, `friction` in 1/fs (0: velocity Verlet on the constrained force).  Neither centre-of-mass
    velocity nor displacement is removed here: start from sum m v = 0.  The path starts as lambda = 1 throughout; `ti_path` sets
    another.  `obs` [S,8] (KE eV, T = 2 KE / ((3 n - 3) kB) K, U_s, dH/dlambda, lambda, work, 0, 0) is written by every `ti_step`."""
    FAMILY, OBS, SECOND = "ti", _lib.TI_OBS, ("energies", (), None)

    def __init__(self, pos: torch.Tensor, offsets: Sequence[int], masses, springs, velocities: torch.Tensor, reference: torch.Tensor,
                 temperatures, seeds, schedule: str = "smooth", dt: float = 1.0, friction: float = 0.01):
        self.schedule = schedule_name(schedule)
        self.params = _lib.M3GTiParams(schedule=SCHEDULES[self.schedule], reserved=0, dt=dt, friction=friction)
        self._layout(pos, None, offsets)
        self._rows("velocities", velocities)
        self._rows("reference", reference)
        self.springs = np.ascontiguousarray(np.asarray(springs, dtype=np.float64).reshape(-1))
        if not self._host_arrays(masses, temperatures, seeds) or len(self.springs) != self.N:
            raise ValueError(f"expected {self.N} masses, {self.N} springs and {self.S} seeds (one per structure)")
        self._allocate(state_tensor, self.N, self.S)
        self._init(self.springs, self.temperatures, self.seeds, velocities, reference)

    def _fields(self):
        """`read()`: flags / n_steps / work / count / mean / m2 [S] (Welford's accumulators of dH/dlambda), the velocities [N, 3] and
        the per-atom sums of |x - r0|^2 over the `count` samples [N], copied to the host (waits for the stream)."""
        return (("flags", np.int32, self.S), ("n_steps", np.int64, self.S), ("work", np.float64, self.S),
                ("count", np.int64, self.S), ("mean", np.float64, self.S), ("m2", np.float64, self.S),
                ("v", np.float64, (self.N, 3)), ("msd_sum", np.float64, self.N))


def ti_path(state: TiState, lambda_begin, lambda_end, n_switch: int, n_discard: int = 0) -> None:
    """A new path for the batch (m3g_ti_path): lambda runs from `lambda_begin` to `lambda_end` (one value or one per structure, in
    [0, 1]; equal: fixed coupling) over `n_switch` steps by the state's schedule and stays there; dH/dlambda and |x - r0|^2 are
    sampled from step `n_discard` on.  The work, the step index and the accumulators start anew.  Waits for the stream."""
    lb = np.ascontiguousarray(np.broadcast_to(np.asarray(lambda_begin, dtype=np.float64), (state.S,)))
    le = np.ascontiguousarray(np.broadcast_to(np.asarray(lambda_end, dtype=np.float64), (state.S,)))
    with _cuda.on_device(state.device):
        _lib.check(state.lib.m3g_ti_path(state.N, state.S, _ptr(state.state), state.state.numel(), lb.ctypes.data, le.ctypes.data,
                                         integer("n_switch", n_switch, 0), integer("n_discard", n_discard, 0), _stream()))


def ti_step(state: TiState, forces: torch.Tensor, energies: torch.Tensor, finish_only: bool = False) -> None:
    """One call of the batch (m3g_ti_step) at the model's `forces` [N,3] and `energies` [S] (float32) evaluated at `state.pos`: finish
    the step that ends here, add to the work and the statistics, write `state.obs`, start the next step (not with `finish_only`).
    Three launches, queued on the current stream; no wait, capture-safe."""
    state.step(forces, finish_only, energies)


LOG_KEYS = ("stage", "step", "temperature", "lambda", "dh_dlambda", "spring_energy", "potential", "work")


class FreeEnergy(Driver):
    """Helmholtz free energies of a batch of crystals by thermodynamic integration to Einstein crystals about their starting sites.

    `model`: the `Gradient` returned by `build_model`.  `temperature`: K, > 0.  `spring_constant` (eV/A^2): one value for every atom,
    a {Z: k} dict by species, one array [n] per structure, or "msd": the driver first runs `msd_steps` steps under the model alone
    and sets k_Z = 3 kB T / <|u|^2> per species from the device's sums over the second half of them (the choice of Freitas et al.:
    the Einstein crystal that moves as far as the real one).  `timestep` fs, `friction` 1/fs, `schedule`: "smooth" or "linear", how
    lambda runs in `switch`.  Every input structure becomes `replicas` independent copies in one batch, with velocities and
    thermostat keys derived from its own seed (`seed`: an integer, or one per structure).  `structure_batches`: True evaluates every
    input's copies as an engine batch of their own -- the engine's fp32 rounding depends on the composition of its batch (as
    `PathIntegralMD.ring_batches`), so only then are a structure's numbers bitwise the same alone or beside other inputs; False
    evaluates all copies of all inputs in one engine batch.

    The cell is fixed and the atoms start ON the sites they are tied to, so pass relaxed (or time-averaged) positions.  The method
    rests on the model's forces being the gradient of its energy: the M3GNet energy steps where a pair crosses the two-body cutoff,
    so a neighbour shell within a few thermal amplitudes of the cutoff biases the result.  Not here:
    constant pressure, liquids, reversible-scaling temperature sweeps and quantum corrections."""

    def __init__(self, model: Gradient, temperature: float, spring_constant, timestep: float = 1.0, friction: float = 0.01,
                 schedule: str = "smooth", replicas: int = 4, seed=0, skin: float = 0.5, device="cuda", structure_batches: bool = True,
                 msd_steps: int = 1000):
        super().__init__(model, skin, device)
        self.temperature = positive("temperature", temperature)
        self.timestep = positive("timestep", timestep)
        self.friction = non_negative("friction", friction)
        self.schedule = schedule_name(schedule)
        self.replicas = integer("replicas", replicas, 1)
        self.structure_batches = boolean("structure_batches", structure_batches)
        self.msd_steps = integer("msd_steps", msd_steps, 2)
        if isinstance(spring_constant, str):
            if spring_constant != "msd":
                raise ValueError(f'spring_constant: the only mode by name is "msd"; got {spring_constant!r}')
        elif isinstance(spring_constant, dict):
            if not spring_constant or not all(math.isfinite(float(k)) and float(k) > 0 for k in spring_constant.values()):
                raise ValueError("spring_constant: a {Z: k} dict needs finite values > 0")
        elif np.ndim(spring_constant) == 0:
            positive("spring_constant", spring_constant)
        self.spring_constant = spring_constant
        self.seed = seed

    # ---- the batch: every input R times ------------------------------------------------------------------------------------------
    def _springs(self, z: list) -> list | None:
        """[n] spring constants per input structure from `spring_constant`; None in "msd" mode."""
        k = self.spring_constant
        if isinstance(k, str):
            return None
        if isinstance(k, dict):
            missing = sorted({int(a) for zs in z for a in zs} - {int(a) for a in k})
            if missing:
                raise ValueError(f"spring_constant: no entry for the species {missing}")
            table = {int(a): float(v) for a, v in k.items()}
            return [np.array([table[int(a)] for a in zs]) for zs in z]
        if np.ndim(k) == 0:
            return [np.full(len(zs), float(k)) for zs in z]
        if len(k) != len(z):
            raise ValueError("spring_constant: expected one array per structure")
        out = [np.asarray(x, dtype=np.float64).reshape(-1) for x in k]
        for s, (ks, zs) in enumerate(zip(out, z)):
            if len(ks) != len(zs) or not (np.isfinite(ks).all() and (ks > 0).all()):
                raise ValueError(f"spring_constant: structure {s} needs {len(zs)} finite values > 0")
        return out

    def _batch(self, lat, pos, z, m, springs, copies: int):
        """The `MdBatch` of `copies` copies of every input and their `TiState`, every atom tied to its starting site by `springs`."""
        G = len(z)
        groups = [(g * copies, (g + 1) * copies) for g in range(G)] if self.structure_batches else [(0, G * copies)]
        rep = lambda xs: replicated(xs, copies)   # noqa: E731
        ev = MdBatch(self.model, rep(lat), rep(pos), rep(z), groups, self.skin, self.device, cells=False)
        keys = derived_keys(self.seed, G, 2 * copies)   # of every copy: its velocity seed, then the key of its thermostat
        vel = [maxwell_boltzmann(m[g], self.temperature, int(keys[g][2 * r])) for g in range(G) for r in range(copies)]
        seeds = np.array([keys[g][2 * r + 1] for g in range(G) for r in range(copies)], dtype=np.uint64)
        state = TiState(ev.pos, ev.offsets, np.concatenate(rep(m)), np.concatenate(rep(springs)),
                        torch.tensor(np.concatenate(vel), dtype=torch.float64, device=ev.device), ev.pos.clone(), self.temperature, seeds,
                        schedule=self.schedule, dt=self.timestep, friction=self.friction)
        return ev, state

    def _stage(self, ev: MdBatch, state: TiState, n_steps: int, rows: dict | None, stage: int, loginterval: int) -> None:
        """`n_steps` steps of the state's current path (n_steps + 1 evaluations, the last one finishing only)."""
        def log(k, out):
            obs = state.obs.cpu().numpy()
            rows["stage"].append(np.full(ev.S, stage))
            rows["step"].append(np.full(ev.S, k))
            rows["potential"].append(out[K.TOTAL_ENERGY].double().cpu().numpy())
            for key, col in (("temperature", 1), ("spring_energy", 2), ("dh_dlambda", 3), ("lambda", 4), ("work", 5)):
                rows[key].append(obs[:, col])

        md_loop(ev, state, n_steps, K.TOTAL_ENERGY, log=None if rows is None else log, loginterval=loginterval)

    def _inputs(self, lattices, positions, atomic_numbers, masses, n_cells):
        lat, pos, z = structure_arrays(lattices, positions, atomic_numbers)
        if min(len(a) for a in z) < 2:
            raise ValueError("positions: every structure needs at least two atoms (the centre of mass is held)")
        m = structure_masses(masses, z)
        cells = [len(a) for a in z] if n_cells is None else [integer("n_cells", c, 1) for c in np.broadcast_to(n_cells, (len(z),))]
        return lat, pos, z, m, cells

    def _msd_springs(self, lat, pos, z, m) -> list:
        """k_Z = 3 kB T / <|u|^2> per species and input structure, from `msd_steps` steps at lambda = 1 (the second half sampled)."""
        R = self.replicas
        ev, state = self._batch(lat, pos, z, m, [np.ones(len(a)) for a in z], R)   # (lambda = 1: the springs pull at nothing)
        ti_path(state, 1.0, 1.0, 0, self.msd_steps // 2)
        self._stage(ev, state, self.msd_steps, None, 0, 1)
        ev.raise_on_step_errors("the mean-square-displacement run of the free-energy driver")
        st = state.read()
        out = []
        for g, zs in enumerate(z):
            a, n = int(ev.offsets[g * R]), len(zs)
            if (st["flags"][g * R:(g + 1) * R] & _lib.DYN_ERROR).any():
                raise RuntimeError(f"structure {g}: non-finite forces or energies in the mean-square-displacement run")
            msd = (st["msd_sum"][a:a + R * n].reshape(R, n) / st["count"][g * R:(g + 1) * R, None]).mean(0)
            k = np.empty(n)
            for species in np.unique(zs):
                k[zs == species] = 3.0 * KB * self.temperature / msd[zs == species].mean()
            out.append(k)
        return out

    def _prepare(self, lattices, positions, atomic_numbers, masses, n_cells):
        lat, pos, z, m, cells = self._inputs(lattices, positions, atomic_numbers, masses, n_cells)
        springs = self._springs(z)
        if springs is None:
            springs = self._msd_springs(lat, pos, z, m)
        closed = [einstein_free_energy(m[g], springs[g], self.temperature, abs(np.linalg.det(lat[g])), cells[g]) for g in range(len(z))]
        return lat, pos, z, m, springs, closed

    # ---- non-equilibrium switching ---------------------------------------------------------------------------------------------------
    def switch(self, lattices: Sequence, positions: Sequence, atomic_numbers: Sequence, equilibration: int, switch_steps: int,
               masses: Sequence | None = None, n_cells=None, loginterval: int = 10) -> list:
        """The free energy of every structure by one forward and one backward switch per replica: `equilibration` steps under the
        model (lambda = 1), `switch_steps` steps from 1 to 0 (work W10), `equilibration` steps in the Einstein crystal, `switch_steps`
        steps back (W01).  lattices: [3,3] rows = lattice vectors; positions[i]: [n,3], the sites; atomic_numbers: [n]; masses: [n]
        amu per structure (default: standard atomic weights); n_cells: primitive cells per cell (default: n, a monatomic Bravais
        crystal).  Returns one dict per input structure: delta_f = (W01 - W10) / 2 and dissipation = (W01 + W10) / 2 per replica [R]
        (the dissipated work cancels in the first to leading order and is what the second measures: it falls as 1 / switch_steps),
        free_energy = f_einstein + f_com + mean(delta_f) and free_energy_error, the standard error over the replicas (nan for one),
        per_atom = free_energy / n, work_forward = W10, work_backward = W01, f_einstein, f_com, spring_constants [n], n_steps,
        error (a force or energy of one of its replicas became non-finite: that replica stopped where it stood, and the numbers
        above are not to be used) and `log` (arrays [R, n_log]: stage 0 .. 3, step, temperature K, lambda, dh_dlambda, spring_energy,
        potential, work; one entry every `loginterval` steps of a stage and at its last)."""
        equilibration, switch_steps = integer("equilibration", equilibration, 0), integer("switch_steps", switch_steps, 1)
        loginterval = integer("loginterval", loginterval, 1)
        lat, pos, z, m, springs, closed = self._prepare(lattices, positions, atomic_numbers, masses, n_cells)
        G, R = len(z), self.replicas
        ev, state = self._batch(lat, pos, z, m, springs, R)
        rows = {key: [] for key in LOG_KEYS}
        work = []
        for stage, (lb, le, n) in enumerate(((1.0, 1.0, equilibration), (1.0, 0.0, switch_steps), (0.0, 0.0, equilibration),
                                             (0.0, 1.0, switch_steps))):
            ti_path(state, lb, le, n if lb != le else 0)
            self._stage(ev, state, n, rows, stage, loginterval)
            if lb != le:
                work.append(state.read()["work"])
        ev.raise_on_step_errors("thermodynamic integration")
        st = state.read()
        w10, w01 = work
        logs = {key: np.stack(val, axis=1) for key, val in rows.items()}   # [S, n_log]
        res = []
        for g in range(G):
            sl = slice(g * R, (g + 1) * R)
            df, n = 0.5 * (w01[sl] - w10[sl]), len(z[g])
            f = closed[g]["f_einstein"] + closed[g]["f_com"] + df.mean()
            res.append({"free_energy": float(f), "free_energy_error": float(df.std(ddof=1) / math.sqrt(R)) if R > 1 else float("nan"),
                        "per_atom": float(f / n), "delta_f": df, "dissipation": 0.5 * (w01[sl] + w10[sl]), "work_forward": w10[sl].copy(),
                        "work_backward": w01[sl].copy(), "f_einstein": closed[g]["f_einstein"], "f_com": closed[g]["f_com"],
                        "spring_constants": springs[g].copy(), "n_steps": int(st["n_steps"][sl].min()),
                        "error": bool((st["flags"][sl] & _lib.DYN_ERROR).any()), "log": {key: val[sl].copy() for key, val in logs.items()}})
        return res

    # ---- equilibrium sampling at the Gauss-Legendre nodes ----------------------------------------------------------------------------
    def integrate(self, lattices: Sequence, positions: Sequence, atomic_numbers: Sequence, equilibration: int, steps: int,
                  n_lambda: int = 8, masses: Sequence | None = None, n_cells=None, loginterval: int = 10, blocks: int = 10) -> list:
        """The free energy of every structure by equilibrium sampling: each becomes a ladder of `n_lambda` copies (not `replicas`), copy
        j at the j-th Gauss-Legendre node of [0, 1] throughout, run for `equilibration` + `steps` steps with dH/dlambda sampled by
        the device over the last `steps` + 1.  Returns one dict per input structure: lambdas and weights [n_lambda], mean and
        variance of dH/dlambda per node (the device's Welford accumulators), standard_error per node (from `blocks` block means of
        the log's entries after the equilibration: needs at least 2 entries per block), delta_f = sum_j w_j mean_j and
        delta_f_error = sqrt(sum_j (w_j standard_error_j)^2), free_energy = f_einstein + f_com + delta_f, per_atom, f_einstein, f_com,
        spring_constants, n_steps, error and `log` (as `switch`, stage 0)."""
        equilibration, steps = integer("equilibration", equilibration, 0), integer("steps", steps, 1)
        n_lambda, loginterval, blocks = integer("n_lambda", n_lambda, 1), integer("loginterval", loginterval, 1), integer("blocks", blocks, 2)
        lat, pos, z, m, springs, closed = self._prepare(lattices, positions, atomic_numbers, masses, n_cells)
        G, J = len(z), n_lambda
        x, w = np.polynomial.legendre.leggauss(J)
        nodes, weights = 0.5 * (x + 1.0), 0.5 * w
        ev, state = self._batch(lat, pos, z, m, springs, J)
        rows = {key: [] for key in LOG_KEYS}
        ladder = np.tile(nodes, G)
        ti_path(state, ladder, ladder, 0, equilibration)
        self._stage(ev, state, equilibration + steps, rows, 0, loginterval)
        ev.raise_on_step_errors("thermodynamic integration")
        st = state.read()
        logs = {key: np.stack(val, axis=1) for key, val in rows.items()}
        sampled = logs["step"][0] >= equilibration
        per_block = int(sampled.sum()) // blocks
        res = []
        for g in range(G):
            sl = slice(g * J, (g + 1) * J)
            mean, n = st["mean"][sl], len(z[g])
            if per_block >= 2:
                d = logs["dh_dlambda"][sl][:, sampled][:, :per_block * blocks].reshape(J, blocks, per_block).mean(2)
                se = d.std(axis=1, ddof=1) / math.sqrt(blocks)
            else:
                se = np.full(J, np.nan)
            df = float((weights * mean).sum())
            f = closed[g]["f_einstein"] + closed[g]["f_com"] + df
            res.append({"free_energy": f, "per_atom": f / n, "delta_f": df, "delta_f_error": float(np.sqrt(((weights * se) ** 2).sum())),
                        "lambdas": nodes.copy(), "weights": weights.copy(), "mean": mean.copy(),
                        "variance": st["m2"][sl] / np.maximum(st["count"][sl] - 1, 1), "standard_error": se,
                        "f_einstein": closed[g]["f_einstein"], "f_com": closed[g]["f_com"], "spring_constants": springs[g].copy(),
                        "n_steps": int(st["n_steps"][sl].min()), "error": bool((st["flags"][sl] & _lib.DYN_ERROR).any()),
                        "log": {key: val[sl].copy() for key, val in logs.items()}})
        return res
