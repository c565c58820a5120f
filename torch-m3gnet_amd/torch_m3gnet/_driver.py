"""What the batched drivers (relax, dynamics, replica_exchange, monte_carlo, trajectory, neb, phonons, elasticity) share on the host:
argument checks, the model every driver evaluates, state allocation and read-back, the device state of the five MD step families
(`IntegratorState`: dynamics, path_integral, free_energy), the split of one structure's copies into engine sub-batches, the
evaluation of a batch in engine groups (`GroupedEvaluation`) and the run of the eight drivers that integrate (dynamics, transport,
normal_modes, metadynamics, replica_exchange, monte_carlo, path_integral, free_energy): `MdBatch`, `md_loop` -- the one place that
says when a step only finishes, how a synchronous point restarts and which steps are logged --, `MdLog` / `md_results`,
`derived_keys` and `replicated`; their Langevin warm-up is `dynamics.langevin_warm_up`, beside the `DynState` it makes.  The optimiser
loop relax and neb share is `relax.fire_loop`, beside `fire_step` / `lbfgs_step`; the status read after the last evaluation is
`VerletGraph.raise_on_step_errors`."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _cuda, _lib
from .data import MaterialGraphKey as K
from .data.atomic_masses import masses_of
from .data.graph_gpu import _ptr, _stream
from .data.md import VerletGraph
from .nn.modules import Gradient

EV_A3_TO_GPA = 160.21766208


def positive(name: str, x) -> float:
    x = float(x)
    if not (math.isfinite(x) and x > 0.0):
        raise ValueError(f"{name} must be a finite number > 0; got {x}")
    return x


def non_negative(name: str, x) -> float:
    x = float(x)
    if not (math.isfinite(x) and x >= 0.0):
        raise ValueError(f"{name} must be a finite number >= 0; got {x}")
    return x


def integer(name: str, x, least: int) -> int:
    if isinstance(x, bool) or int(x) != x or x < least:
        raise ValueError(f"{name} must be an integer >= {least}; got {x}")
    return int(x)


def boolean(name: str, x) -> bool:
    if not isinstance(x, (bool, np.bool_)):
        raise ValueError(f"{name} must be True or False; got {x!r}")
    return bool(x)


def structure_arrays(lattices, positions, atomic_numbers):
    """The structure lists every driver takes, checked: ([3,3] fp64 lattices, [n_s,3] fp64 positions, [n_s] atomic numbers)."""
    if not (len(lattices) == len(positions) == len(atomic_numbers)) or len(lattices) == 0:
        raise ValueError("lattices, positions and atomic_numbers must hold one entry per structure (at least one)")
    lat = [np.asarray(L, dtype=np.float64) for L in lattices]
    pos = [np.asarray(p, dtype=np.float64) for p in positions]
    z = [np.asarray(a).reshape(-1) for a in atomic_numbers]
    for s, (L, p, a) in enumerate(zip(lat, pos, z)):
        if L.shape != (3, 3):
            raise ValueError(f"structure {s}: lattice must be [3, 3]; got {L.shape}")
        if p.ndim != 2 or p.shape[1] != 3 or p.shape[0] != len(a) or len(a) == 0:
            raise ValueError(f"structure {s}: positions must be [n, 3] with n = len(atomic_numbers) >= 1; got {p.shape} for {len(a)} atoms")
        if not (np.isfinite(L).all() and np.isfinite(p).all()):
            raise ValueError(f"structure {s}: non-finite lattice or positions")
        if abs(np.linalg.det(L)) < 1e-12:
            raise ValueError(f"structure {s}: singular lattice")
    return lat, pos, z


def structure_masses(masses, z) -> list:
    """[n_s] fp64 masses (amu) per structure: the caller's, checked, or the standard atomic weights of `z`."""
    if masses is None:
        return [masses_of(a) for a in z]
    if len(masses) != len(z):
        raise ValueError("masses: expected one array per structure")
    m = [np.asarray(x, dtype=np.float64).reshape(-1) for x in masses]
    for s, (ms, a) in enumerate(zip(m, z)):
        if len(ms) != len(a) or not (np.isfinite(ms).all() and (ms > 0).all()):
            raise ValueError(f"structure {s}: masses must be {len(a)} finite values > 0")
    return m


def per_structure(name: str, x: np.ndarray, n_structs: int) -> np.ndarray:
    """[S] view of `x` (checked at construction: 0-d or 1-d): the one value for every structure, or the caller's S values."""
    if x.ndim != 0 and len(x) != n_structs:
        raise ValueError(f"{name}: expected one value or one per structure ({n_structs}); got {len(x)}")
    return np.broadcast_to(x, (n_structs,))


def atom_offsets(z: list) -> np.ndarray:
    """S + 1 atom offsets of a batch from its per-structure arrays (species, say)."""
    return np.concatenate([[0], np.cumsum([len(a) for a in z])])


def structure_seeds(seed, n_structs: int) -> np.ndarray:
    """Per-structure 64-bit Philox keys: `seed` itself when it is a sequence of S integers, else derived from (seed, s)."""
    if np.ndim(seed) == 1:
        seeds = np.asarray(seed, dtype=np.uint64)
        if len(seeds) != n_structs:
            raise ValueError(f"seed: expected one per structure ({n_structs}); got {len(seeds)}")
        return seeds
    return np.array([np.random.SeedSequence([int(seed), s]).generate_state(1, np.uint64)[0] for s in range(n_structs)], dtype=np.uint64)


def derived_keys(seed, n_inputs: int, per_input) -> list:
    """`per_input` keys (one count, or one per input) for every input: a copy's keys derive from its input's own seed only, so an
    input's run does not depend on its neighbours."""
    return [structure_seeds(int(sd), int(n)) for sd, n in zip(structure_seeds(seed, n_inputs), np.broadcast_to(per_input, (n_inputs,)))]


def replicated(xs, copies: int) -> list:
    """Every entry of `xs` `copies` times, the copies of an entry side by side."""
    return [x for x in xs for _ in range(copies)]


def check_tensor(name: str, x: torch.Tensor, shape: tuple, dtype: torch.dtype, device=None) -> None:
    """`x` is a contiguous `dtype` tensor of `shape` (a string entry stands for any size), on `device` when one is given."""
    fits = x.dim() == len(shape) and all(isinstance(n, str) or d == n for d, n in zip(x.shape, shape))
    if x.dtype != dtype or not fits or not x.is_contiguous() or (device is not None and x.device != device):
        where = "" if device is None else f" on {device}"
        raise ValueError(f"{name} must be a contiguous [{', '.join(map(str, shape))}] {str(dtype).split('.')[-1]} tensor{where}")


def batch_layout(pos: torch.Tensor, lattice: torch.Tensor | None, offsets):
    """(offsets int64, N, S) of a state over the caller's `pos` [N,3] / `lattice` [S,3,3] (fp64, moved in place), checked."""
    check_tensor("pos", pos, ("N", 3), torch.float64)
    offsets = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64))
    n_structs = int(len(offsets) - 1)
    if n_structs < 1:
        raise ValueError("offsets must hold S + 1 >= 2 entries")
    if lattice is not None:
        check_tensor("lattice", lattice, (n_structs, 3, 3), torch.float64)
    return offsets, int(pos.size(0)), n_structs


def gpu_device(device, what: str) -> torch.device:
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError(f"{what} runs on a GPU device; got {device}")
    return torch.device("cuda", torch.cuda.current_device()) if device.index is None else device


def state_tensor(state_bytes, *sizes, device) -> torch.Tensor:
    """The uint8 tensor of a device state, of the size `state_bytes` (an m3g_*_state_bytes) gives for `sizes`."""
    nbytes = C.c_size_t()
    _lib.check(state_bytes(*sizes, C.byref(nbytes)))
    return torch.empty(nbytes.value, dtype=torch.uint8, device=device)


def read_state(read, sizes: tuple, state: torch.Tensor, fields) -> dict:
    """A state's arrays copied to the host by its m3g_*_read (waits for the stream).  `fields`: (name, dtype, shape) in the order of the
    host pointers `read` takes after (*sizes, state, state_bytes)."""
    out = {name: np.empty(shape, dtype) for name, dtype, shape in fields}
    with _cuda.on_device(state.device):
        _lib.check(read(*sizes, _ptr(state), state.numel(), *(a.ctypes.data for a in out.values()), _stream()))
    return out


class IntegratorState:
    """What the device states of the five MD step families share (`DynState`, `NhcState`, `MtkCellState`, `PimdState`, `TiState`; C
    ABI m3g_<FAMILY>_*, device side csrc/m3g_integrator.h).  A subclass's constructor sets `params`, then calls, between its own
    checks, `_layout`, `_rows`, `_host_arrays`, `_allocate` and `_init`; it supplies `_fields()` for `read()`."""
    FAMILY = ""      # "dyn": the entry points m3g_dyn_state_bytes, _state_view, _init, _step and _read
    OBS = 0          # columns of an `obs` row
    CELLS = False    # the step takes the lattice and its fp32 copy
    SECOND = None    # the step's float32 input after the forces: (name, shape of a structure's row, ValueError text if it is required)

    def _entry(self, name: str):
        return getattr(self.lib, f"m3g_{self.FAMILY}_{name}")

    def _layout(self, pos: torch.Tensor, lattice: torch.Tensor | None, offsets) -> None:
        """offsets, N, S of the batch over the caller's `pos` / `lattice` (moved in place), and `lattice32`, the fp32 copy of the cells."""
        self.offsets, self.N, self.S = batch_layout(pos, lattice, offsets)
        self.pos, self.lattice = pos, lattice
        self.lattice32 = lattice.to(torch.float32) if lattice is not None else None
        self.device = pos.device

    def _rows(self, name: str, x: torch.Tensor) -> None:
        if x.dtype != torch.float64 or tuple(x.shape) != (self.N, 3) or x.device != self.pos.device:
            raise ValueError(f"{name} must be a [{self.N}, 3] float64 tensor on {self.pos.device}")

    def _host_arrays(self, masses, temperatures, seeds=None, units: int | None = None) -> bool:
        """`masses` [N], `temperatures` and (where the family draws) `seeds`, one per unit (structure; `units`: ring), as contiguous
        host arrays; whether the masses and seeds have those lengths."""
        units = self.S if units is None else units
        self.masses = np.ascontiguousarray(np.asarray(masses, dtype=np.float64).reshape(-1))
        self.temperatures = np.ascontiguousarray(np.broadcast_to(np.asarray(temperatures, dtype=np.float64), (units,)))
        if seeds is not None:
            self.seeds = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64).reshape(-1))
        return len(self.masses) == self.N and (seeds is None or len(self.seeds) == units)

    def _allocate(self, state_tensor, *sizes, units: int | None = None) -> None:
        """The state tensor of the family's `state_bytes(*sizes)` from `state_tensor` (the name the subclass's module imported: every
        driver module allocates through its own), the NaN `obs` [units, OBS] and `velocities`, the live [N,3] fp64 view of the
        integrator's own velocities inside the state (the family's `state_view`)."""
        self.sizes = sizes
        self.lib = _lib.load_library()
        self.state = state_tensor(self._entry("state_bytes"), *sizes, device=self.device)
        self.obs = torch.full((self.S if units is None else units, self.OBS), float("nan"), dtype=torch.float64, device=self.device)
        # what every step call passes unchanged: the entry point, and pointers to what is this object's own (not the caller's tensors)
        self._step, self._step_head = self._entry("step"), (C.byref(self.params), self.N, self.S, _ptr(self.state), self.state.numel())
        self._own = (_ptr(self.lattice32), _ptr(self.obs))
        mass_at, vel_at = C.c_size_t(), C.c_size_t()
        _lib.check(self._entry("state_view")(*sizes, C.byref(mass_at), C.byref(vel_at)))
        self.velocities = self.state[vel_at.value:vel_at.value + 24 * self.N].view(torch.float64).view(self.N, 3)

    def _init(self, *arrays) -> None:
        """The family's init: (params, N, S, offsets, masses, *arrays, state, bytes, stream); host arrays and device tensors (copied)."""
        held = [a if isinstance(a, np.ndarray) else a.contiguous() for a in arrays]
        with _cuda.on_device(self.device):
            _lib.check(self._entry("init")(C.byref(self.params), self.N, self.S, self.offsets.ctypes.data, self.masses.ctypes.data,
                                           *(a.ctypes.data if isinstance(a, np.ndarray) else _ptr(a) for a in held), _ptr(self.state),
                                           self.state.numel(), _stream()))

    def read(self) -> dict:
        """The arrays `_fields()` lists, copied to the host by the family's read (waits for the stream)."""
        return read_state(self._entry("read"), self.sizes, self.state, self._fields())

    def step(self, forces: torch.Tensor, finish_only: bool, second: torch.Tensor | None = None) -> None:
        """The family's step at `forces` [N,3] float32 and, where the family has SECOND = (name, row shape, needed), at `second`
        [S, *row shape] float32: None goes on as a null pointer unless `needed`, the ValueError text for a missing one, is set."""
        check_tensor("forces", forces, (self.N, 3), torch.float32)
        inputs = (_ptr(forces),)
        if self.SECOND is not None:
            name, row, needed = self.SECOND
            if second is not None:
                check_tensor(name, second, (self.S,) + row, torch.float32)
            elif needed:
                raise ValueError(needed)
            inputs = (_ptr(forces), _ptr(second))
        lattice32, obs = self._own
        cells = (_ptr(self.lattice), lattice32) if self.CELLS else ()
        with _cuda.on_device(self.device):
            _lib.check(self._step(*self._step_head, *inputs, _ptr(self.pos), *cells, 1 if finish_only else 0, obs, _stream()))


def sub_batches(n_copies: int, n: int, max_atoms: int):
    """(first_copy, count) of the engine sub-batches of `n_copies` copies of one structure of `n` atoms: in order, at most `max_atoms`
    atoms each (at least one copy).  The engine's rounding depends on the composition of its batch, so a structure's sub-batches hold
    its own copies only -- and its results are the same alone or in any batch."""
    per = max(1, max_atoms // n)
    for first in range(0, n_copies, per):
        yield first, min(per, n_copies - first)


class Driver:
    """The model handling of every driver.  `model`: the `Gradient` returned by `build_model`; the driver evaluates a
    `pair_virial=True` engine of its own made from its `Sequential`, at the precision of the caller's engine."""

    def __init__(self, model: Gradient, skin: float = 0.5, device="cuda"):
        if not isinstance(model, Gradient):
            raise TypeError(f"{type(self).__name__} needs the Gradient model returned by build_model")
        self.skin = positive("skin", skin)
        self.model = Gradient(model.model, pair_virial=True, legendre_backward=model.legendre_backward)
        if model._engine is not None:
            self.model.engine.set_precision(model._engine.precision)
        self.device = torch.device(device)


class GroupedEvaluation:
    """The engine evaluation of a batch cut into groups of consecutive structures, one `VerletGraph` (one engine batch) per group: the
    engine's fp32 rounding depends on the composition of its batch, so a structure's numbers are bitwise the same alone or beside
    others only when its group holds nothing else.  `groups`: (first, last) structure spans that cover the batch in order."""

    def __init__(self, model: Gradient, lat: list, z: list, groups: list, skin: float, device):
        cfg = model.engine.cfg
        self.model, self.spans = model, groups
        self.graphs = [VerletGraph(lat[lo:hi], z[lo:hi], cfg.cutoff, cfg.threebody_cutoff, skin=skin, device=device) for lo, hi in groups]
        self.device = self.graphs[0].device
        self.offsets = atom_offsets(z)
        self.N, self.S = int(self.offsets[-1]), len(z)
        self.rows = [(int(self.offsets[lo]), int(self.offsets[hi])) for lo, hi in groups]

    def lattices(self) -> torch.Tensor:
        """[S,3,3] fp64, a copy of the graphs' cells."""
        return (torch.cat([vg.lattice for vg in self.graphs]) if len(self.graphs) > 1 else self.graphs[0].lattice).clone()

    def buffers(self, forces: bool = True) -> dict:
        """Whole-batch float32 tensors for `evaluate(into=...)`; without `forces` the energies only (forces and stresses None)."""
        f32 = dict(dtype=torch.float32, device=self.device)
        return {K.TOTAL_ENERGY: torch.empty(self.S, **f32), K.FORCES: torch.empty(self.N, 3, **f32) if forces else None,
                K.STRESSES: torch.empty(self.S, 6, **f32) if forces else None}

    def evaluate(self, pos: torch.Tensor, into: dict | None = None, forces: bool = True) -> dict:
        """Energies (and, with `forces`, forces and stresses) of the whole batch at `pos` [N,3]: every group's `VerletGraph.step` --
        each waits for its skin test, as in `MolecularDynamics.run`: the only waits -- copied into the tensors of `into`, which is
        returned.  `into` None (one group only): that group's own output tensors."""
        if into is None:
            (vg,) = self.graphs
            return vg.step(self.model, pos, forces=forces)
        for vg, (a, b), (lo, hi) in zip(self.graphs, self.rows, self.spans):
            part = vg.step(self.model, pos[a:b], forces=forces)
            into[K.TOTAL_ENERGY][lo:hi].copy_(part[K.TOTAL_ENERGY])
            if forces:
                into[K.FORCES][a:b].copy_(part[K.FORCES])
                into[K.STRESSES][lo:hi].copy_(part[K.STRESSES])
        return into

    def raise_on_step_errors(self, what: str) -> None:
        for vg in self.graphs:
            vg.raise_on_step_errors(what)


class MdBatch(GroupedEvaluation):
    """The batch of an MD run (one group covering everything is the bare `VerletGraph`): beside the groups' graphs `pos` [N,3] fp64
    from the host positions and, with `cells`, `lattice` [S,3,3] fp64 -- the tensors an integrator state moves in place --, `atoms`,
    the (a, b) rows of every structure, and `whole`, the buffers of `evaluate` (one group: None, the engine's own tensors serve)."""

    def __init__(self, model: Gradient, lat: list, pos: list, z: list, groups: list, skin: float, device, cells: bool = True,
                 whole: bool = True):
        super().__init__(model, lat, z, groups, skin, device)
        self.atoms = [(int(a), int(b)) for a, b in zip(self.offsets, self.offsets[1:])]
        self.pos = torch.tensor(np.concatenate(pos), dtype=torch.float64, device=self.device)
        self.lattice = self.lattices() if cells else None
        self.whole = self.buffers() if whole and len(groups) > 1 else None


def md_loop(batch: MdBatch, state, steps: int, second=K.STRESSES, *, log=None, loginterval: int = 1, first_logged: int = 0,
            before=None, sync_at=None, at_sync=None, after=None, into: dict | None = None) -> dict:
    """`steps` steps of `state` (an `IntegratorState`) over `batch`: steps + 1 evaluations (into `into`, default `batch.whole`; each
    waits for its skin test, the only waits), each followed by `state.step(forces, finish_only, out[second])`, which finishes the
    step that ends there and, but at the last, starts the next.  Returns the last evaluation.  `before(k, out, logged)` runs between
    the two (samplers, reads, the clone of a cell about to move) and may return forces to integrate in place of the engine's.  Where
    `sync_at(k)` holds the step is finished, `at_sync(k, out)` acts on the synchronous velocities, the next step is started from
    the same forces without a second finish kick (not after the last), and what `at_sync` returned, if anything, is called.
    `log(j, out)` follows the integrator call for j = k - `first_logged` >= 0 at every multiple of `loginterval` and at the last step
    (host copies happen there only); `after(k, out)` closes the step."""
    into = batch.whole if into is None else into
    out = None
    for k in range(steps + 1):
        out = batch.evaluate(batch.pos, into)
        j = k - first_logged
        logged = log is not None and j >= 0 and (j % loginterval == 0 or k == steps)
        forces = before(k, out, logged) if before is not None else None
        forces, extra = out[K.FORCES] if forces is None else forces, None if second is None else out[second]
        if sync_at is not None and sync_at(k):
            state.step(forces, True, extra)        # synchronous velocities, STARTED cleared
            resumed = at_sync(k, out)
            if k < steps:
                state.step(forces, False, extra)   # starts the next step: no second finish kick
            if resumed is not None:
                resumed()
        else:
            state.step(forces, k == steps, extra)
        if logged:
            log(j, out)
        if after is not None:
            after(k, out)
    return out


class MdLog:
    """The log of an MD run: step, e_pot, ke (eV), t (K), p (GPa), v (A^3) of every structure at the steps `append` is called; with
    `conserved` (the ensembles of `NhcState`, whose obs rows hold the extended energy in column 4) also conserved = e_pot + ke +
    extended (eV); with `cell` (the ensemble of `MtkCellState`, whose obs rows hold the pressure tensor in columns 6 .. 11) also
    pressure_tensor [6] (GPa, Voigt order xx, yy, zz, yz, zx, xy) and lattice [3,3] (A)."""

    def __init__(self, conserved: bool = False, cell: bool = False):
        self.rows = {key: [] for key in ("step", "e_pot", "ke", "t", "p", "v") + (("conserved",) if conserved else ())
                     + (("pressure_tensor", "lattice") if cell else ())}

    def append(self, k: int, energies: torch.Tensor, obs: torch.Tensor, lattice: torch.Tensor | None = None) -> None:
        """Step `k` at `energies` [S] and `DynState.obs` [S,4] / `NhcState.obs` [S,6] / `MtkCellState.obs` [S,12] (copies both to the
        host: waits), with `cell` also at the cells `lattice` [S,3,3] the observables were taken in."""
        obs = obs.cpu().numpy()
        if "lattice" in self.rows:
            self.rows["pressure_tensor"].append(obs[:, 6:12] * EV_A3_TO_GPA)
            self.rows["lattice"].append(lattice.cpu().numpy())
        self.rows["step"].append(np.full(len(obs), k))
        self.rows["e_pot"].append(energies.double().cpu().numpy())
        for j, key in enumerate(("ke", "t", "p", "v")):
            self.rows[key].append(obs[:, j] * (EV_A3_TO_GPA if key == "p" else 1.0))
        if "conserved" in self.rows:
            self.rows["conserved"].append(self.rows["e_pot"][-1] + obs[:, 0] + obs[:, 4])

    def of(self, state):
        """The `log` of `md_loop` that appends `state.obs` beside the energies."""
        return lambda j, out: self.append(j, out[K.TOTAL_ENERGY], state.obs)

    def arrays(self) -> dict:
        return {key: np.stack(val, axis=1) for key, val in self.rows.items()}   # [S, n_log]


def md_results(batch: MdBatch, dyn, out: dict, log: MdLog, what: str) -> list:
    """The tail of an MD run: the graphs' status (raises for `what`), `dyn.read()` (waits), the last evaluation `out`, the positions
    and the cells copied to the host, and the dict `MolecularDynamics.run` returns for every structure."""
    batch.raise_on_step_errors(what)
    st = dyn.read()
    e, f, sv = (out[key].double().cpu().numpy() for key in (K.TOTAL_ENERGY, K.FORCES, K.STRESSES))
    p_host, l_host, logs = batch.pos.cpu().numpy(), batch.lattice.cpu().numpy(), log.arrays()
    return [{"positions": p_host[a:b].copy(), "velocities": st["v"][a:b].copy(), "lattice": l_host[s].copy(),
             "total_energy": float(e[s]), "forces": f[a:b].copy(), "stresses": sv[s].copy(), "n_steps": int(st["n_steps"][s]),
             "error": bool(st["flags"][s] & _lib.DYN_ERROR), "log": {key: val[s].copy() for key, val in logs.items()}}
            for s, (a, b) in enumerate(batch.atoms)]
