"""Batched collective-variable biasing on the device (C ABI: m3g_meta_*, csrc/m3g_meta.hip) over the Langevin integrator of
`dynamics`: multiple-walker metadynamics (Laio, Parrinello, PNAS 99, 12562 (2002)), well-tempered (Barducci, Bussi, Parrinello, PRL
100, 020603 (2008)) or plain, and umbrella sampling (Torrie, Valleau, J. Comput. Phys. 23, 187 (1977)) with WHAM (Kumar et al.,
J. Comput. Chem. 13, 1011 (1992)) -- what PLUMED calls METAD, RESTRAINT, LOWER_WALLS / UPPER_WALLS.  Multiple-walker metadynamics
is a batch of copies that share one hill list; an umbrella-sampling run is a batch of windows.  The bias is three kernel launches on
the stream of the run (`bias_forces`): the host never sees a position, the Verlet lists stay valid, and the biased forces go to
`dyn_step` unchanged.

Limits: the cells are fixed (NVE / NVT only); at most two collective variables (CVs); "coordination" costs O(|A| |B|) per step; the
centres of "distance" and "projection" are taken over the unwrapped positions without the minimum image; and the model's energy
steps where a pair crosses the two-body cutoff, so a CV that drags a pair through the cutoff carries that step into
the free energy it reports.

Units as in `dynamics`: A, fs, amu, eV, K."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Sequence

import numpy as np
import torch

from . import _cuda, _lib
from ._driver import (Driver, MdBatch, MdLog, check_tensor, derived_keys, integer, md_loop, md_results, non_negative, positive, read_state,
                      replicated, state_tensor, structure_arrays, structure_masses)
from .data import MaterialGraphKey as K
from .data.graph_gpu import _ptr, _stream
from .dynamics import KB, DynState, maxwell_boltzmann
from .nn.modules import Gradient

KINDS = {"distance": _lib.CV_DISTANCE, "projection": _lib.CV_PROJECTION, "coordination": _lib.CV_COORDINATION}
MAX_POWER = 6


@dataclass(frozen=True)
class CollectiveVariable:
    """A checked CV description over atom indices of one structure (`distance`, `projection`, `coordination` make them)."""
    kind: str
    a: tuple
    b: tuple
    direction: tuple | None = None
    origin: tuple | None = None
    r0: float = 1.0
    p: int = 1
    r_cut: float = 1.0


def _indices(name: str, x, empty_ok: bool = False) -> tuple:
    idx = np.asarray(x if x is not None else [], dtype=object).reshape(-1)
    if any(isinstance(i, (bool, np.bool_)) or not isinstance(i, (int, np.integer)) or i < 0 for i in idx):
        raise ValueError(f"{name} must hold atom indices >= 0; got {x!r}")
    idx = tuple(int(i) for i in idx)
    if len(set(idx)) != len(idx):
        raise ValueError(f"{name} holds an atom twice")
    if not idx and not empty_ok:
        raise ValueError(f"{name} must hold at least one atom")
    return idx


def distance(a, b) -> CollectiveVariable:
    """|c_A - c_B|: the distance between the mass-weighted centres of the atoms `a` and `b` (unwrapped positions, no minimum image:
    keep the two groups in one periodic image).  At distance 0 the gradient is zero."""
    return CollectiveVariable("distance", _indices("a", a), _indices("b", b))


def projection(a, b, direction, origin=None) -> CollectiveVariable:
    """(c_A - c_B - origin) . n: the displacement of the centre of `a` relative to that of `b` (empty: relative to the coordinate
    origin) along `direction` (normalised here).  `origin` [3]: default, c_A - c_B of every structure's starting positions, so the
    CV starts at 0.  The hop coordinate of a diffusing atom relative to the rest of the crystal: Langevin dynamics does not hold the
    centre of mass, hence the relative form."""
    n = np.asarray(direction, dtype=np.float64).reshape(-1)
    if n.shape != (3,) or not np.isfinite(n).all() or not np.linalg.norm(n) > 0.0:
        raise ValueError(f"direction must be a finite, non-zero 3-vector; got {direction!r}")
    n = n / np.linalg.norm(n)
    if origin is not None:
        origin = np.asarray(origin, dtype=np.float64).reshape(-1)
        if origin.shape != (3,) or not np.isfinite(origin).all():
            raise ValueError(f"origin must be a finite 3-vector; got {origin!r}")
        origin = tuple(origin)
    return CollectiveVariable("projection", _indices("a", a), _indices("b", b, empty_ok=True), direction=tuple(n), origin=origin)


def coordination(a, b, r0: float, p: int = 3, r_cut: float | None = None) -> CollectiveVariable:
    """sum_{i in a} sum_{j in b, j != i} f(r_ij) with sigma(r) = 1 / (1 + (r / r0)^(2 p)), p = 1 .. 6, and f = (sigma(r) -
    sigma(r_cut)) / (1 - sigma(r_cut)) below `r_cut` (default 2.5 r0), 0 beyond: continuous at the cutoff.  Minimum image of the
    fixed cell; r_cut must not exceed half the smallest perpendicular width of any cell.  O(|a| |b|) per step."""
    r0 = positive("r0", r0)
    if isinstance(p, bool) or not isinstance(p, (int, np.integer)) or not 1 <= p <= MAX_POWER:
        raise ValueError(f"p must be an integer in 1 .. {MAX_POWER}; got {p!r}")
    r_cut = positive("r_cut", 2.5 * r0 if r_cut is None else r_cut)
    return CollectiveVariable("coordination", _indices("a", a), _indices("b", b), r0=r0, p=int(p), r_cut=r_cut)


def _cv_list(cvs) -> list:
    cvs = [cvs] if isinstance(cvs, CollectiveVariable) else list(cvs)
    if not 1 <= len(cvs) <= _lib.META_MAX_CV or not all(isinstance(cv, CollectiveVariable) for cv in cvs):
        raise ValueError(f"cvs must be 1 .. {_lib.META_MAX_CV} collective variables made by distance / projection / coordination")
    return cvs


def _per(name: str, x, shape: tuple, default: float = 0.0) -> np.ndarray:
    """`x` (None: `default`) broadcast to `shape`, fp64, contiguous."""
    x = np.asarray(default if x is None else x, dtype=np.float64)
    try:
        return np.ascontiguousarray(np.broadcast_to(x, shape))
    except ValueError:
        raise ValueError(f"{name}: expected a value that broadcasts to {shape}; got shape {x.shape}") from None


class BiasState:
    """The bias state of a batch on the device (m3g_meta_init).  `offsets`: S + 1 atom offsets; `group_offsets`: G + 1 structure
    offsets of the walker groups (the walkers of a group share one hill list; default: every structure its own group); `lattices`
    [S,3,3] (fixed); `cvs`: 1 .. 2 CVs, their atom indices relative to every structure; `weights` [N] (the masses); `sigma` [n_cv]
    or [G,n_cv], `height` and `inv_kdt` (1 / (kB DeltaT); 0: plain metadynamics) one value or [G]; `max_hills` per group;
    `centres` / `kappa`: the harmonic restraint kappa / 2 (s - centre)^2, [n_cv] or [S,n_cv] (kappa 0: off); `walls`: [n_cv,4] or
    [S,n_cv,4] = (lower, kappa_lower, upper, kappa_upper); `origins`: [S,n_cv,3] for "projection" CVs without an origin of their
    own; `membership` [n_cv, N] uint8 (0 none, 1 A, 2 B, 3 both) replaces the CVs' index lists, for structures whose groups
    differ.  `obs` [S,8] (s_0, s_1, V, V_hills, V_restraint + walls, dV/ds_0, dV/ds_1, height deposited) and `forces_out` [N,3]
    float32 are written by every `bias_forces`."""

    def __init__(self, offsets: Sequence[int], lattices, cvs, weights, sigma, height=0.0, inv_kdt=0.0, max_hills: int = 0,
                 group_offsets: Sequence[int] | None = None, centres=None, kappa=None, walls=None, origins=None, membership=None,
                 device="cuda"):
        self.cvs = _cv_list(cvs)
        n_cv = self.n_cv = len(self.cvs)
        self.offsets = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64).reshape(-1))
        self.S = len(self.offsets) - 1
        if self.S < 1:
            raise ValueError("offsets must hold S + 1 >= 2 entries")
        self.N = int(self.offsets[-1])
        self.group_offsets = np.ascontiguousarray(np.asarray(np.arange(self.S + 1) if group_offsets is None else group_offsets,
                                                             dtype=np.int64).reshape(-1))
        self.G = len(self.group_offsets) - 1
        if self.G < 1:
            raise ValueError("group_offsets must hold G + 1 >= 2 entries")
        self.max_hills = integer("max_hills", max_hills, 0)
        self.lattices = np.ascontiguousarray(np.asarray(lattices, dtype=np.float64))
        if self.lattices.shape != (self.S, 3, 3):
            raise ValueError(f"lattices must be [{self.S}, 3, 3]; got {self.lattices.shape}")
        self.weights = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).reshape(-1))
        if len(self.weights) != self.N:
            raise ValueError(f"weights: expected {self.N} entries; got {len(self.weights)}")
        self.params = _lib.M3GMetaParams(n_cv=n_cv, reserved=0, max_hills=self.max_hills)
        self.membership = np.zeros((n_cv, self.N), dtype=np.uint8)
        sizes = np.diff(self.offsets)
        for k, cv in enumerate(self.cvs):
            self.params.kind[k] = KINDS[cv.kind]
            self.params.power[k], self.params.r0[k], self.params.r_cut[k] = cv.p, cv.r0, cv.r_cut
            for a in range(3):
                self.params.direction[k][a] = 0.0 if cv.direction is None else cv.direction[a]
            for side, idx in ((1, cv.a), (2, cv.b)):
                if idx and max(idx) >= sizes.min():
                    raise ValueError(f"CV {k}: atom index {max(idx)} is outside a structure of {sizes.min()} atoms")
                for s in range(self.S):
                    self.membership[k, self.offsets[s] + np.asarray(idx, dtype=np.int64)] |= side
        if membership is not None:   # per atom of the batch instead: structures whose groups differ
            self.membership = np.ascontiguousarray(np.asarray(membership, dtype=np.uint8))
            if self.membership.shape != (n_cv, self.N):
                raise ValueError(f"membership must be [{n_cv}, {self.N}]; got {self.membership.shape}")
        self.origins = _per("origins", origins, (self.S, n_cv, 3)).copy()
        for k, cv in enumerate(self.cvs):
            if cv.origin is not None:
                self.origins[:, k] = cv.origin
        self.centres, self.kappa = _per("centres", centres, (self.S, n_cv)), _per("kappa", kappa, (self.S, n_cv))
        self.walls = _per("walls", walls, (self.S, n_cv, 4))
        self.sigma, self.height = _per("sigma", sigma, (self.G, n_cv)), _per("height", height, (self.G,))
        self.inv_kdt = _per("inv_kdt", inv_kdt, (self.G,))
        self.device = torch.device(device)
        self.lib = _lib.load_library()
        sizes = (self.N, self.S, self.G, n_cv, self.max_hills)
        self.state = state_tensor(self.lib.m3g_meta_state_bytes, *sizes, device=self.device)
        at = C.c_size_t()
        _lib.check(self.lib.m3g_meta_state_view(*sizes, C.byref(at)))
        self.gradients = self.state[at.value:at.value + 24 * n_cv * self.N].view(torch.float64).view(n_cv, self.N, 3)
        self.obs = torch.full((self.S, _lib.META_OBS), float("nan"), dtype=torch.float64, device=self.device)
        self.forces_out = torch.zeros(self.N, 3, dtype=torch.float32, device=self.device)
        with _cuda.on_device(self.device):
            _lib.check(self.lib.m3g_meta_init(C.byref(self.params), self.N, self.S, self.G, self.offsets.ctypes.data,
                                              self.group_offsets.ctypes.data, self.lattices.ctypes.data, self.membership.ctypes.data,
                                              self.weights.ctypes.data, self.origins.ctypes.data, self.centres.ctypes.data,
                                              self.kappa.ctypes.data, self.walls.ctypes.data, self.sigma.ctypes.data, self.height.ctypes.data,
                                              self.inv_kdt.ctypes.data, _ptr(self.state), self.state.numel(), _stream()))

    def _sizes(self) -> tuple:
        return C.byref(self.params), self.N, self.S, self.G

    def set_hills(self, centres: Sequence, heights: Sequence) -> None:
        """Replace the hill lists (a restart): per group `centres` [n_g, n_cv] and `heights` [n_g], n_g a multiple of the group's
        walkers and at most `max_hills`.  Waits for the stream."""
        if len(centres) != self.G or len(heights) != self.G:
            raise ValueError(f"set_hills: expected one list per group ({self.G})")
        counts = np.zeros(self.G, dtype=np.int64)
        c_all, h_all = np.zeros((self.G, self.max_hills, self.n_cv)), np.zeros((self.G, self.max_hills))
        for g, (c, h) in enumerate(zip(centres, heights)):
            c, h = np.asarray(c, dtype=np.float64).reshape(-1, self.n_cv), np.asarray(h, dtype=np.float64).reshape(-1)
            if len(c) != len(h) or len(h) > self.max_hills:
                raise ValueError(f"set_hills: group {g} needs as many centres as heights, at most max_hills = {self.max_hills}")
            counts[g] = len(h)
            c_all[g, :len(h)], h_all[g, :len(h)] = c, h
        with _cuda.on_device(self.device):
            _lib.check(self.lib.m3g_meta_set_hills(*self._sizes(), _ptr(self.state), self.state.numel(), self.group_offsets.ctypes.data,
                                                   counts.ctypes.data, c_all.ctypes.data, h_all.ctypes.data, _stream()))

    def read(self) -> dict:
        """flags (int32 [S]: 1 = a non-finite CV was met, 2 = the hill list is full), deposits (int64 [S]), n_hills (int64 [G]),
        centres [G, max_hills, n_cv] and heights [G, max_hills], copied to the host (waits for the stream)."""
        return read_state(self.lib.m3g_meta_read, self._sizes(), self.state,
                          (("flags", np.int32, self.S), ("deposits", np.int64, self.S), ("n_hills", np.int64, self.G),
                           ("centres", np.float64, (self.G, self.max_hills, self.n_cv)), ("heights", np.float64, (self.G, self.max_hills))))


def bias_forces(state: BiasState, pos: torch.Tensor, forces: torch.Tensor, deposit: bool = False, out: torch.Tensor | None = None) -> torch.Tensor:
    """One bias call of every structure (m3g_meta_bias) at the unwrapped positions `pos` [N,3] fp64 and the engine's `forces` [N,3]
    float32: writes `state.obs` and the biased forces into `out` (default `state.forces_out`; may be `forces` itself), which is
    returned and goes to `dyn_step` unchanged.  `deposit`: every walker appends a hill at its CV (against the list as it stood
    before the call).  Three launches queued on the current stream; no wait, capture-safe."""
    check_tensor("pos", pos, (state.N, 3), torch.float64, state.obs.device)
    check_tensor("forces", forces, (state.N, 3), torch.float32, state.obs.device)
    out = state.forces_out if out is None else out
    check_tensor("out", out, (state.N, 3), torch.float32, state.obs.device)
    with _cuda.on_device(state.obs.device):
        _lib.check(state.lib.m3g_meta_bias(*state._sizes(), _ptr(state.state), state.state.numel(), _ptr(pos), _ptr(forces), _ptr(out),
                                           1 if deposit else 0, _ptr(state.obs), _stream()))
    return out


def hills_bias(grid, centres, heights, sigma) -> np.ndarray:
    """V_hills at the points `grid` ([m] for one CV, [m, n_cv]) of the hills `centres` [n, n_cv], `heights` [n], widths `sigma`."""
    sigma = np.asarray(sigma, dtype=np.float64).reshape(-1)
    grid = np.asarray(grid, dtype=np.float64).reshape(-1, len(sigma))
    centres, heights = np.asarray(centres, dtype=np.float64).reshape(-1, len(sigma)), np.asarray(heights, dtype=np.float64).reshape(-1)
    q = (((grid[:, None, :] - centres[None, :, :]) / sigma) ** 2).sum(-1)
    return (heights[None, :] * np.exp(-0.5 * q)).sum(1)


def free_energy_scale(temperature: float, bias_factor: float | None) -> float:
    """F = -scale V_hills: (T + DeltaT) / DeltaT = gamma / (gamma - 1) for well-tempered metadynamics, 1 for plain."""
    return 1.0 if bias_factor is None else bias_factor / (bias_factor - 1.0)


class Hills:
    """The hill list of one input: `centres` [n, n_cv], `heights` [n] (eV), `sigma` [n_cv]; `bias(grid)` is V_hills there and
    `free_energy(grid)` = -(T + DeltaT) / DeltaT V_hills (plain metadynamics: -V_hills), shifted to a minimum of zero."""

    def __init__(self, centres, heights, sigma, temperature: float, bias_factor: float | None):
        self.centres, self.heights, self.sigma = centres, heights, np.asarray(sigma, dtype=np.float64)
        self.temperature, self.bias_factor = temperature, bias_factor

    def bias(self, grid) -> np.ndarray:
        return hills_bias(grid, self.centres, self.heights, self.sigma)

    def free_energy(self, grid) -> np.ndarray:
        f = -free_energy_scale(self.temperature, self.bias_factor) * self.bias(grid)
        return f - f.min()


def walker_keys(seed, n_inputs: int, copies: int):
    """(velocity seeds, thermostat keys), each [n_inputs, copies]: a copy's keys derive from its input's own seed only (as
    `FreeEnergy` derives them), so an input's run does not depend on its neighbours.  `MolecularDynamics.run` of one structure with
    `velocities=[maxwell_boltzmann(m, T, velocity seed)]` and `seed=[thermostat key]` is the same unbiased trajectory."""
    keys = np.stack(derived_keys(seed, n_inputs, 2 * copies))
    return keys[:, 0::2].copy(), keys[:, 1::2].copy()


class _BiasedLangevin(Driver):
    """What `Metadynamics` and `UmbrellaSampling` share: `copies` copies of every input in one batch, one engine group per input,
    BAOAB Langevin through `DynState` / `dyn_step` with the forces `bias_forces` hands over."""

    def __init__(self, model: Gradient, cvs, temperature: float, timestep: float, friction: float, skin: float, seed, device):
        super().__init__(model, skin, device)
        self.cvs = _cv_list(cvs)
        self.temperature, self.timestep, self.friction = positive("temperature", temperature), positive("timestep", timestep), non_negative("friction", friction)
        self.seed = seed

    def _run(self, lattices, positions, atomic_numbers, masses, copies: int, steps: int, equilibration: int, pace: int, loginterval: int,
             bias_args) -> tuple:
        steps, equilibration = integer("steps", steps, 0), integer("equilibration", equilibration, 0)
        loginterval = integer("loginterval", loginterval, 1)
        lat, pos, z = structure_arrays(lattices, positions, atomic_numbers)
        m = structure_masses(masses, z)
        G = len(z)
        rep = lambda xs: replicated(xs, copies)   # noqa: E731
        ev = MdBatch(self.model, rep(lat), rep(pos), rep(z), [(g * copies, (g + 1) * copies) for g in range(G)], self.skin, self.device)
        dev, pos_t = ev.device, ev.pos
        v_seeds, t_keys = walker_keys(self.seed, G, copies)
        vel = [maxwell_boltzmann(m[g], self.temperature, int(v_seeds[g, r])) for g in range(G) for r in range(copies)]
        m_all = np.concatenate(rep(m))
        dyn = DynState(pos_t, ev.lattice, ev.offsets, m_all, torch.tensor(np.concatenate(vel), device=dev), self.temperature, t_keys.reshape(-1),
                       ensemble="nvt_langevin", dt=self.timestep, friction=self.friction)
        origins = np.zeros((ev.S, len(self.cvs), 3))   # "projection" without an origin: the CV starts at 0
        for s in range(ev.S):
            x, w = pos[s // copies], m[s // copies]
            for k, cv in enumerate(self.cvs):
                if cv.kind == "projection" and cv.origin is None:
                    centre = lambda idx: (w[list(idx), None] * x[list(idx)]).sum(0) / w[list(idx)].sum() if idx else np.zeros(3)   # noqa: E731
                    origins[s, k] = centre(cv.a) - centre(cv.b)
        bias = BiasState(ev.offsets, np.stack(rep(lat)), self.cvs, m_all, origins=origins, device=dev, **bias_args(G, ev.S))
        trace = torch.zeros(steps + 1, ev.S, _lib.META_OBS, dtype=torch.float64, device=dev)

        def biased(k, out, logged):
            j = k - equilibration
            forces = bias_forces(bias, pos_t, out[K.FORCES], deposit=(pace > 0 and j > 0 and j % pace == 0))
            if j >= 0:
                trace[j].copy_(bias.obs)
            return forces

        log = MdLog()
        out = md_loop(ev, dyn, equilibration + steps, before=biased, log=log.of(dyn), loginterval=loginterval, first_logged=equilibration)
        runs = md_results(ev, dyn, out, log, type(self).__name__)
        return runs, trace.cpu().numpy().transpose(1, 0, 2), bias.read(), bias


class Metadynamics(_BiasedLangevin):
    """Multiple-walker metadynamics of a batch of structures along 1 .. 2 CVs.

    `model`: the `Gradient` returned by `build_model`; `cvs`: made by `distance`, `projection`, `coordination`; `temperature` (K);
    `height` (eV) and `sigma` ([n_cv], in the CVs' units) of the Gaussians, one deposited by every walker every `pace` steps;
    `bias_factor` gamma = (T + DeltaT) / T > 1: well-tempered (the heights decay as exp(-V_hills / kB DeltaT)), None: plain;
    `walkers`: copies of every input that share its hill list; `walls`: [n_cv, 4] = (lower, kappa_lower, upper, kappa_upper) in
    the CVs' units and eV per unit^2, kappa 0 = off; BAOAB Langevin with `timestep` (fs) and `friction` (1/fs).  See the module's
    limits: fixed cells, at most two CVs, O(|A| |B|) coordination, the model's cutoff step."""

    def __init__(self, model: Gradient, cvs, temperature: float, height: float, sigma, pace: int, bias_factor: float | None = None,
                 walkers: int = 1, walls=None, timestep: float = 1.0, friction: float = 0.01, skin: float = 0.5, seed=0, device="cuda"):
        super().__init__(model, cvs, temperature, timestep, friction, skin, seed, device)
        self.height = non_negative("height", height)
        self.sigma = np.asarray(sigma, dtype=np.float64).reshape(-1)
        if self.sigma.shape != (len(self.cvs),) or not (np.isfinite(self.sigma).all() and (self.sigma > 0).all()):
            raise ValueError(f"sigma must hold one finite value > 0 per CV ({len(self.cvs)}); got {sigma!r}")
        self.pace, self.walkers = integer("pace", pace, 1), integer("walkers", walkers, 1)
        if bias_factor is not None and not (math.isfinite(float(bias_factor)) and float(bias_factor) > 1.0):
            raise ValueError(f"bias_factor must be a finite number > 1 (or None: plain metadynamics); got {bias_factor!r}")
        self.bias_factor = None if bias_factor is None else float(bias_factor)
        self.walls = None if walls is None else _per("walls", walls, (len(self.cvs), 4))

    def run(self, lattices: Sequence, positions: Sequence, atomic_numbers: Sequence, steps: int, equilibration: int = 0,
            masses: Sequence | None = None, loginterval: int = 10) -> list:
        """`equilibration` steps without deposits (the walls act), then `steps` steps with a deposit at every `pace`-th.  Every input
        becomes `walkers` copies with keys of their own (`walker_keys`) and one engine batch of its own, so its numbers do not depend
        on its neighbours.  Returns one dict per input: `walkers` (the dict of `MolecularDynamics.run` for every walker), `cv`
        [walkers, steps + 1, n_cv], `bias_energy` [walkers, steps + 1] (eV: the bias every walker felt), `hills` (a `Hills`),
        `bias` and `free_energy` (its methods: functions of a grid), `n_hills`, `full` (the list filled up: never, as it is sized
        steps // pace * walkers) and `error` (a walker met a non-finite CV)."""
        R = self.walkers
        inv_kdt = 0.0 if self.bias_factor is None else 1.0 / (KB * (self.bias_factor - 1.0) * self.temperature)
        max_hills = integer("steps", steps, 0) // self.pace * R
        args = lambda G, S: dict(sigma=self.sigma, height=self.height, inv_kdt=inv_kdt, max_hills=max_hills, walls=self.walls,   # noqa: E731
                                 group_offsets=np.arange(G + 1) * R)
        runs, trace, bs, _ = self._run(lattices, positions, atomic_numbers, masses, R, steps, equilibration, self.pace, loginterval, args)
        n_cv, res = len(self.cvs), []
        for g in range(len(runs) // R):
            n = int(bs["n_hills"][g])
            hills = Hills(bs["centres"][g, :n].copy(), bs["heights"][g, :n].copy(), self.sigma, self.temperature, self.bias_factor)
            rows = slice(g * R, (g + 1) * R)
            res.append({"walkers": runs[rows], "cv": trace[rows, :, :n_cv].copy(), "bias_energy": trace[rows, :, 2].copy(), "hills": hills,
                        "bias": hills.bias, "free_energy": hills.free_energy, "n_hills": n,
                        "full": bool((bs["flags"][rows] & _lib.META_FULL).any()), "error": bool((bs["flags"][rows] & _lib.META_ERROR).any())})
        return res


class UmbrellaSampling(_BiasedLangevin):
    """Umbrella sampling of a batch of structures along one CV: every input times every window is one structure of the batch, under
    the static restraint kappa_w / 2 (s - centre_w)^2 (`centres` and `kappa`: one per window; kappa in eV per squared CV unit) and
    no hills.  The other arguments as `Metadynamics`; `wham` turns the samples into a free energy."""

    def __init__(self, model: Gradient, cv, centres, kappa, temperature: float, timestep: float = 1.0, friction: float = 0.01,
                 skin: float = 0.5, seed=0, device="cuda"):
        super().__init__(model, cv, temperature, timestep, friction, skin, seed, device)
        if len(self.cvs) != 1:
            raise ValueError("UmbrellaSampling takes one CV")
        self.centres = np.asarray(centres, dtype=np.float64).reshape(-1)
        if len(self.centres) < 1 or not np.isfinite(self.centres).all():
            raise ValueError("centres must hold one finite value per window (at least one)")
        self.kappa = _per("kappa", kappa, self.centres.shape)
        if not (np.isfinite(self.kappa).all() and (self.kappa >= 0).all()):
            raise ValueError("kappa must be finite and >= 0")

    def run(self, lattices: Sequence, positions: Sequence, atomic_numbers: Sequence, steps: int, equilibration: int = 0,
            masses: Sequence | None = None, loginterval: int = 10) -> list:
        """`equilibration` steps, then `steps` sampled steps, of every window of every input.  Returns one dict per input: `windows`
        (the dict of `MolecularDynamics.run` per window), `samples` [n_windows, steps + 1] (the CV), `bias_energy` (the same shape,
        eV), `centres`, `kappa` and `error`."""
        W = len(self.centres)
        args = lambda G, S: dict(sigma=1.0, centres=np.tile(self.centres, G)[:, None], kappa=np.tile(self.kappa, G)[:, None])   # noqa: E731
        runs, trace, bs, _ = self._run(lattices, positions, atomic_numbers, masses, W, steps, equilibration, 0, loginterval, args)
        return [{"windows": runs[g * W:(g + 1) * W], "samples": trace[g * W:(g + 1) * W, :, 0].copy(),
                 "bias_energy": trace[g * W:(g + 1) * W, :, 2].copy(), "centres": self.centres.copy(), "kappa": self.kappa.copy(),
                 "error": bool((bs["flags"][g * W:(g + 1) * W] & _lib.META_ERROR).any())} for g in range(len(runs) // W)]


def wham(samples: Sequence, centres, kappas, temperature: float, bins, tolerance: float = 1e-10, max_iterations: int = 100000) -> dict:
    """The weighted-histogram analysis of 1-D umbrella windows on the host: `samples` (one array of CV values per window) under the
    restraints kappas_w / 2 (s - centres_w)^2 at `temperature` (K); `bins`: a number of equal bins over the range of the samples, or
    the bin edges.  Self-consistent iteration of p(s_b) = sum_w n_w(b) / sum_w N_w exp(-(u_w(s_b) - f_w) / kB T), exp(-f_w / kB T) =
    sum_b p(s_b) exp(-u_w(s_b) / kB T), until no f_w moves by more than `tolerance` (eV).  Returns `s` (bin centres), `free_energy`
    (eV, -kB T ln p, minimum 0, inf in empty bins), `probability` (normalised over the bins), `offsets` (f_w, f_0 = 0) and
    `iterations`."""
    centres, kappas = np.asarray(centres, dtype=np.float64).reshape(-1), np.asarray(kappas, dtype=np.float64).reshape(-1)
    samples = [np.asarray(x, dtype=np.float64).reshape(-1) for x in samples]
    if not (len(samples) == len(centres) == len(kappas)) or not samples or any(len(x) == 0 or not np.isfinite(x).all() for x in samples):
        raise ValueError("wham: one non-empty finite sample array, centre and kappa per window")
    if not (np.isfinite(centres).all() and np.isfinite(kappas).all() and (kappas >= 0).all()):
        raise ValueError("wham: centres must be finite and kappas finite and >= 0")
    kt = KB * positive("temperature", temperature)
    if np.ndim(bins) == 0:
        lo, hi = min(x.min() for x in samples), max(x.max() for x in samples)
        edges = np.linspace(lo, hi, integer("bins", bins, 1) + 1)
    else:
        edges = np.asarray(bins, dtype=np.float64).reshape(-1)
        if len(edges) < 2 or not (np.diff(edges) > 0).all():
            raise ValueError("wham: bin edges must increase strictly")
    s = 0.5 * (edges[1:] + edges[:-1])
    hist = np.stack([np.histogram(x, edges)[0] for x in samples]).astype(np.float64)    # [W, B]
    counts = hist.sum(1)
    if not (counts > 0).all():
        raise ValueError("wham: a window has no sample inside the bins")
    u = 0.5 * kappas[:, None] * (s[None, :] - centres[:, None]) ** 2 / kt                 # [W, B]
    f = np.zeros(len(samples))
    top = hist.sum(0)
    for it in range(1, max_iterations + 1):
        p = top / (counts[:, None] * np.exp(f[:, None] - u)).sum(0)
        f_new = -np.log((p[None, :] * np.exp(-u)).sum(1))
        f_new -= f_new[0]
        moved = np.abs(f_new - f).max()
        f = f_new
        if moved * kt <= tolerance:
            break
    p = top / (counts[:, None] * np.exp(f[:, None] - u)).sum(0)
    p = p / p.sum()
    with np.errstate(divide="ignore"):
        free = -kt * np.log(p)
    return {"s": s, "free_energy": free - free[np.isfinite(free)].min(), "probability": p, "offsets": f * kt, "iterations": it}
