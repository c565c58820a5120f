"""Scattering observables accumulated on the device: static structure factor S(q), intermediate scattering function F(q,t), dynamic
structure factor S(q,w) and the longitudinal / transverse current correlations of every structure of a batch (C ABI: m3g_sq_*,
csrc/m3g_scattering.hip).  The reciprocal-space companion of `trajectory.py`.

`MolecularDynamics.run(..., observables=ScatteringObservables(...))` (alone, or in a list beside a `TrajectoryObservables`) samples the
trajectory on the device while it integrates -- no frame ever goes to the host -- and every result dict gains "scattering".
`SqState` / `sq_sample` are the layer below (they mirror `TrajState` / `traj_sample`) and take any frames.

Conventions (the same ones are restated in tests/scattering_reference.py).  Structure s has its own integer Miller triples h != 0; with
L the CURRENT cell (rows = lattice vectors) q = 2 pi h L^-T, so q . r = 2 pi h . (r L^-1): every h is commensurate with every cell.
Per species a:
    rho_a(q) = sum_{j in a} exp(-i q . r_j)      j_a(q) = sum_{j in a} v_j exp(-i q . r_j)      j_L = qhat . j      j_T = j - qhat j_L
(with remove_com, r and v relative to the structure's mass-weighted centre of mass: a diffusing centre of mass would multiply F(q,t)
by a spurious phase).  The device keeps, per q, species pair a <= b and lag l, the sums over the samples that have a frame l samples
back (lag_count[l] of them) of
    F_ab  : Re[rho_a(t) rho_b*(t-l) + rho_b(t) rho_a*(t-l)] / 2
    CL_ab : the same of j_L
    CT_ab : half the same of j_T . j_T*            (the mean over the two transverse directions)
and the results are, with N the atoms of the structure, c_a = N_a / N and time = l * sample_interval * timestep (fs):
    f[a][b][q, l]   = F_ab / (lag_count[l] N)       c_l, c_t likewise (A^2/fs^2)       s = f_total at lag 0
    f_total         = sum over ORDERED pairs (a, b) = sum_a f[a][a] + 2 sum_{a<b} f[a][b]
    with weights b  : f_total = sum_ab b_a b_b f[a][b] / sum_a c_a b_a^2                (c_l_total, c_t_total alike)
    *_shell         : the mean of the totals over the q-vectors whose |q| (starting cell) falls in a bin of width shell_width
    s_qw, c_l_qw, c_t_qw [shell, k] = 2 int_0^T C(t) w(t) cos(2 pi f_k t) dt of the shell averages, the Hann-windowed cosine transform
                      of `trajectory.hann_cosine_transform` on `frequency` (THz); not divided by their value at t = 0
    dispersion_l/_t : the frequency (THz) at which c_l_qw / c_t_qw of a shell is largest."""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np
import torch

from . import _cuda, _lib
from ._driver import atom_offsets, boolean, check_tensor, integer, positive, read_state, state_tensor
from .data.graph_gpu import _ptr, _stream
from .trajectory import hann_cosine_transform, pair_index


def cartesian_q(lattice, hkl) -> np.ndarray:
    """q = 2 pi h L^-T [Q,3] of Miller triples `hkl` [Q,3] in the cell `lattice` (rows = lattice vectors)."""
    L = np.asarray(lattice, dtype=np.float64)
    return 2.0 * np.pi * np.asarray(hkl, dtype=np.float64).reshape(-1, 3) @ np.linalg.inv(L).T


def default_shell_width(lattice) -> float:
    """Half the length of the shortest reciprocal lattice vector of the cell."""
    return 0.5 * float(np.linalg.norm(cartesian_q(lattice, np.eye(3)), axis=1).min())


def shell_index(q_modulus, shell_width: float) -> np.ndarray:
    return np.floor(np.asarray(q_modulus, dtype=np.float64) / shell_width + 1e-9).astype(np.int64)


def q_vectors(lattice, q_max: float, max_per_shell: int | None = None, shell_width: float | None = None, seed: int = 0) -> np.ndarray:
    """All Miller triples h != 0 with |q| <= q_max in the cell `lattice`, one of each +-h pair (the accumulated quantities are even in
    h: the one whose first non-zero index is positive), sorted by |q| and then by h; [Q,3] int32.  With `max_per_shell` at most that
    many per |q| bin of `shell_width` (default: `default_shell_width`), picked by a permutation seeded with `seed`."""
    L = np.asarray(lattice, dtype=np.float64)
    q_max = positive("q_max", q_max)
    reach = [int(np.floor(q_max * np.linalg.norm(L[k]) / (2.0 * np.pi) * (1.0 + 1e-12))) for k in range(3)]   # |h_k| = |q . a_k| / 2 pi
    grid = np.stack(np.meshgrid(*[np.arange(-n, n + 1) for n in reach], indexing="ij"), axis=-1).reshape(-1, 3)
    first = np.where(grid[:, 0] != 0, grid[:, 0], np.where(grid[:, 1] != 0, grid[:, 1], grid[:, 2]))
    grid = grid[first > 0]
    mod = np.linalg.norm(cartesian_q(L, grid), axis=1)
    keep = mod <= q_max
    grid, mod = grid[keep], mod[keep]
    order = np.lexsort((grid[:, 2], grid[:, 1], grid[:, 0], np.round(mod, 9)))
    grid, mod = grid[order], mod[order]
    if max_per_shell is not None and len(grid):
        max_per_shell = integer("max_per_shell", max_per_shell, 1)
        width = default_shell_width(L) if shell_width is None else positive("shell_width", shell_width)
        shell = shell_index(mod, width)
        rng = np.random.default_rng(seed)
        rows = []
        for k in np.unique(shell):
            members = np.nonzero(shell == k)[0]
            if len(members) > max_per_shell:
                members = np.sort(members[rng.permutation(len(members))[:max_per_shell]])
            rows.append(members)
        grid = grid[np.concatenate(rows)]
    return np.ascontiguousarray(grid.astype(np.int32))


class SqState:
    """Accumulators of a batch on the device (m3g_sq_init).  `offsets`: S + 1 atom offsets; `species` [N]: local species index of every
    atom; `masses` [N] amu; `hkl`: one [Q_s,3] integer array per structure (an empty one is legal).  The ring of the last `n_lags`
    samples takes n_lags * Q * max_species * 80 bytes."""

    def __init__(self, n_atoms: int, offsets: Sequence[int], species, masses, hkl: Sequence, n_lags: int = 64, remove_com: bool = True,
                 max_species: int | None = None, device="cuda"):
        self.offsets = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64))
        self.N, self.S = integer("n_atoms", n_atoms, 1), int(len(self.offsets) - 1)
        self.species = np.ascontiguousarray(np.asarray(species, dtype=np.int32).reshape(-1))
        self.masses = np.ascontiguousarray(np.asarray(masses, dtype=np.float64).reshape(-1))
        if len(self.species) != self.N or len(self.masses) != self.N:
            raise ValueError(f"expected {self.N} species indices and masses")
        if len(hkl) != self.S:
            raise ValueError(f"hkl: expected one array per structure ({self.S})")
        per = [np.asarray(h, dtype=np.int32).reshape(-1, 3) for h in hkl]
        self.q_offsets = np.ascontiguousarray(np.concatenate([[0], np.cumsum([len(h) for h in per])]).astype(np.int64))
        self.hkl = np.ascontiguousarray(np.concatenate(per).astype(np.int32))
        self.Q = int(self.q_offsets[-1])
        self.M = int(self.species.max()) + 1 if max_species is None else integer("max_species", max_species, 1)
        self.lags = integer("n_lags", n_lags, 1)
        self.sizes = _lib.M3GSqSizes(self.N, self.S, self.Q, self.M, self.lags)
        self.params = _lib.M3GSqParams(1 if boolean("remove_com", remove_com) else 0, 0)
        self.P = self.M * (self.M + 1) // 2
        self.lib = _lib.load_library()
        self.device = torch.device(device)
        self.state = state_tensor(self.lib.m3g_sq_state_bytes, C.byref(self.sizes), device=self.device)
        with _cuda.on_device(self.device):
            _lib.check(self.lib.m3g_sq_init(C.byref(self.sizes), C.byref(self.params), self.offsets.ctypes.data, self.species.ctypes.data,
                                            self.masses.ctypes.data, self.q_offsets.ctypes.data, self.hkl.ctypes.data, _ptr(self.state),
                                            self.state.numel(), _stream()))

    def read(self) -> dict:
        """The raw accumulators, copied to the host (waits for the stream): f, cl, ct [Q, P, n_lags] (sums: not yet divided by atom
        counts or lag_count), lag_count [S, n_lags], n_samples, flags [S]."""
        S, G, shape = self.S, self.lags, (self.Q, self.P, self.lags)
        return read_state(self.lib.m3g_sq_read, (C.byref(self.sizes),), self.state,
                          (("f", np.float64, shape), ("cl", np.float64, shape), ("ct", np.float64, shape), ("lag_count", np.int64, (S, G)),
                           ("n_samples", np.int64, S), ("flags", np.int32, S)))

    def frame(self, lag: int = 0):
        """(rho [Q, M], j_L [Q, M], j_T [Q, M, 3]) complex: the ring entry `lag` samples back (0: the last sample), copied to the host
        (waits for the stream)."""
        rho, jl, jt = np.empty((self.Q, self.M), np.complex128), np.empty((self.Q, self.M), np.complex128), np.empty((self.Q, self.M, 3), np.complex128)
        with _cuda.on_device(self.device):
            _lib.check(self.lib.m3g_sq_frame(C.byref(self.sizes), _ptr(self.state), self.state.numel(), int(lag), rho.ctypes.data,
                                             jl.ctypes.data, jt.ctypes.data, _stream()))
        return rho, jl, jt


def sq_sample(state: SqState, pos: torch.Tensor, lattice: torch.Tensor, vel: torch.Tensor, forces: torch.Tensor | None = None,
              kick: float = 0.0) -> None:
    """One sample of the batch (m3g_sq_sample): `pos` [N,3] fp64 (unwrapped), `lattice` [S,3,3] fp64, `vel` [N,3] fp64; `forces` and
    `kick` as in `trajectory.traj_sample`.  Queued on the current stream; no wait, capture-safe."""
    check_tensor("pos", pos, (state.N, 3), torch.float64)
    check_tensor("lattice", lattice, (state.S, 3, 3), torch.float64)
    check_tensor("vel", vel, (state.N, 3), torch.float64)
    if forces is not None:
        check_tensor("forces", forces, (state.N, 3), torch.float32)
    with _cuda.on_device(state.device):
        _lib.check(state.lib.m3g_sq_sample(C.byref(state.sizes), C.byref(state.params), _ptr(state.state), state.state.numel(), _ptr(pos),
                                           _ptr(lattice), _ptr(vel), _ptr(forces), float(kick), _stream()))


# ---- host post-processing (numpy, one structure) ------------------------------------------------------------------------------------
def scattering_from_sums(f_sum, cl_sum, ct_sum, lag_count, counts, q_modulus, dt: float, shell_width: float, weights=None,
                         max_species: int | None = None) -> dict:
    """The normalised functions of one structure from its accumulated sums [Q, P, n_lags] (module docstring).  `counts` [n_sp]: atoms
    per species; `q_modulus` [Q]; `dt`: the time between two samples (fs); `weights` [n_sp]: scattering lengths, or None."""
    counts = np.asarray(counts, dtype=np.float64)
    lag_count = np.asarray(lag_count)
    q_modulus = np.asarray(q_modulus, dtype=np.float64)
    n_sp, G, Q = len(counts), len(lag_count), len(q_modulus)
    M = n_sp if max_species is None else max_species
    n_atoms = counts.sum()
    b = np.ones(n_sp) if weights is None else np.asarray(weights, dtype=np.float64)
    scale = 1.0 if weights is None else float((counts / n_atoms * b * b).sum())
    out = {"time": np.arange(G) * dt, "lag_count": lag_count.copy()}
    with np.errstate(divide="ignore", invalid="ignore"):
        norm = lag_count.astype(np.float64) * n_atoms
        for key, sums in (("f", f_sum), ("c_l", cl_sum), ("c_t", ct_sum)):
            sums = np.asarray(sums, dtype=np.float64).reshape(Q, -1, G)
            part = [[sums[:, pair_index(a, c, M)] / norm for c in range(n_sp)] for a in range(n_sp)]
            total = np.zeros((Q, G))
            for a in range(n_sp):
                for c in range(n_sp):   # ordered pairs
                    total += b[a] * b[c] * part[a][c]
            out[key], out[key + "_total"] = part, total / scale
    out["s"] = out["f_total"][:, 0].copy()
    shell = shell_index(q_modulus, shell_width)
    bins = np.unique(shell)
    member = [shell == k for k in bins]
    out["q_shell"] = np.array([q_modulus[m].mean() for m in member])
    out["shell_count"] = np.array([int(m.sum()) for m in member])
    for key in ("f", "c_l", "c_t"):
        out[key + "_shell"] = np.array([out[key + "_total"][m].mean(axis=0) for m in member]).reshape(len(bins), G)
    out["s_shell"] = out["f_shell"][:, 0].copy()
    have = bool((lag_count > 0).all()) and G > 1
    for key, spec in (("f", "s_qw"), ("c_l", "c_l_qw"), ("c_t", "c_t_qw")):
        freq, spectrum = hann_cosine_transform(out[key + "_shell"], dt)
        out[spec] = spectrum if have else np.full((len(bins), G), np.nan)
    out["frequency"] = freq * 1e3
    for key, spec in (("dispersion_l", "c_l_qw"), ("dispersion_t", "c_t_qw")):
        out[key] = np.array([out["frequency"][np.argmax(row)] if np.isfinite(row).all() else np.nan for row in out[spec]])
    return out


class ScatteringObservables:
    """What `MolecularDynamics.run(..., observables=...)` accumulates in reciprocal space.  `q_max` (1/A): every Miller triple of each
    structure's starting cell up to it (`q_vectors`, thinned to `max_per_shell` per |q| bin of `shell_width`, default half the shortest
    reciprocal lattice vector of the structure); or `hkl`: one [Q,3] integer array for all structures, or one per structure.
    `n_lags`: the correlations reach n_lags - 1 samples back; `sample_interval`: MD steps between two samples; `remove_com`:
    positions and velocities relative to the structure's centre of mass; `weights`: {atomic number: scattering length} for the
    weighted totals.  Each result dict of the run gains "scattering" (keys and normalisation: module docstring)."""

    def __init__(self, q_max: float | None = None, hkl=None, n_lags: int = 64, sample_interval: int = 1, remove_com: bool = True,
                 max_per_shell: int | None = 32, shell_width: float | None = None, weights: dict | None = None, seed: int = 0):
        if (q_max is None) == (hkl is None):
            raise ValueError("give exactly one of q_max and hkl")
        self.q_max = None if q_max is None else positive("q_max", q_max)
        self.hkl = hkl
        self.n_lags = integer("n_lags", n_lags, 1)
        if self.n_lags > _lib.SQ_MAX_LAGS:
            raise ValueError(f"n_lags must be at most {_lib.SQ_MAX_LAGS}")
        self.sample_interval = integer("sample_interval", sample_interval, 1)
        self.remove_com = boolean("remove_com", remove_com)
        self.max_per_shell = None if max_per_shell is None else integer("max_per_shell", max_per_shell, 1)
        self.shell_width = None if shell_width is None else positive("shell_width", shell_width)
        self.weights = None if weights is None else {int(z): float(b) for z, b in weights.items()}
        self.seed = int(seed)

    def _hkl_of(self, s: int, n_structs: int, lattice) -> np.ndarray:
        if self.hkl is None:
            h = q_vectors(lattice, self.q_max, self.max_per_shell, self.shell_width, self.seed)
        else:
            per = isinstance(self.hkl, (list, tuple)) and len(self.hkl) == n_structs and np.ndim(self.hkl[0]) == 2
            h = np.asarray(self.hkl[s] if per else self.hkl)
            if h.ndim != 2 or h.shape[1] != 3 or not np.array_equal(h, np.round(h)):
                raise ValueError("hkl must be [Q, 3] integer Miller triples (one array, or one per structure)")
            h = h.astype(np.int32)
        if len(h) > _lib.SQ_MAX_Q or (len(h) and np.abs(h).max() > _lib.SQ_MAX_INDEX):
            raise ValueError(f"structure {s}: {len(h)} q-vectors with indices up to {np.abs(h).max()}; at most {_lib.SQ_MAX_Q} vectors "
                             f"with |h_k| <= {_lib.SQ_MAX_INDEX}")
        return h

    def begin(self, lattices, atomic_numbers, masses, device) -> SqState:
        """The device state for these structures: atomic numbers mapped to local species indices (sorted unique Z per structure), the
        q-vectors of every structure.  The tables of the run stay on the state (`species_z`, `species_counts`, `hkl_per`, `lattices`)."""
        zs_all = [np.unique(np.asarray(z)) for z in atomic_numbers]
        for s, zs in enumerate(zs_all):
            if len(zs) > _lib.SQ_MAX_SPECIES:
                raise ValueError(f"structure {s}: {len(zs)} species; the scattering observables take at most {_lib.SQ_MAX_SPECIES}")
            if self.weights is not None and any(int(z) not in self.weights for z in zs):
                raise ValueError(f"structure {s}: weights has no scattering length for every atomic number of {zs.tolist()}")
        species = [np.searchsorted(zs, np.asarray(z)) for zs, z in zip(zs_all, atomic_numbers)]
        counts = [np.bincount(sp, minlength=len(zs)) for sp, zs in zip(species, zs_all)]
        lats = [np.asarray(L, dtype=np.float64).copy() for L in lattices]
        hkl = [self._hkl_of(s, len(lats), L) for s, L in enumerate(lats)]
        if sum(len(h) for h in hkl) == 0:
            raise ValueError("no q-vector in any structure: q_max is below the shortest reciprocal lattice vectors")
        offsets = atom_offsets(atomic_numbers)
        state = SqState(int(offsets[-1]), offsets, np.concatenate(species), np.concatenate(masses), hkl, self.n_lags, self.remove_com,
                        device=device)
        state.species_z, state.species_counts, state.hkl_per, state.lattices = zs_all, counts, hkl, lats
        return state

    def results(self, state: SqState, timestep: float) -> list:
        """One scattering dict per structure from the accumulators of a state `begin` returned (waits for the stream)."""
        acc = state.read()
        out = []
        for s, (zs, counts, hkl, L) in enumerate(zip(state.species_z, state.species_counts, state.hkl_per, state.lattices)):
            lo, hi = state.q_offsets[s], state.q_offsets[s + 1]
            q = cartesian_q(L, hkl)
            mod = np.linalg.norm(q, axis=1)
            width = self.shell_width if self.shell_width is not None else default_shell_width(L)
            b = None if self.weights is None else [self.weights[int(z)] for z in zs]
            res = {"species": zs.copy(), "n_samples": int(acc["n_samples"][s]), "hkl": hkl.copy(), "q": q, "q_modulus": mod,
                   "cell_valid": not bool(acc["flags"][s] & _lib.SQ_CELL)}
            res.update(scattering_from_sums(acc["f"][lo:hi], acc["cl"][lo:hi], acc["ct"][lo:hi], acc["lag_count"][s], counts, mod,
                                            self.sample_interval * timestep, width, b, state.M))
            out.append(res)
        return out
