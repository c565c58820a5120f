"""Batched finite-displacement phonons on the device: force constants, band structures, DOS and harmonic thermal properties (C ABI:
m3g_ph_*, csrc/m3g_phonons.hip).

The usual way to get phonons from an M3GNet potential is phonopy over an ASE calculator: one host round trip per displaced supercell,
evaluated one at a time.  `Phonons.run` takes a batch of structures instead.  Every displaced supercell of every structure is one row
block of a single fp64 `pos` written by one launch (`ph_displace`); the displaced batch is evaluated through the path `Relaxer` uses
(`VerletGraph.step`), in sub-batches of whole displaced supercells of one structure, at most `max_atoms` atoms; the force constants of the whole batch
are one launch (`ph_force_constants`) and the dynamical matrices of any number of q-points one launch (`ph_dynamical_matrices`).
Eigenvalues come from `torch.linalg.eigvalsh` on the device (the default) or from the library's own batched Hermitian Jacobi solver
(`eigensolver="jacobi"`, `linalg.eigh_batched`); eigenvectors, group velocities (`ph_group_velocities`, one launch) and the projected
DOS always from the latter.  DOS and thermal properties are fp64 torch ops on top.

Semantics (include/m3gnet_hip.h, "batched finite-displacement phonons"): phonopy's method with a diagonal supercell and no symmetry
reduction; +-delta along x, y, z for every atom of the home cell; central differences; the acoustic sum rule imposed on the self term
(asr=True); phonopy's dynamical matrix over the shortest images with weights 1 / multiplicity, Hermitised.  Frequencies in THz,
imaginary modes as negative numbers."""
from __future__ import annotations

import ctypes as C
import math
from typing import Sequence

import numpy as np
import torch

from . import _cuda, _lib
from .linalg import EIGH_MAX_N, eigh_batched
from ._driver import (Driver, boolean, check_tensor, gpu_device, integer, positive, state_tensor, structure_arrays, structure_masses,
                      sub_batches)
from .data import MaterialGraphKey as K
from .data.graph_gpu import _ptr, _stream
from .data.md import VerletGraph
from .nn.modules import Gradient

# CODATA (SI 2019 exact values; the atomic mass constant from CODATA 2018)
_EV = 1.602176634e-19          # J
_AMU = 1.66053906660e-27       # kg
_ANGSTROM = 1e-10              # m
_PLANCK = 6.62607015e-34       # J s
_BOLTZMANN = 1.380649e-23      # J / K
THZ_PER_SQRT_EV_A2_AMU = math.sqrt(_EV / (_ANGSTROM ** 2 * _AMU)) / (2.0 * math.pi) / 1e12   # 15.633304... THz
H_EV_PER_THZ = _PLANCK * 1e12 / _EV    # h nu in eV for nu = 1 THz
KB_EV = _BOLTZMANN / _EV               # eV / K

# The eigen-solver path.  complex128 `eigvalsh` works on the device but took 1.9 s for 8,000 12 x 12 matrices on the MI355X, against
# 6.7 ms for the real symmetric embedding [[A, -B], [B, A]] of H = A + iB, which holds every eigenvalue of H twice (profiles/phonons.txt).
EIGH_PATH = "real_embedding"
EIGENSOLVERS = ("embedding", "jacobi")   # Phonons(eigensolver=...): today's path (the default), or m3g_eigh_batched for 3n <= EIGH_MAX_N


def _check_eigensolver(name) -> str:
    if name not in EIGENSOLVERS:
        raise ValueError(f"eigensolver must be one of {EIGENSOLVERS}; got {name!r}")
    return name


def _sizes(n_unit: Sequence[int], supercells: np.ndarray) -> _lib.M3GPhSizes:
    cells = supercells.prod(axis=1)
    nu = np.asarray(n_unit, dtype=np.int64)
    return _lib.M3GPhSizes(len(nu), int(nu.sum()), int((nu * cells).sum()), int((nu * nu * cells).sum()))


def _check_supercells(supercells, n: int) -> np.ndarray:
    sc = np.asarray(supercells)
    if sc.shape == (3,):
        sc = np.broadcast_to(sc, (n, 3))
    if sc.shape != (n, 3) or not np.issubdtype(sc.dtype, np.integer) or (sc < 1).any():
        raise ValueError(f"supercells must be [{n}, 3] (or one [3]) integers >= 1; got {np.asarray(supercells).tolist()}")
    return np.ascontiguousarray(sc.astype(np.int32))


class PhononState:
    """Finite-displacement phonons of a batch of structures on the device (m3g_ph_init).  `lattices` [S] of [3,3] (rows = lattice
    vectors), `positions` [S] of [n_s,3] (Cartesian, A), `masses` [S] of [n_s] (amu), `supercells` [S,3] (diagonal supercell), `delta`
    (A).  Holds `pos` [rows, 3] float64 (the displaced batch, written by `ph_displace`), `phi` [n_pairs, 3, 3] float64, `sums` [U, 9]
    float64 (raw sum_j Phi[u, j]) and `nonfinite` [S] int32 (written by `ph_force_constants`).  Row blocks of structure s: `row_offsets`,
    `super_sizes`; force-constant rows: `pair_offsets`."""

    def __init__(self, lattices, positions, masses, supercells, delta: float = 0.01, device="cuda"):
        self.S = len(lattices)
        if not (len(positions) == len(masses) == self.S) or self.S == 0:
            raise ValueError("lattices, positions and masses must hold one entry per structure (at least one)")
        self.lattices = np.ascontiguousarray(np.stack([np.asarray(L, dtype=np.float64).reshape(3, 3) for L in lattices]))
        self.positions = np.ascontiguousarray(np.concatenate([np.asarray(p, dtype=np.float64).reshape(-1, 3) for p in positions]))
        self.masses = np.ascontiguousarray(np.concatenate([np.asarray(m, dtype=np.float64).reshape(-1) for m in masses]))
        self.n_unit = np.array([len(np.asarray(p).reshape(-1, 3)) for p in positions], dtype=np.int64)
        if len(self.masses) != len(self.positions):
            raise ValueError("masses must hold one value per atom")
        self.supercells = _check_supercells(supercells, self.S)
        self.delta = float(delta)
        cells = self.supercells.astype(np.int64).prod(axis=1)
        self.super_sizes = self.n_unit * cells
        self.unit_offsets = np.concatenate([[0], np.cumsum(self.n_unit)]).astype(np.int64)
        self.row_offsets = np.concatenate([[0], np.cumsum((1 + 6 * self.n_unit) * self.super_sizes)]).astype(np.int64)
        self.pair_offsets = np.concatenate([[0], np.cumsum(self.n_unit * self.super_sizes)]).astype(np.int64)
        self.sizes = _sizes(self.n_unit, self.supercells)
        self.rows = int(self.row_offsets[-1])
        self.device = gpu_device(device, "PhononState")
        self.lib = _lib.load_library()
        self.state = state_tensor(self.lib.m3g_ph_state_bytes, C.byref(self.sizes), device=self.device)
        self.pos = torch.zeros(self.rows, 3, dtype=torch.float64, device=self.device)
        self.phi = torch.full((self.sizes.n_pairs, 3, 3), float("nan"), dtype=torch.float64, device=self.device)
        self.sums = torch.full((self.sizes.n_unit_atoms, 9), float("nan"), dtype=torch.float64, device=self.device)
        self.nonfinite = torch.zeros(self.S, dtype=torch.int32, device=self.device)
        with _cuda.on_device(self.device):
            _lib.check(self.lib.m3g_ph_init(C.byref(self.sizes), self.unit_offsets.ctypes.data, self.supercells.ctypes.data,
                                            self.lattices.ctypes.data, self.positions.ctypes.data, self.masses.ctypes.data, self.delta,
                                            _ptr(self.state), self.state.numel(), _stream()))

    def supercell_lattice(self, s: int) -> np.ndarray:
        return self.supercells[s][:, None].astype(np.float64) * self.lattices[s]

    def supercell_numbers(self, s: int, atomic_numbers) -> np.ndarray:
        """Per-atom values of unit cell s tiled in the supercell order j = l n_u + b."""
        return np.tile(np.asarray(atomic_numbers).reshape(-1), int(self.supercells[s].astype(np.int64).prod()))


def ph_displace(state: PhononState) -> torch.Tensor:
    """Positions of every row of the displaced batch (m3g_ph_displace), written to and returned as `state.pos`.  Queued on the current
    stream; no wait, capture-safe."""
    with _cuda.on_device(state.device):
        _lib.check(state.lib.m3g_ph_displace(C.byref(state.sizes), _ptr(state.state), state.state.numel(), _ptr(state.pos), _stream()))
    return state.pos


def ph_force_constants(state: PhononState, forces: torch.Tensor, asr: bool = True) -> torch.Tensor:
    """Force constants of every structure (m3g_ph_force_constants) from `forces` [rows, 3] float32 of the displaced batch: written to
    and returned as `state.phi`; `state.sums` and `state.nonfinite` too.  Queued on the current stream; no wait, capture-safe."""
    check_tensor("forces", forces, (state.rows, 3), torch.float32, state.pos.device)
    with _cuda.on_device(state.device):
        _lib.check(state.lib.m3g_ph_force_constants(C.byref(state.sizes), _ptr(state.state), state.state.numel(), _ptr(forces),
                                                    1 if asr else 0, _ptr(state.phi), _ptr(state.sums), _ptr(state.nonfinite), _stream()))
    return state.phi


def ph_dynamical_matrices(state: PhononState, structure: int, q) -> torch.Tensor:
    """Dynamical matrices [Q, 3n, 3n] complex128 (eV / (A^2 amu)) of structure `structure` at the fractional q-points `q` [Q, 3]
    (m3g_ph_dynmat over `state.phi`).  One launch."""
    s = int(structure)
    if not 0 <= s < state.S:
        raise ValueError(f"structure must lie in [0, {state.S})")
    q = torch.as_tensor(q, dtype=torch.float64, device=state.device).reshape(-1, 3).contiguous()
    n = int(state.n_unit[s])
    out = torch.zeros(len(q), 3 * n, 3 * n, dtype=torch.complex128, device=state.device)
    if len(q) == 0:
        return out
    q_struct = torch.full((len(q),), s, dtype=torch.int32, device=state.device)
    with _cuda.on_device(state.device):
        _lib.check(state.lib.m3g_ph_dynmat(C.byref(state.sizes), _ptr(state.state), state.state.numel(), _ptr(state.phi), len(q), _ptr(q),
                                           _ptr(q_struct), n, _ptr(out), _stream()))
    return out


def ph_dynamical_matrix_gradients(state: PhononState, structure: int, q) -> torch.Tensor:
    """dD / dq_alpha [Q, 3, 3n, 3n] complex128 (eV / (A amu)) of structure `structure` at the fractional q-points `q` [Q, 3], with
    respect to the CARTESIAN q in 1/A without 2 pi -- the convention of `band_structure`'s `distance` (m3g_ph_dynmat_gradient over
    `state.phi`: every image term of D times 2 pi i r_alpha).  One launch."""
    s = int(structure)
    if not 0 <= s < state.S:
        raise ValueError(f"structure must lie in [0, {state.S})")
    q = torch.as_tensor(q, dtype=torch.float64, device=state.device).reshape(-1, 3).contiguous()
    n = int(state.n_unit[s])
    out = torch.zeros(len(q), 3, 3 * n, 3 * n, dtype=torch.complex128, device=state.device)
    if len(q) == 0:
        return out
    q_struct = torch.full((len(q),), s, dtype=torch.int32, device=state.device)
    with _cuda.on_device(state.device):
        _lib.check(state.lib.m3g_ph_dynmat_gradient(C.byref(state.sizes), _ptr(state.state), state.state.numel(), _ptr(state.phi), len(q),
                                                    _ptr(q), _ptr(q_struct), n, _ptr(out), _stream()))
    return out


def unit_direction(direction) -> np.ndarray:
    """`direction` [3] (finite, not zero) scaled to unit length."""
    d = np.asarray(direction, dtype=np.float64)
    if d.shape != (3,) or not np.isfinite(d).all() or not np.linalg.norm(d) > 0.0:
        raise ValueError(f"direction must be three finite numbers, not all zero; got {np.asarray(direction).tolist()}")
    return np.ascontiguousarray(d / np.linalg.norm(d))


def ph_group_velocities(eigenvalues: torch.Tensor, eigenvectors: torch.Tensor, gradient: torch.Tensor, direction=(1.0, 2.0, 3.0),
                        degeneracy_tolerance: float = 1e-4, cutoff_frequency: float = 1e-3) -> torch.Tensor:
    """Group velocities [Q, n, 3] float64 (THz A; 1 THz A = 100 m/s), v = d f / d q_cart (m3g_ph_group_velocities, one launch, one
    workgroup per q): `eigenvalues` [Q, n] of D (ascending), `eigenvectors` [Q, n, n] (columns), `gradient` [Q, 3, n, n]
    (`ph_dynamical_matrix_gradients`).  Modes closer than `degeneracy_tolerance` (THz) form a set; a set of several modes is rotated to
    the eigenvectors of its block of sum_alpha direction_alpha dD_alpha first (phonopy's rule, `direction` normalised here).  A mode
    below `cutoff_frequency` (THz) gets exactly 0; a q with a non-finite eigenvalue NaN.  n <= _lib.PH_GV_MAX_N."""
    if not (torch.is_tensor(eigenvalues) and eigenvalues.dim() == 2):
        raise ValueError("eigenvalues must be a [Q, n] float64 tensor")
    nq, n = (int(k) for k in eigenvalues.shape)
    d = unit_direction(direction)
    tol, cut = float(degeneracy_tolerance), float(cutoff_frequency)
    if not (math.isfinite(tol) and tol >= 0.0):
        raise ValueError(f"degeneracy_tolerance must be finite and >= 0; got {degeneracy_tolerance}")
    if not (math.isfinite(cut) and cut >= 0.0):
        raise ValueError(f"cutoff_frequency must be finite and >= 0; got {cutoff_frequency}")
    if not 1 <= n <= _lib.PH_GV_MAX_N:
        raise ValueError(f"ph_group_velocities: n = {n} is outside [1, {_lib.PH_GV_MAX_N}] (the LDS of one workgroup holds two n x "
                         f"{_lib.PH_GV_MAX_SET} blocks of a degenerate set)")
    dev = eigenvalues.device
    if dev.type != "cuda":
        raise ValueError(f"ph_group_velocities runs on a GPU device; got {dev}")
    check_tensor("eigenvalues", eigenvalues, (nq, n), torch.float64, dev)
    check_tensor("eigenvectors", eigenvectors, (nq, n, n), torch.complex128, dev)
    check_tensor("gradient", gradient, (nq, 3, n, n), torch.complex128, dev)
    v = torch.empty(nq, n, 3, dtype=torch.float64, device=dev)
    if nq:
        with _cuda.on_device(dev):
            _lib.check(_lib.load_library().m3g_ph_group_velocities(nq, n, _ptr(eigenvalues), _ptr(eigenvectors), _ptr(gradient), tol, cut,
                                                                   d.ctypes.data, _ptr(v), _stream()))
    return v


def _eigh(d: torch.Tensor):
    """(eigenvalues [Q, n] ascending, eigenvectors [Q, n, n] as columns) of Hermitian [Q, n, n] complex128 on the device: the
    library's Jacobi solver up to EIGH_MAX_N, `torch.linalg.eigh` beyond (slow: 1.8 - 2.5 s for 8,000 12 x 12 matrices,
    profiles/phonons.txt -- but still on the device)."""
    if d.shape[-1] <= EIGH_MAX_N:
        w, v, _ = eigh_batched(d, eigenvectors=True)   # (a flagged matrix is NaN already)
        return w, v
    w, v = torch.linalg.eigh(d)
    return w.contiguous(), v.contiguous()


def _eigvalsh(d: torch.Tensor) -> torch.Tensor:
    """Ascending eigenvalues [..., n] of Hermitian matrices [..., n, n] (complex128): every other eigenvalue of the real embedding."""
    a, b = d.real, d.imag
    emb = torch.cat([torch.cat([a, -b], dim=-1), torch.cat([b, a], dim=-1)], dim=-2)
    return torch.linalg.eigvalsh(emb)[..., ::2]


def to_frequencies(eigenvalues: torch.Tensor) -> torch.Tensor:
    """THz from eigenvalues in eV / (A^2 amu): sign(lambda) sqrt(|lambda|) x THZ_PER_SQRT_EV_A2_AMU (imaginary modes negative)."""
    return torch.sign(eigenvalues) * torch.sqrt(torch.abs(eigenvalues)) * THZ_PER_SQRT_EV_A2_AMU


def gaussian_dos(frequencies: torch.Tensor, weights: torch.Tensor, grid: torch.Tensor, sigma: float) -> torch.Tensor:
    """sum_q w_q sum_modes exp(-(f - f_qi)^2 / (2 sigma^2)) / (sqrt(2 pi) sigma) on `grid` (states / THz per unit cell, with sum w = 1)."""
    f = frequencies.reshape(len(weights), -1)
    x = (grid[:, None, None] - f[None]) / sigma
    g = torch.exp(-0.5 * x * x) / (math.sqrt(2.0 * math.pi) * sigma)
    return (g.sum(dim=2) * weights[None]).sum(dim=1)


def projected_gaussian_dos(frequencies: torch.Tensor, projections: torch.Tensor, weights: torch.Tensor, grid: torch.Tensor,
                           sigma: float) -> torch.Tensor:
    """`gaussian_dos` per atom [n_atoms, G]: the Gaussian of mode (q, i) weighted by `projections` [Q, n_atoms, modes]."""
    f = frequencies.reshape(len(weights), -1)
    x = (grid[:, None, None] - f[None]) / sigma
    g = torch.exp(-0.5 * x * x) / (math.sqrt(2.0 * math.pi) * sigma)   # [G, Q, modes]
    return torch.einsum("gqm,qam,q->ag", g, projections, weights)


def harmonic_thermal(frequencies: torch.Tensor, weights: torch.Tensor, temperatures: torch.Tensor, cutoff_frequency: float = 1e-3) -> dict:
    """Harmonic free energy F, entropy S, heat capacity Cv and energy E per unit cell (eV, eV/K) at `temperatures` (K, >= 0) from
    frequencies [Q, modes] (THz) with q weights [Q] summing to 1.  Modes below `cutoff_frequency` (THz; imaginary ones included) are
    left out and counted in `n_excluded` (over the whole mesh)."""
    f = frequencies.reshape(len(weights), -1)
    keep = f >= cutoff_frequency
    w = (weights[:, None] * keep).reshape(-1)
    e = (torch.where(keep, f, torch.zeros_like(f)) * H_EV_PER_THZ).reshape(-1)   # h nu, eV
    T = temperatures.reshape(-1, 1)
    kT = KB_EV * T
    hot = T > 0
    x = torch.where(hot & (w > 0), e / torch.where(hot, kT, torch.ones_like(kT)), torch.full_like(kT * e, float("inf")))
    em1 = torch.expm1(-x)                              # e^-x - 1 (-1 at T = 0)
    bose = torch.where(torch.isinf(x), torch.zeros_like(x), -torch.exp(-x) / em1)   # 1 / (e^x - 1)
    log_term = torch.log(-em1)                         # ln(1 - e^-x)
    F = (w * (0.5 * e + torch.where(hot, kT * log_term, torch.zeros_like(x)))).sum(1)
    E = (w * (0.5 * e + e * bose)).sum(1)
    S = (w * torch.where(hot, -KB_EV * log_term + e * bose / torch.where(hot, T, torch.ones_like(T)), torch.zeros_like(x))).sum(1)
    cv_mode = torch.where(torch.isinf(x), torch.zeros_like(x), KB_EV * x * x * bose * (1.0 + bose))   # x^2 e^x / (e^x - 1)^2
    Cv = (w * cv_mode).sum(1)
    return {"temperatures": temperatures.reshape(-1), "free_energy": F, "entropy": S, "heat_capacity": Cv, "energy": E,
            "n_excluded": int((~keep).sum())}


def monkhorst_pack(n, gamma_centered: bool = True) -> np.ndarray:
    """[n1 n2 n3, 3] fractional q-points: Gamma-centred (i / n) or Monkhorst-Pack ((2i - n + 1) / (2n)), folded into [-1/2, 1/2)."""
    n = np.broadcast_to(np.asarray(n), (3,))
    if not np.issubdtype(n.dtype, np.integer) or (n < 1).any():
        raise ValueError(f"mesh must be integers >= 1; got {np.asarray(n).tolist()}")
    axes = [np.arange(k) / k if gamma_centered else (2 * np.arange(k) - k + 1) / (2 * k) for k in n]
    q = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)
    return q - np.floor(q + 0.5)


class PhononResult:
    """Phonons of one structure: `force_constants` [n, N_s, 3, 3] (eV/A^2, phonopy's compact layout), `residual_fmax` (largest force
    of the undisplaced supercell, eV/A), `asr_violation` (raw max |sum_j Phi|), `asr_correction` [n, 3, 3] (what the sum rule added to
    each self term; zeros with asr=False), `error` (a non-finite force: everything is NaN).  Frequencies (THz) come from the device
    on demand: `frequencies(q)`, `band_structure`, `mesh`, `dos`, `thermal_properties`, and with eigenvectors `modes(q)`,
    `group_velocities`, `projected_dos`."""

    def __init__(self, state: PhononState, s: int, asr: bool, max_qpoints: int, cutoff_frequency: float, residual_fmax: float,
                 phi: np.ndarray, sums: np.ndarray, nonfinite: int, eigensolver: str = "embedding"):
        self._state, self._s, self._max_q, self.cutoff_frequency = state, s, max_qpoints, cutoff_frequency
        self.eigensolver = _check_eigensolver(eigensolver)
        n, ns = int(state.n_unit[s]), int(state.super_sizes[s])
        self.n_atoms, self.supercell = n, tuple(int(k) for k in state.supercells[s])
        self.lattice = state.lattices[s].copy()
        self.masses = state.masses[state.unit_offsets[s]:state.unit_offsets[s + 1]].copy()
        self.positions = state.positions[state.unit_offsets[s]:state.unit_offsets[s + 1]].copy()
        self.atomic_numbers = None   # (set by `Phonons.run`, which knows them: `NormalModeAnalysis` builds its MD supercell from them)
        self.force_constants = phi.reshape(n, ns, 3, 3)
        self.residual_fmax = residual_fmax
        self.error = nonfinite != 0
        raw = sums.reshape(n, 3, 3)
        self.asr_violation = float(np.abs(raw).max())
        self.asr_correction = -raw if asr else np.zeros_like(raw)

    def frequencies(self, q) -> np.ndarray:
        """[Q, 3n] frequencies (THz, ascending, imaginary modes negative) at fractional q-points [Q, 3]."""
        q = np.asarray(q, dtype=np.float64).reshape(-1, 3)
        n3 = 3 * self.n_atoms
        if self.error:
            return np.full((len(q), n3), np.nan)
        out = []
        for a in range(0, len(q), self._max_q):   # q batches of at most max_qpoints: each matrix is independent of the others
            d = ph_dynamical_matrices(self._state, self._s, q[a:a + self._max_q])
            lam = eigh_batched(d, eigenvectors=False)[0] if self.eigensolver == "jacobi" and n3 <= EIGH_MAX_N else _eigvalsh(d)
            out.append(to_frequencies(lam).cpu().numpy())
        return np.concatenate(out) if out else np.zeros((0, n3))

    def modes(self, q) -> dict:
        """`frequencies` [Q, 3n] (THz, ascending, imaginary modes negative) and `eigenvectors` [Q, 3n, 3n] complex128 (column k
        belongs to frequency k, orthonormal; the polarisation of atom u in rows 3u .. 3u + 2) at fractional q-points [Q, 3].  The
        library's Jacobi solver for 3n <= EIGH_MAX_N, `torch.linalg.eigh` on the device beyond (slow)."""
        q = np.asarray(q, dtype=np.float64).reshape(-1, 3)
        n3 = 3 * self.n_atoms
        if self.error:
            return {"frequencies": np.full((len(q), n3), np.nan), "eigenvectors": np.full((len(q), n3, n3), np.nan, dtype=np.complex128)}
        f, e = [np.zeros((0, n3))], [np.zeros((0, n3, n3), dtype=np.complex128)]
        for a in range(0, len(q), self._max_q):
            w, v = _eigh(ph_dynamical_matrices(self._state, self._s, q[a:a + self._max_q]))
            f.append(to_frequencies(w).cpu().numpy())
            e.append(v.cpu().numpy())
        return {"frequencies": np.concatenate(f), "eigenvectors": np.concatenate(e)}

    def group_velocities(self, q, direction=(1, 2, 3), degeneracy_tolerance: float = 1e-4) -> np.ndarray:
        """[Q, 3n, 3] group velocities d f / d q_cart (THz A; 1 THz A = 100 m/s; q_cart in 1/A without 2 pi, as `band_structure`'s
        `distance`) at fractional q-points [Q, 3], in the order of `frequencies`.  Phonopy's rules: modes closer than
        `degeneracy_tolerance` (THz) are rotated within their set to the eigenvectors of the derivative along `direction` (Cartesian,
        normalised here) first; a mode below `cutoff_frequency` gets exactly 0."""
        q = np.asarray(q, dtype=np.float64).reshape(-1, 3)
        n3 = 3 * self.n_atoms
        unit_direction(direction)   # (refused before any work)
        if not (math.isfinite(float(degeneracy_tolerance)) and float(degeneracy_tolerance) >= 0.0):
            raise ValueError(f"degeneracy_tolerance must be finite and >= 0; got {degeneracy_tolerance}")
        if n3 > _lib.PH_GV_MAX_N:
            raise ValueError(f"group_velocities: 3n = {n3} is above {_lib.PH_GV_MAX_N} (_lib.PH_GV_MAX_N)")
        if self.error:
            return np.full((len(q), n3, 3), np.nan)
        out = [np.zeros((0, n3, 3))]
        for a in range(0, len(q), self._max_q):
            w, v = _eigh(ph_dynamical_matrices(self._state, self._s, q[a:a + self._max_q]))
            g = ph_dynamical_matrix_gradients(self._state, self._s, q[a:a + self._max_q])
            out.append(ph_group_velocities(w, v, g, direction, degeneracy_tolerance, self.cutoff_frequency).cpu().numpy())
        return np.concatenate(out)

    def band_structure(self, path, npts: int = 51) -> dict:
        """Frequencies along the straight segments between consecutive fractional q-points of `path` (npts points per segment, both
        ends included).  Returns q [Q,3], distance [Q] (cumulative, 1/A in Cartesian reciprocal space, no 2 pi), frequencies [Q, 3n]
        and the distances of the path's vertices."""
        path = np.asarray(path, dtype=np.float64)
        if path.ndim != 2 or path.shape[1] != 3 or len(path) < 2:
            raise ValueError("path must be [>= 2, 3] fractional q-points")
        npts = integer("npts", npts, 2)
        t = np.linspace(0.0, 1.0, npts)[:, None]
        q = np.concatenate([a + t * (b - a) for a, b in zip(path[:-1], path[1:])])
        recip = np.linalg.inv(self.lattice).T   # rows: reciprocal vectors (no 2 pi)
        steps = np.linalg.norm(np.diff(q, axis=0) @ recip, axis=1)
        dist = np.concatenate([[0.0], np.cumsum(steps)])
        return {"q": q, "distance": dist, "vertices": dist[::npts].tolist() + [float(dist[-1])], "frequencies": self.frequencies(q)}

    def mesh(self, n, gamma_centered: bool = True) -> dict:
        """Frequencies on an n1 x n2 x n3 mesh (Gamma-centred, or Monkhorst-Pack) with uniform weights."""
        q = monkhorst_pack(n, gamma_centered)
        return {"q": q, "weights": np.full(len(q), 1.0 / len(q)), "frequencies": self.frequencies(q)}

    def dos(self, mesh=(10, 10, 10), sigma: float = 0.1, npts: int = 201, fmin: float | None = None, fmax: float | None = None,
            gamma_centered: bool = True) -> dict:
        """Gaussian-smeared density of states (states / THz per unit cell; integrates to 3n) on a mesh."""
        if not (math.isfinite(sigma) and sigma > 0):
            raise ValueError(f"sigma must be finite and > 0; got {sigma}")
        m = self.mesh(mesh, gamma_centered)
        f = m["frequencies"]
        lo = float(np.nanmin(f)) - 5 * sigma if fmin is None else float(fmin)
        hi = float(np.nanmax(f)) + 5 * sigma if fmax is None else float(fmax)
        dev = self._state.device
        grid = torch.linspace(lo, hi, int(npts), dtype=torch.float64, device=dev)
        g = gaussian_dos(torch.tensor(f, device=dev), torch.tensor(m["weights"], device=dev), grid, float(sigma))
        return {"frequency_points": grid.cpu().numpy(), "dos": g.cpu().numpy()}

    def projected_dos(self, mesh=(10, 10, 10), sigma: float = 0.1, npts: int = 201, fmin: float | None = None, fmax: float | None = None,
                      gamma_centered: bool = True) -> dict:
        """Gaussian-smeared density of states per atom [n_atoms, npts] (states / THz per unit cell) on a mesh: each mode's Gaussian
        weighted by sum_a |e_ua|^2, which sums to 1 over the atoms -- so the rows sum to the total DOS of the same frequencies (`dos`
        of a result with eigensolver="jacobi" where 3n <= EIGH_MAX_N: the eigenvalues have the same bits with and without vectors)."""
        if not (math.isfinite(sigma) and sigma > 0):
            raise ValueError(f"sigma must be finite and > 0; got {sigma}")
        q = monkhorst_pack(mesh, gamma_centered)
        m = self.modes(q)
        f = m["frequencies"]
        lo = float(np.nanmin(f)) - 5 * sigma if fmin is None else float(fmin)
        hi = float(np.nanmax(f)) + 5 * sigma if fmax is None else float(fmax)
        dev = self._state.device
        grid = torch.linspace(lo, hi, int(npts), dtype=torch.float64, device=dev)
        e = torch.tensor(m["eigenvectors"], device=dev)
        p = (e.real ** 2 + e.imag ** 2).reshape(len(q), self.n_atoms, 3, -1).sum(dim=2)   # [Q, atom, mode]
        g = projected_gaussian_dos(torch.tensor(f, device=dev), p, torch.full((len(q),), 1.0 / len(q), dtype=torch.float64, device=dev),
                                   grid, float(sigma))
        return {"frequency_points": grid.cpu().numpy(), "projected_dos": g.cpu().numpy()}

    def thermal_properties(self, temperatures, mesh=(10, 10, 10), gamma_centered: bool = True) -> dict:
        """Harmonic F, S, Cv, E per unit cell (eV, eV/K) at `temperatures` (K) over a mesh; `n_excluded` modes below cutoff_frequency."""
        T = np.asarray(temperatures, dtype=np.float64).reshape(-1)
        if not (np.isfinite(T).all() and (T >= 0).all()):
            raise ValueError("temperatures must be finite and >= 0")
        m = self.mesh(mesh, gamma_centered)
        dev = self._state.device
        out = harmonic_thermal(torch.tensor(m["frequencies"], device=dev), torch.tensor(m["weights"], device=dev), torch.tensor(T, device=dev),
                               self.cutoff_frequency)
        return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}


class Phonons(Driver):
    """Batched finite-displacement phonons under an M3GNet potential.

    `model`: the `Gradient` returned by `build_model` (evaluated, like `Relaxer`'s, through a pair-virial engine made from its
    `Sequential`).  `delta`: displacement (A); `asr`: impose the acoustic sum rule; `max_atoms`: atoms per engine sub-batch (whole
    displaced supercells of one structure; a supercell larger than it is evaluated alone); `max_qpoints`: q-points per
    dynamical-matrix launch; `eigensolver`: "embedding" (the default: `torch.linalg.eigvalsh` on the real embedding) or "jacobi"
    (`frequencies` through the library's batched Hermitian solver where 3n <= EIGH_MAX_N, the embedding beyond).  A structure's results are bitwise the same alone or in any batch for a given `max_atoms`; a different
    `max_atoms` can change the engine's sub-batches and so the last bits of its forces."""

    def __init__(self, model: Gradient, delta: float = 0.01, asr: bool = True, max_atoms: int = 200_000, max_qpoints: int = 4096,
                 cutoff_frequency: float = 1e-3, skin: float = 0.5, device="cuda", eigensolver: str = "embedding"):
        super().__init__(model, skin, device)
        self.eigensolver = _check_eigensolver(eigensolver)
        self.delta, self.asr = positive("delta", delta), boolean("asr", asr)
        self.max_atoms, self.max_qpoints = integer("max_atoms", max_atoms, 1), integer("max_qpoints", max_qpoints, 1)
        cutoff_frequency = float(cutoff_frequency)
        if not (math.isfinite(cutoff_frequency) and cutoff_frequency >= 0.0):
            raise ValueError(f"cutoff_frequency must be finite and >= 0; got {cutoff_frequency}")
        self.cutoff_frequency = cutoff_frequency

    def _check(self, lattices, positions, atomic_numbers, supercells, masses):
        lat, pos, z = structure_arrays(lattices, positions, atomic_numbers)
        return lat, pos, z, _check_supercells(supercells, len(lat)), structure_masses(masses, z)

    def run(self, lattices: Sequence, positions: Sequence, atomic_numbers: Sequence, supercells, masses=None) -> list:
        """Phonons of every structure (lattices [3,3] rows = lattice vectors, positions [n_s,3] Cartesian, atomic_numbers [n_s],
        supercells [S,3] or one [3] diagonal supercell, masses [n_s] amu per structure or None for the standard atomic weights).
        Returns one `PhononResult` per structure."""
        lat, pos, z, sc, m = self._check(lattices, positions, atomic_numbers, supercells, masses)
        model, dev = self.model, self.device
        cfg = model.engine.cfg
        st = PhononState(lat, pos, m, sc, self.delta, device=dev)
        ph_displace(st)
        forces = torch.empty(st.rows, 3, dtype=torch.float32, device=st.pos.device)
        row = 0   # the displaced supercells in row order, structure by structure (`sub_batches`)
        for s in range(st.S):
            ns = int(st.super_sizes[s])
            for _, nc in sub_batches(1 + 6 * int(st.n_unit[s]), ns, self.max_atoms):
                n_rows = nc * ns
                vg = VerletGraph([st.supercell_lattice(s)] * nc, [st.supercell_numbers(s, z[s])] * nc, cfg.cutoff, cfg.threebody_cutoff,
                                 skin=self.skin, device=dev)
                out = vg.step(model, st.pos[row:row + n_rows])
                vg.raise_on_step_errors("phonons")
                forces[row:row + n_rows] = out[K.FORCES]
                row += n_rows
        ph_force_constants(st, forces, self.asr)
        # residual forces: the undisplaced supercell of every structure
        norms = forces.double().norm(dim=1)
        res_f = [float(norms[int(st.row_offsets[s]):int(st.row_offsets[s] + st.super_sizes[s])].max()) for s in range(st.S)]
        phi, sums, bad = st.phi.cpu().numpy(), st.sums.cpu().numpy(), st.nonfinite.cpu().numpy()
        self.forces = forces   # (the displaced batch's forces, kept for inspection)
        res = [PhononResult(st, s, self.asr, self.max_qpoints, self.cutoff_frequency, res_f[s],
                            phi[int(st.pair_offsets[s]):int(st.pair_offsets[s + 1])], sums[int(st.unit_offsets[s]):int(st.unit_offsets[s + 1])],
                            int(bad[s]), self.eigensolver) for s in range(st.S)]
        for r, a in zip(res, z):
            r.atomic_numbers = a.copy()
        return res
