"""Trajectory observables accumulated on the device: radial distribution function, mean-square displacement and velocity
autocorrelation of every structure of a batch (C ABI: m3g_traj_*, csrc/m3g_trajectory.hip).

`MolecularDynamics.run(..., observables=TrajectoryObservables(...))` samples the trajectory on the device while it integrates -- no
frame ever goes to the host -- and returns, per structure, g(r), coordination numbers, MSD, VACF, diffusion coefficients and the
vibrational density of states.  `TrajState` / `traj_sample` are the layer below (they mirror `DynState` / `dyn_step`) and take any
frames.

Conventions (the same ones are restated in tests/trajectory_reference.py).  The device keeps, per structure, the integer counts
H_ab[k] of UNORDERED pairs i < j of species (a <= b) whose minimum-image distance falls in bin k of width r_max / rdf_bins, the
number of samples n and the sum of the cell volumes; <V> = volume_sum / n, v_k = 4 pi (r_{k+1}^3 - r_k^3) / 3, N_a atoms of species
a, N atoms in all:
    g_ab[k]    = <V> H_ab[k] / (n N_a N_b v_k)          a != b
    g_aa[k]    = 2 <V> H_aa[k] / (n N_a^2 v_k)
    g_total[k] = 2 <V> sum_ab H_ab[k] / (n N^2 v_k)
    coordination[a][b][k] = (ordered a -> b pairs up to the upper edge of bin k) / (n N_a): the running sum of H_ab (a != b) or 2 H_aa
The minimum image is exact below half the smallest perpendicular width of the cell; `rdf_valid` is False when a sample saw r_max
above it (NPT: the cell moves).  Per species a and lag l (time = l * sample_interval * timestep, fs), over the samples that have a
frame l samples back (lag_count[l] of them) and the N_a atoms of the species:
    msd[a][l]  = < |r_i(t + l) - r_i(t)|^2 >            A^2   (unwrapped positions; with remove_com relative to the centre of mass)
    vacf[a][l] = < v_i(t + l) . v_i(t) >                A^2/fs^2
    diffusion_msd[a]  = slope of the least-squares line through msd over `fit_window` (fractions of the longest lag) / 6
    diffusion_vacf[a] = trapezoid integral of vacf over the lags / 3
    vdos[a][k] = 2 int_0^T c(t) w(t) cos(2 pi f_k t) dt, c = vacf / vacf[0], w = (1 + cos(pi t / T)) / 2 (Hann), T the longest lag,
                 f_k = k / (2 n_lags dt) -- `vdos_frequency` in THz
Diffusion coefficients come in A^2/fs and in cm^2/s (1 A^2/fs = 0.1 cm^2/s)."""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np
import torch

from . import _cuda, _lib
from ._driver import atom_offsets, boolean, check_tensor, integer, positive, read_state, state_tensor
from .data.graph_gpu import _ptr, _stream

A2_FS_TO_CM2_S = 0.1


def _trapezoid(y, x):
    """Trapezoid integral of y over x along the last axis (numpy.trapezoid, which numpy 1.x does not have)."""
    y, x = np.asarray(y, dtype=np.float64), np.asarray(x, dtype=np.float64)
    return (0.5 * (y[..., 1:] + y[..., :-1]) * np.diff(x)).sum(axis=-1)


def perpendicular_widths(lattice) -> np.ndarray:
    """w_k = V / |a_i x a_j| of a cell (rows = lattice vectors): the distances between its opposite faces."""
    L = np.asarray(lattice, dtype=np.float64)
    cross = np.stack([np.cross(L[1], L[2]), np.cross(L[2], L[0]), np.cross(L[0], L[1])])
    return abs(np.linalg.det(L)) / np.linalg.norm(cross, axis=1)


def pair_index(a: int, b: int, max_species: int) -> int:
    """Row of the species pair (a, b) in the histogram: row-major upper triangle."""
    a, b = min(a, b), max(a, b)
    return a * max_species - a * (a - 1) // 2 + (b - a)


class TrajState:
    """Accumulators of a batch on the device (m3g_traj_init).  `n_atoms`: N; `offsets`: S + 1 atom offsets; `species` [N]: local
    species index of every atom, 0 .. max_species - 1; `masses` [N] amu.  `rdf_bins` = 0 switches the RDF off (then `rdf_r_max` is
    unused), `n_lags` = 0 the correlations (the ring of the last n_lags frames takes n_lags * N * 48 bytes)."""

    def __init__(self, n_atoms: int, offsets: Sequence[int], species, masses, rdf_r_max: float | None = None, rdf_bins: int = 0,
                 n_lags: int = 0, remove_com: bool = True, max_species: int | None = None, device="cuda"):
        self.offsets = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64))
        self.N, self.S = integer("n_atoms", n_atoms, 1), int(len(self.offsets) - 1)
        self.species = np.ascontiguousarray(np.asarray(species, dtype=np.int32).reshape(-1))
        self.masses = np.ascontiguousarray(np.asarray(masses, dtype=np.float64).reshape(-1))
        if len(self.species) != self.N or len(self.masses) != self.N:
            raise ValueError(f"expected {self.N} species indices and masses")
        self.M = int(self.species.max()) + 1 if max_species is None else integer("max_species", max_species, 1)
        self.bins, self.lags = integer("rdf_bins", rdf_bins, 0), integer("n_lags", n_lags, 0)
        self.r_max = positive("rdf_r_max", rdf_r_max) if self.bins else 1.0
        self.sizes = _lib.M3GTrajSizes(self.N, self.S, self.M, self.bins, self.lags)
        self.params = _lib.M3GTrajParams(self.r_max, 1 if boolean("remove_com", remove_com) else 0)
        self.P = self.M * (self.M + 1) // 2
        self.lib = _lib.load_library()
        self.device = torch.device(device)
        self.state = state_tensor(self.lib.m3g_traj_state_bytes, C.byref(self.sizes), device=self.device)
        with _cuda.on_device(self.device):
            _lib.check(self.lib.m3g_traj_init(C.byref(self.sizes), C.byref(self.params), self.offsets.ctypes.data, self.species.ctypes.data,
                                              self.masses.ctypes.data, _ptr(self.state), self.state.numel(), _stream()))

    def read(self) -> dict:
        """The raw accumulators, copied to the host (waits for the stream): hist [S, P, rdf_bins] uint64, msd / vacf [S, max_species,
        n_lags] (sums: not yet divided by atom counts or lag_count), lag_count [S, n_lags], n_samples, volume_sum, flags [S]."""
        S, M, B, G = self.S, self.M, self.bins, self.lags
        return read_state(self.lib.m3g_traj_read, (C.byref(self.sizes),), self.state,   # (a switched-off observable: an array of no elements)
                          (("hist", np.uint64, (S, self.P, B)), ("msd", np.float64, (S, M, G)), ("vacf", np.float64, (S, M, G)),
                           ("lag_count", np.int64, (S, G)), ("n_samples", np.int64, S), ("volume_sum", np.float64, S),
                           ("flags", np.int32, S)))

    def frame(self, lag: int = 0):
        """(positions, velocities) [N, 3] of the stored frame `lag` samples back (0: the last sample), copied to the host: the full-step
        velocities the sampler reconstructed, centre of mass removed where asked for (waits for the stream)."""
        pos, vel = np.empty((self.N, 3)), np.empty((self.N, 3))
        with _cuda.on_device(self.device):
            _lib.check(self.lib.m3g_traj_frame(C.byref(self.sizes), _ptr(self.state), self.state.numel(), int(lag), pos.ctypes.data,
                                               vel.ctypes.data, _stream()))
        return pos, vel


def traj_sample(state: TrajState, pos: torch.Tensor, lattice: torch.Tensor | None, vel: torch.Tensor | None,
                forces: torch.Tensor | None = None, kick: float = 0.0) -> None:
    """One sample of the batch (m3g_traj_sample): `pos` [N,3] fp64 (unwrapped), `lattice` [S,3,3] fp64 (needed by the RDF), `vel` [N,3]
    fp64 (needed by the correlations).  With `forces` [N,3] float32 the stored velocity is vel + kick * kappa * forces / m: give the
    integrator's velocities (`DynState.velocities`) and the forces of `pos` BEFORE the `dyn_step` of the same forces, with kick =
    timestep / 2 (0 before the first step).  Queued on the current stream; no wait, capture-safe."""
    check_tensor("pos", pos, (state.N, 3), torch.float64)
    if lattice is not None:
        check_tensor("lattice", lattice, (state.S, 3, 3), torch.float64)
    if vel is not None:
        check_tensor("vel", vel, (state.N, 3), torch.float64)
    if forces is not None:
        check_tensor("forces", forces, (state.N, 3), torch.float32)
    with _cuda.on_device(state.device):
        _lib.check(state.lib.m3g_traj_sample(C.byref(state.sizes), C.byref(state.params), _ptr(state.state), state.state.numel(), _ptr(pos),
                                             _ptr(lattice), _ptr(vel), _ptr(forces), float(kick), _stream()))


# ---- host post-processing (numpy, one structure) ------------------------------------------------------------------------------------
def rdf_from_counts(hist, counts, n_samples: int, volume_sum: float, r_max: float, max_species: int | None = None) -> dict:
    """g(r) and coordination numbers of one structure from its pair counts `hist` [P, bins] (module docstring); `counts` [n_sp]: atoms
    per species.  Species pairs without atoms, or a run without samples, give NaN."""
    counts = np.asarray(counts, dtype=np.float64)
    n_sp = len(counts)
    M = n_sp if max_species is None else max_species
    hist = np.asarray(hist).astype(np.float64)
    bins = hist.shape[1]
    edges = np.linspace(0.0, r_max, bins + 1)
    shell = 4.0 * np.pi / 3.0 * (edges[1:] ** 3 - edges[:-1] ** 3)
    n = float(n_samples)
    with np.errstate(divide="ignore", invalid="ignore"):
        v_mean = volume_sum / n
        g = [[None] * n_sp for _ in range(n_sp)]
        cn = [[None] * n_sp for _ in range(n_sp)]
        for a in range(n_sp):
            for b in range(n_sp):
                h = hist[pair_index(a, b, M)]
                ordered = 2.0 * h if a == b else h   # ordered a -> b pairs
                g[a][b] = v_mean * ordered / (n * counts[a] * counts[b] * shell)
                cn[a][b] = np.cumsum(ordered) / (n * counts[a])
        used = [pair_index(a, b, M) for a in range(n_sp) for b in range(a, n_sp)]
        g_total = 2.0 * v_mean * hist[used].sum(axis=0) / (n * counts.sum() ** 2 * shell)
    return {"r": 0.5 * (edges[1:] + edges[:-1]), "r_edges": edges, "g": g, "g_total": g_total, "coordination": cn}


def hann_cosine_transform(c, dt: float):
    """(f_k, 2 int_0^T c(t) w(t) cos(2 pi f_k t) dt) of a function sampled every `dt` along the last axis of `c` [..., G]: w = (1 + cos(pi
    t / T)) / 2 (Hann), T the longest lag, f_k = k / (2 G dt) in 1/fs, the integral by the trapezoid rule.  The transform behind the
    VDOS here and the spectra of `scattering.py`."""
    c = np.asarray(c, dtype=np.float64)
    G = c.shape[-1]
    time = np.arange(G) * dt
    freq = np.arange(G) / (2.0 * G * dt)
    window = 0.5 * (1.0 + np.cos(np.pi * time / time[-1])) if G > 1 else np.ones(1)
    kernel = np.cos(2.0 * np.pi * freq[:, None] * time[None, :])
    return freq, 2.0 * _trapezoid(kernel * (c * window)[..., None, :], time)


def correlations_from_sums(msd_sum, vacf_sum, lag_count, counts, dt: float, fit_window=(0.2, 0.8)) -> dict:
    """MSD, VACF, diffusion coefficients and VDOS of one structure from its accumulated sums [n_sp, n_lags] (module docstring); `dt`:
    the time between two samples (fs)."""
    counts = np.asarray(counts, dtype=np.float64)
    lag_count = np.asarray(lag_count)
    G = len(lag_count)
    time = np.arange(G) * dt
    with np.errstate(divide="ignore", invalid="ignore"):
        norm = counts[:, None] * lag_count[None, :].astype(np.float64)
        msd = np.asarray(msd_sum, dtype=np.float64) / norm
        vacf = np.asarray(vacf_sum, dtype=np.float64) / norm
    n_sp = len(counts)
    lo, hi = fit_window[0] * time[-1], fit_window[1] * time[-1]
    fit = (time >= lo) & (time <= hi) & (lag_count > 0)
    d_msd, d_vacf = np.full(n_sp, np.nan), np.full(n_sp, np.nan)
    freq = np.arange(G) / (2.0 * G * dt)   # 1/fs
    vdos = np.full((n_sp, G), np.nan)
    have = lag_count > 0
    for a in range(n_sp):
        if fit.sum() >= 2:
            d_msd[a] = np.polyfit(time[fit], msd[a][fit], 1)[0] / 6.0
        if have.all() and G > 1:
            d_vacf[a] = _trapezoid(vacf[a], time) / 3.0
            with np.errstate(divide="ignore", invalid="ignore"):
                vdos[a] = hann_cosine_transform(vacf[a] / vacf[a][0], dt)[1]
    return {"time": time, "msd": msd, "vacf": vacf, "lag_count": lag_count.copy(), "diffusion_msd": d_msd, "diffusion_vacf": d_vacf,
            "diffusion_msd_cm2_s": d_msd * A2_FS_TO_CM2_S, "diffusion_vacf_cm2_s": d_vacf * A2_FS_TO_CM2_S,
            "vdos_frequency": freq * 1e3, "vdos": vdos}


class TrajectoryObservables:
    """What `MolecularDynamics.run(..., observables=...)` accumulates.  `rdf_r_max` (A; None: half the smallest perpendicular width of
    any starting cell, the largest range the minimum image is exact for) and `rdf_bins` (0: no RDF); `n_lags` (0: no MSD / VACF): the
    correlations reach n_lags - 1 samples back; `sample_interval`: MD steps between two samples; `remove_com`: positions and
    velocities relative to the structure's centre of mass; `fit_window`: the part of the lag range (fractions of the longest lag)
    the MSD line is fitted over.  Each result dict of the run gains "observables" (keys and normalisation: module docstring).  A
    structure whose `error` flag is set stopped moving when its forces became non-finite: its observables are returned as they are
    and are not meaningful."""

    def __init__(self, rdf_r_max: float | None = None, rdf_bins: int = 200, n_lags: int = 0, sample_interval: int = 1,
                 remove_com: bool = True, fit_window=(0.2, 0.8)):
        self.rdf_bins = integer("rdf_bins", rdf_bins, 0)
        self.n_lags = integer("n_lags", n_lags, 0)
        if self.rdf_bins > _lib.TRAJ_MAX_BINS or self.n_lags > _lib.TRAJ_MAX_LAGS:
            raise ValueError(f"rdf_bins and n_lags must be at most {_lib.TRAJ_MAX_BINS} and {_lib.TRAJ_MAX_LAGS}")
        if self.rdf_bins == 0 and self.n_lags == 0:
            raise ValueError("rdf_bins and n_lags are both 0: nothing to accumulate")
        self.rdf_r_max = None if rdf_r_max is None else positive("rdf_r_max", rdf_r_max)
        self.sample_interval = integer("sample_interval", sample_interval, 1)
        self.remove_com = boolean("remove_com", remove_com)
        lo, hi = (float(x) for x in fit_window)
        if not 0.0 <= lo < hi <= 1.0:
            raise ValueError(f"fit_window must be 0 <= low < high <= 1; got {fit_window}")
        self.fit_window = (lo, hi)

    def begin(self, lattices, atomic_numbers, masses, device) -> TrajState:
        """The device state for these structures: atomic numbers mapped to local species indices (sorted unique Z per structure).
        The species and count tables of the run stay on the state (`species_z`, `species_counts`), not on this object."""
        zs_all = [np.unique(np.asarray(z)) for z in atomic_numbers]
        for s, zs in enumerate(zs_all):
            if len(zs) > _lib.TRAJ_MAX_SPECIES:
                raise ValueError(f"structure {s}: {len(zs)} species; the trajectory observables take at most {_lib.TRAJ_MAX_SPECIES}")
        species = [np.searchsorted(zs, np.asarray(z)) for zs, z in zip(zs_all, atomic_numbers)]
        counts = [np.bincount(sp, minlength=len(zs)) for sp, zs in zip(species, zs_all)]
        half = min(float(perpendicular_widths(L).min()) for L in lattices) / 2.0
        r_max = self.rdf_r_max
        if self.rdf_bins:
            if r_max is None:
                r_max = half
            elif r_max > half * (1.0 + 1e-12):   # (the rounding of the width itself: a / 2 of a cubic cell passes, as on the device)
                raise ValueError(f"rdf_r_max = {r_max} A is above half the smallest perpendicular width of the cells ({half:.6g} A): "
                                 "the minimum image is not exact there")
        offsets = atom_offsets(atomic_numbers)
        state = TrajState(int(offsets[-1]), offsets, np.concatenate(species), np.concatenate(masses), r_max, self.rdf_bins, self.n_lags,
                          self.remove_com, device=device)
        state.species_z, state.species_counts = zs_all, counts
        return state

    def results(self, state: TrajState, timestep: float) -> list:
        """One observables dict per structure from the accumulators of a state `begin` returned (waits for the stream)."""
        acc = state.read()
        out = []
        for s, (zs, counts) in enumerate(zip(state.species_z, state.species_counts)):
            obs = {"species": zs.copy(), "n_samples": int(acc["n_samples"][s])}
            if state.bins:
                obs.update(rdf_from_counts(acc["hist"][s], counts, obs["n_samples"], float(acc["volume_sum"][s]), state.r_max, state.M))
                obs["rdf_valid"] = not bool(acc["flags"][s] & _lib.TRAJ_RDF_RANGE)
            if state.lags:
                n_sp = len(zs)
                obs.update(correlations_from_sums(acc["msd"][s][:n_sp], acc["vacf"][s][:n_sp], acc["lag_count"][s], counts,
                                                  self.sample_interval * timestep, self.fit_window))
            out.append(obs)
        return out
