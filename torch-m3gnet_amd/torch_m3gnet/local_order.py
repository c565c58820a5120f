"""Local-order observables accumulated on the device: the Steinhardt bond-orientational order parameters q_l of every atom, their
neighbour average qbar_l (Lechner and Dellago), the solid-like atoms of ten Wolde and Frenkel and their connected clusters, for every
structure of a batch (C ABI: m3g_lo_*, csrc/m3g_local_order.hip).  The per-atom companion of `trajectory.py` and `scattering.py`:
which atoms are crystalline, in which structure, and how large the solid region is.

`MolecularDynamics.run(..., observables=LocalOrderObservables(...))` (alone, or in a list beside the other two kinds) samples the
trajectory on the device while it integrates -- no frame ever goes to the host -- and every result dict gains "local_order".  It needs
positions and cells only, so it also runs with "npt_mtk" and "npt_mtk_cell".  `LoState` / `lo_sample` are the layer below and take any
frames; `local_order` is the one-shot form for static structures.

Definitions (the same ones are restated in include/m3gnet_hip.h and tests/local_order_reference.py).  Atom j != i is a neighbour of i
when the minimum-image distance r_ij < r_cut of the structure (strict; all species count; valid while r_cut <= half the smallest
perpendicular width of the CURRENT cell, checked per sample).  With Y_lm the orthonormal spherical harmonics (Condon-Shortley phase)
and N_b(i) the number of neighbours:
    q_lm(i)    = 1/N_b sum_{j in nb(i)} Y_lm(rhat_ij)              q_l = sqrt(4 pi/(2l+1) sum_{m=-l..l} |q_lm|^2)        (0 without neighbours)
    qbar_lm(i) = (q_lm(i) + sum_{j in nb(i)} q_lm(j)) / (N_b + 1)  qbar_l likewise
    Q_lm       = sum_i N_b(i) q_lm(i) / sum_i N_b(i)               Q_l likewise: the order of the whole structure (0 without a bond)
    s_ij       = Re sum_m q_Lm(i) q_Lm*(j) / (|q_L(i)| |q_L(j)|)   L = solid_degree; the bond is connected when s_ij > solid_threshold
    atom i is solid-like when it has >= solid_bonds connected bonds; solid-like neighbours share a cluster, whose label is the
    smallest atom index in it (non-solid atoms: -1).
Reference values of (q4, q6): fcc (0.19094, 0.57452), hcp (0.09722, 0.48476), bcc with both shells (0.03637, 0.51069), simple cubic
(0.76376, 0.35355), a liquid ~ (0, 0.3) per atom and ~ 0 after the neighbour average.
A sample in which a structure raises a flag (`cell`: singular cell; `range`: r_cut beyond half the width; `neighbors`: an atom with more
than 32 neighbours; `nonfinite`: a non-finite or zero distance) is left out of that structure's histograms, sums and series
(`n_skipped` counts it)."""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np
import torch

from . import _cuda, _lib
from ._driver import atom_offsets, check_tensor, integer, positive, read_state, state_tensor, structure_arrays
from .data.graph_gpu import _ptr, _stream

FLAG_NAMES = (("cell", _lib.LO_CELL), ("range", _lib.LO_RANGE), ("neighbors", _lib.LO_NEIGHBORS), ("nonfinite", _lib.LO_NONFINITE))
ORDERS = _lib.LO_MAX_DEGREE + 1   # m = 0 .. 12: the row of one degree in a q_lm entry
NB_BINS = _lib.LO_MAX_NEIGHBORS + 1


def check_degrees(degrees, solid_degree) -> tuple:
    """`degrees` as a tuple of 1 .. 3 distinct integers in 1 .. 12 that holds `solid_degree`."""
    degrees = tuple(integer("degrees", l, 1) for l in (degrees if isinstance(degrees, (list, tuple, np.ndarray)) else (degrees,)))
    if not 1 <= len(degrees) <= _lib.LO_MAX_DEGREES or len(set(degrees)) != len(degrees) or max(degrees) > _lib.LO_MAX_DEGREE:
        raise ValueError(f"degrees must be 1 .. {_lib.LO_MAX_DEGREES} distinct integers in 1 .. {_lib.LO_MAX_DEGREE}; got {degrees}")
    if solid_degree not in degrees:
        raise ValueError(f"solid_degree {solid_degree} must be one of the degrees {degrees}")
    return degrees


class LoState:
    """Accumulators of a batch on the device (m3g_lo_init).  `offsets`: S + 1 atom offsets; `species` [N]: local species index of every
    atom; `r_cut` [S] (A): the neighbour cut-off of every structure; `degrees`: the l of q_l.  The lists and the per-atom frame take
    936 + 224 len(degrees) bytes per atom."""

    def __init__(self, n_atoms: int, offsets: Sequence[int], species, r_cut, degrees=(4, 6), solid_degree: int = 6,
                 solid_threshold: float = 0.5, solid_bonds: int = 7, hist_bins: int = 100, series_cap: int = 4096,
                 max_species: int | None = None, device="cuda"):
        self.offsets = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64))
        self.N, self.S = integer("n_atoms", n_atoms, 1), int(len(self.offsets) - 1)
        self.species = np.ascontiguousarray(np.asarray(species, dtype=np.int32).reshape(-1))
        self.r_cut = np.ascontiguousarray(np.broadcast_to(np.asarray(r_cut, dtype=np.float64), (self.S,)))
        if len(self.species) != self.N:
            raise ValueError(f"expected {self.N} species indices")
        self.degrees = check_degrees(degrees, solid_degree)
        self.D = len(self.degrees)
        self.M = int(self.species.max()) + 1 if max_species is None else integer("max_species", max_species, 1)
        self.B, self.K = integer("hist_bins", hist_bins, 1), integer("series_cap", series_cap, 1)
        self.sizes = _lib.M3GLoSizes(self.N, self.S, self.M, self.D, self.B, self.K)
        padded = self.degrees + (0,) * (_lib.LO_MAX_DEGREES - self.D)
        self.params = _lib.M3GLoParams((C.c_int32 * _lib.LO_MAX_DEGREES)(*padded), int(solid_degree), integer("solid_bonds", solid_bonds, 1),
                                       float(solid_threshold))
        self.lib = _lib.load_library()
        self.device = torch.device(device)
        self.state = state_tensor(self.lib.m3g_lo_state_bytes, C.byref(self.sizes), device=self.device)
        with _cuda.on_device(self.device):
            _lib.check(self.lib.m3g_lo_init(C.byref(self.sizes), C.byref(self.params), self.offsets.ctypes.data, self.species.ctypes.data,
                                            self.r_cut.ctypes.data, _ptr(self.state), self.state.numel(), _stream()))

    def read(self) -> dict:
        """The raw accumulators, copied to the host (waits for the stream): hist_q, hist_qbar [S, M, D, bins] and hist_nb [S, M, 33]
        (counts), moments [S, M, D, 4] (sums of q_l, q_l^2, qbar_l, qbar_l^2), series_counts [S, cap, 3] (n_solid, n_clusters,
        largest_cluster), series_order [S, cap, 2, D] (Q_l, mean qbar_l), n_samples, n_skipped, flags [S]."""
        S, M, D, B, K = self.S, self.M, self.D, self.B, self.K
        return read_state(self.lib.m3g_lo_read, (C.byref(self.sizes),), self.state,
                          (("hist_q", np.uint64, (S, M, D, B)), ("hist_qbar", np.uint64, (S, M, D, B)), ("hist_nb", np.uint64, (S, M, NB_BINS)),
                           ("moments", np.float64, (S, M, D, 4)), ("series_counts", np.int64, (S, K, 3)),
                           ("series_order", np.float64, (S, K, 2, D)), ("n_samples", np.int64, S), ("n_skipped", np.int64, S),
                           ("flags", np.int32, S)))

    def frame(self) -> dict:
        """The per-atom arrays of the last sample, copied to the host (waits for the stream): qlm [N, D, 13] complex (m = 0 .. 12, zero
        beyond l), ql, qbar [N, D], n_neighbors (uncapped), n_conn, solid (0 / 1), label [N] int32."""
        N, D = self.N, self.D
        out = read_state(self.lib.m3g_lo_frame, (C.byref(self.sizes),), self.state,
                         (("qlm", np.float64, (N, D, ORDERS, 2)), ("ql", np.float64, (N, D)), ("qbar", np.float64, (N, D)),
                          ("n_neighbors", np.int32, N), ("n_conn", np.int32, N), ("solid", np.int32, N), ("label", np.int32, N)))
        out["qlm"] = out["qlm"].view(np.complex128).reshape(N, D, ORDERS)
        return out


def lo_sample(state: LoState, pos: torch.Tensor, lattice: torch.Tensor) -> None:
    """One sample of the batch (m3g_lo_sample): `pos` [N,3] fp64 (unwrapped or not), `lattice` [S,3,3] fp64.  Queued on the current
    stream; no wait, capture-safe."""
    check_tensor("pos", pos, (state.N, 3), torch.float64)
    check_tensor("lattice", lattice, (state.S, 3, 3), torch.float64)
    with _cuda.on_device(state.device):
        _lib.check(state.lib.m3g_lo_sample(C.byref(state.sizes), C.byref(state.params), _ptr(state.state), state.state.numel(), _ptr(pos),
                                           _ptr(lattice), _stream()))


def decode_flags(flags: int) -> dict:
    """{"cell", "range", "neighbors", "nonfinite"}: whether a sample of the structure raised the flag (it was then left out)."""
    return {name: bool(int(flags) & bit) for name, bit in FLAG_NAMES}


# ---- host post-processing (numpy, one structure) ------------------------------------------------------------------------------------
def local_order_from_sums(hist_q, hist_qbar, hist_nb, moments, series_counts, series_order, n_samples: int, counts, sample_interval: int,
                          timestep: float) -> dict:
    """The statistics of one structure from its accumulators (`LoState.read`, the rows of its own species): hist_q, hist_qbar
    [n_sp, D, bins] and hist_nb [n_sp, 33] counts, moments [n_sp, D, 4], series_counts [cap, 3], series_order [cap, 2, D]; `counts`
    [n_sp]: atoms per species.  Means and variances are over atoms and samples; the histograms are densities on [0, 1] (their sum times
    the bin width is 1), the coordination histogram the share of atoms per neighbour count."""
    counts = np.asarray(counts, dtype=np.float64)
    hist_q, hist_qbar = np.asarray(hist_q, dtype=np.float64), np.asarray(hist_qbar, dtype=np.float64)
    moments = np.asarray(moments, dtype=np.float64)
    bins = hist_q.shape[-1]
    kept = min(int(n_samples), len(series_counts))
    out = {"bin_centres": (np.arange(bins) + 0.5) / bins}
    with np.errstate(divide="ignore", invalid="ignore"):
        terms = (counts * n_samples)[:, None]   # values behind every sum of a species
        for key, at in (("q", 0), ("qbar", 2)):
            mean = moments[:, :, at] / terms
            out[key + "_mean"] = mean
            out[key + "_var"] = np.maximum(moments[:, :, at + 1] / terms - mean * mean, 0.0)
        out["q_hist"], out["qbar_hist"] = hist_q * bins / terms[:, :, None], hist_qbar * bins / terms[:, :, None]
        out["coordination_hist"] = np.asarray(hist_nb, dtype=np.float64) / terms
    n_solid = np.asarray(series_counts)[:kept, 0].copy()
    step = np.arange(kept) * sample_interval
    out.update(step=step, time=step * timestep, n_solid=n_solid, solid_fraction=n_solid / counts.sum(),
               n_clusters=np.asarray(series_counts)[:kept, 1].copy(), largest_cluster=np.asarray(series_counts)[:kept, 2].copy(),
               Q=np.asarray(series_order)[:kept, 0].copy(), mean_qbar=np.asarray(series_order)[:kept, 1].copy())
    return out


def cutoffs_of(r_cut, atomic_numbers) -> np.ndarray:
    """[S] neighbour cut-offs (A) from `r_cut`: one value, one per structure, or {atomic number: value} looked up with every
    structure's majority species (the smallest atomic number among equals)."""
    S = len(atomic_numbers)
    if isinstance(r_cut, dict):
        table = {int(z): positive("r_cut", v) for z, v in r_cut.items()}
        out = []
        for s, z in enumerate(atomic_numbers):
            zs, n = np.unique(np.asarray(z), return_counts=True)
            major = int(zs[np.argmax(n)])
            if major not in table:
                raise ValueError(f"structure {s}: r_cut has no entry for its majority species {major}")
            out.append(table[major])
        return np.asarray(out, dtype=np.float64)
    r = np.asarray(r_cut, dtype=np.float64)
    if r.ndim > 1 or (r.ndim == 1 and len(r) != S):
        raise ValueError(f"r_cut: expected one value, one per structure ({S}) or a dict by atomic number")
    return np.array([positive("r_cut", v) for v in np.broadcast_to(r, (S,))])


class LocalOrderObservables:
    """What `MolecularDynamics.run(..., observables=...)` accumulates per atom.  `r_cut` (A): the neighbour cut-off -- one value, one per
    structure, or {atomic number: value} taken from a structure's majority species; between the first and the second shell (fcc, hcp)
    or past the second (bcc).  `degrees`: up to three l in 1 .. 12; `solid_degree`, `solid_threshold`, `solid_bonds`: the solid-like
    bond criterion; `hist_bins`: bins of the q_l and qbar_l histograms on [0, 1]; `sample_interval`: MD steps between two samples;
    `max_samples`: rows of the series (later samples still enter the histograms).  Each result dict of the run gains "local_order"."""

    def __init__(self, r_cut, degrees=(4, 6), solid_degree: int = 6, solid_threshold: float = 0.5, solid_bonds: int = 7, hist_bins: int = 100,
                 sample_interval: int = 10, max_samples: int = 4096):
        if isinstance(r_cut, dict):
            self.r_cut = {int(z): positive("r_cut", v) for z, v in r_cut.items()}
        else:
            self.r_cut = np.asarray(r_cut, dtype=np.float64)
            if self.r_cut.ndim > 1 or not (np.isfinite(self.r_cut).all() and (self.r_cut > 0).all()):
                raise ValueError("r_cut must be one finite value > 0 (A), one per structure, or a dict by atomic number")
        self.degrees = check_degrees(degrees, solid_degree)
        self.solid_degree = int(solid_degree)
        self.solid_threshold = float(solid_threshold)
        if not -1.0 <= self.solid_threshold <= 1.0:
            raise ValueError(f"solid_threshold must lie in -1 .. 1; got {solid_threshold}")
        self.solid_bonds = integer("solid_bonds", solid_bonds, 1)
        if self.solid_bonds > _lib.LO_MAX_NEIGHBORS:
            raise ValueError(f"solid_bonds must be at most {_lib.LO_MAX_NEIGHBORS}")
        self.hist_bins = integer("hist_bins", hist_bins, 1)
        if self.hist_bins > _lib.LO_MAX_BINS:
            raise ValueError(f"hist_bins must be at most {_lib.LO_MAX_BINS}")
        self.sample_interval = integer("sample_interval", sample_interval, 1)
        self.max_samples = integer("max_samples", max_samples, 1)
        if self.max_samples > _lib.LO_MAX_SERIES:
            raise ValueError(f"max_samples must be at most {_lib.LO_MAX_SERIES}")

    def begin(self, lattices, atomic_numbers, masses, device) -> LoState:
        """The device state for these structures: atomic numbers mapped to local species indices (sorted unique Z per structure), the
        cut-off of every structure.  `masses` is ignored (the signature of the sibling observables).  The tables of the run stay on the
        state (`species_z`, `species_counts`)."""
        zs_all = [np.unique(np.asarray(z)) for z in atomic_numbers]
        for s, zs in enumerate(zs_all):
            if len(zs) > _lib.LO_MAX_SPECIES:
                raise ValueError(f"structure {s}: {len(zs)} species; the local-order observables take at most {_lib.LO_MAX_SPECIES}")
        cut = cutoffs_of(self.r_cut, atomic_numbers)
        species = [np.searchsorted(zs, np.asarray(z)) for zs, z in zip(zs_all, atomic_numbers)]
        counts = [np.bincount(sp, minlength=len(zs)) for sp, zs in zip(species, zs_all)]
        offsets = atom_offsets(atomic_numbers)
        state = LoState(int(offsets[-1]), offsets, np.concatenate(species), cut, self.degrees, self.solid_degree, self.solid_threshold,
                        self.solid_bonds, self.hist_bins, self.max_samples, device=device)
        state.species_z, state.species_counts = zs_all, counts
        return state

    def results(self, state: LoState, timestep: float) -> list:
        """One local-order dict per structure from the accumulators of a state `begin` returned (waits for the stream): species,
        degrees, r_cut, n_samples, n_skipped, flags; q_mean, q_var, qbar_mean, qbar_var [n_sp, D]; q_hist, qbar_hist [n_sp, D, bins]
        with bin_centres; coordination_hist [n_sp, 33]; the series step, time, solid_fraction, n_solid, n_clusters, largest_cluster,
        Q and mean_qbar [n, D] (row k is the k-th sample that was kept: step = k sample_interval while nothing was skipped); and
        `frame`, the per-atom arrays of the last sample (`LoState.frame`; None before any sample)."""
        acc = state.read()
        frame = state.frame() if int((acc["n_samples"] + acc["n_skipped"]).max()) > 0 else None
        out = []
        for s, (zs, counts) in enumerate(zip(state.species_z, state.species_counts)):
            n_sp, rows = len(zs), slice(state.offsets[s], state.offsets[s + 1])
            res = {"species": zs.copy(), "degrees": np.array(state.degrees), "r_cut": float(state.r_cut[s]),
                   "n_samples": int(acc["n_samples"][s]), "n_skipped": int(acc["n_skipped"][s]), "flags": decode_flags(acc["flags"][s])}
            res.update(local_order_from_sums(acc["hist_q"][s, :n_sp], acc["hist_qbar"][s, :n_sp], acc["hist_nb"][s, :n_sp],
                                             acc["moments"][s, :n_sp], acc["series_counts"][s], acc["series_order"][s], res["n_samples"],
                                             counts, self.sample_interval, timestep))
            res["frame"] = None if frame is None else {key: val[rows].copy() for key, val in frame.items()}
            out.append(res)
        return out


def local_order(lattices, positions, atomic_numbers, r_cut, degrees=(4, 6), solid_degree: int = 6, solid_threshold: float = 0.5,
                solid_bonds: int = 7, device="cuda") -> list:
    """The local order of static structures (the output of `Relaxer`, say): one init, one sample and one frame for the batch.  Returns
    one dict per structure: qlm [n, D, 13] complex, ql, qbar [n, D], n_neighbors, n_conn, solid, label [n]; n_solid, n_clusters,
    largest_cluster, solid_fraction; Q, mean_qbar [D]; flags (a raised flag: the per-atom arrays are as computed, the structure's
    counts and Q are None)."""
    lat, pos, z = structure_arrays(lattices, positions, atomic_numbers)
    obs = LocalOrderObservables(r_cut, degrees, solid_degree, solid_threshold, solid_bonds, hist_bins=1, sample_interval=1, max_samples=1)
    state = obs.begin(lat, z, None, device)
    lo_sample(state, torch.tensor(np.concatenate(pos), dtype=torch.float64, device=state.device),
              torch.tensor(np.stack(lat), dtype=torch.float64, device=state.device))
    acc, frame = state.read(), state.frame()
    out = []
    for s in range(state.S):
        rows = slice(state.offsets[s], state.offsets[s + 1])
        res = {key: val[rows].copy() for key, val in frame.items()}
        ok = int(acc["n_samples"][s]) == 1
        counts = acc["series_counts"][s, 0]
        res.update(degrees=np.array(state.degrees), flags=decode_flags(acc["flags"][s]),
                   n_solid=int(counts[0]) if ok else None, n_clusters=int(counts[1]) if ok else None,
                   largest_cluster=int(counts[2]) if ok else None, solid_fraction=counts[0] / len(z[s]) if ok else None,
                   Q=acc["series_order"][s, 0, 0].copy() if ok else None, mean_qbar=acc["series_order"][s, 0, 1].copy() if ok else None)
        out.append(res)
    return out
