"""Normal-mode analysis of molecular dynamics on the device (C ABI: m3g_nma_*, csrc/m3g_nma.hip): the anharmonic frequency and the
lifetime of every phonon mode at temperature T, from an MD supercell projected on the harmonic eigenvectors of `phonons` at the
commensurate q-points (Ladd, Moran and Hoover, Phys. Rev. B 34, 5058 (1986); McGaughey and Kaviany, Phys. Rev. B 69, 094303 (2004);
the spectral energy density of Thomas et al., Phys. Rev. B 81, 081411 (2010)).

Structure s: a unit cell of n_u atoms, a diagonal MD supercell (c1, c2, c3) in the order of `PhononState` (atom j = l n_u + b,
l = (l1 c2 + l2) c3 + l3, N_c cells), q-points in fractional reciprocal coordinates of the unit cell and eigenvectors E[q]
[3 n_u, 3 n_u] as `PhononResult.modes` returns them (column nu the mode, rows 3b .. 3b + 2 atom b; phonopy's convention).  With f_j the
fractional coordinate of the equilibrium site of atom j in unit-cell units:
    Qdot[q,nu] = N_c^(-1/2) sum_j sqrt(m_j) exp(-2 pi i q.f_j) sum_a conj(E[q][3b+a, nu]) v[j,a]
    Q   [q,nu] = the same with u_j = r_j - r0_j - (mass-weighted mean of r - r0) in place of v
The device accumulates, per mode, sum |Qdot|^2, sum |Q|^2 and acf[lag] = sum_t conj(Qdot(t - lag)) Qdot(t) over a ring of the last
n_lags samples, and per structure sum_t sum_j m_j |v_j|^2 -- no frame goes to the host and no 3N x 3N projector is formed.  On the
host (numpy): a mode's kinetic temperature <|Qdot|^2> / (kappa kB), its effective frequency sqrt(<|Qdot|^2> / <|Q|^2>) / 2 pi, and
from Re C(t) / C(0) ~ exp(-Gamma t) cos(omega t) its frequency, linewidth Gamma and lifetime tau = 1 / (2 Gamma) (the decay time of
the mode's energy); then kappa_RTA = (1/V) sum kB v_g v_g tau with the group velocities of `phonons`.

Limits: diagonal supercells; 3 n_u <= `_lib.NMA_MAX_N` (E[q] lives in LDS); classical statistics in kappa_RTA (every mode carries
kB: right for classical MD, too much heat capacity below the Debye temperature).

Units as in `dynamics`: A, fs, amu, eV, K; frequencies in THz."""
from __future__ import annotations

import ctypes as C
import math
from typing import Sequence

import numpy as np
import torch

from . import _cuda, _lib
from ._driver import (Driver, MdBatch, MdLog, boolean, check_tensor, integer, md_loop, md_results, non_negative, positive, read_state,
                      state_tensor, structure_seeds)
from .data import MaterialGraphKey as K
from .data.graph_gpu import _ptr, _stream
from .dynamics import KAPPA, KB, DynState, langevin_warm_up
from .nn.modules import Gradient
from .phonons import _check_supercells

KB_THZ2_A2_FS_PER_A3_IN_W_PER_M_K = 1.380649e-23 * 1e4 * 1e-15 / 1e-30   # kB (J/K) (THz A)^2 fs / A^3 in W / (m K): 1.380649e-4
PRODUCTION = ("nve", "nvt_langevin")


def commensurate_qpoints(supercell) -> np.ndarray:
    """All (i / c1, j / c2, k / c3), 0 <= i < c1 ..., [c1 c2 c3, 3], k fastest: the q-points an MD supercell (c1, c2, c3) carries."""
    c = _check_supercells(supercell, 1)[0]
    grid = np.stack(np.meshgrid(*(np.arange(n) for n in c), indexing="ij"), axis=-1).reshape(-1, 3)
    return grid / c.astype(np.float64)


class NmaState:
    """Normal-mode accumulators of a batch on the device (m3g_nma_init).  One entry per structure: `lattices` [3,3] (the UNIT cell,
    rows = lattice vectors), `frac` [n_u,3] (fractional coordinates of the unit cell's atoms), `masses` [n_u] (amu), `supercells`
    [S,3] or one [3] (the MD supercell), `qpoints` [Q_s,3], `eigenvectors` [Q_s, 3 n_u, 3 n_u] complex.  The batch's atoms are the
    supercells one after another in the order of the module docstring (`offsets`).  `n_lags` = 0 switches the autocorrelation off;
    its ring and sums take 2 x n_lags x n_modes x 16 bytes.  Everything is checked before the first device call."""

    def __init__(self, lattices: Sequence, frac: Sequence, masses: Sequence, supercells, qpoints: Sequence, eigenvectors: Sequence,
                 n_lags: int = 0, remove_com: bool = True, device="cuda"):
        self.S = len(lattices)
        if not (len(frac) == len(masses) == len(qpoints) == len(eigenvectors) == self.S) or self.S == 0:
            raise ValueError("lattices, frac, masses, qpoints and eigenvectors must hold one entry per structure (at least one)")
        self.lags = integer("n_lags", n_lags, 0)
        if self.lags > _lib.NMA_MAX_LAGS:
            raise ValueError(f"n_lags must be at most {_lib.NMA_MAX_LAGS}; got {n_lags}")
        self.remove_com = boolean("remove_com", remove_com)
        self.supercells = _check_supercells(supercells, self.S)
        lat, fr, ms, qs, es = [], [], [], [], []
        for s in range(self.S):
            L, f = np.asarray(lattices[s], dtype=np.float64), np.asarray(frac[s], dtype=np.float64)
            m, q, e = np.asarray(masses[s], dtype=np.float64).reshape(-1), np.asarray(qpoints[s], dtype=np.float64), np.asarray(eigenvectors[s])
            if L.shape != (3, 3) or not np.isfinite(L).all() or abs(np.linalg.det(L)) < 1e-12:
                raise ValueError(f"structure {s}: lattice must be a finite, non-singular [3, 3]")
            if f.ndim != 2 or f.shape[1] != 3 or len(f) == 0 or len(m) != len(f) or not np.isfinite(f).all():
                raise ValueError(f"structure {s}: frac must be a finite [n_u, 3] with one mass per atom; got {f.shape} and {len(m)} masses")
            n3 = 3 * len(f)
            if n3 > _lib.NMA_MAX_N:
                raise ValueError(f"structure {s}: 3 n_u = {n3} is above {_lib.NMA_MAX_N} (_lib.NMA_MAX_N)")
            if not (np.isfinite(m).all() and (m > 0).all()):
                raise ValueError(f"structure {s}: masses must be finite and > 0")
            if q.ndim != 2 or q.shape[1] != 3 or len(q) == 0 or not np.isfinite(q).all():
                raise ValueError(f"structure {s}: qpoints must be a finite [Q, 3] with Q >= 1; got {q.shape}")
            if e.shape != (len(q), n3, n3):
                raise ValueError(f"structure {s}: eigenvectors must be [{len(q)}, {n3}, {n3}]; got {e.shape}")
            e = e.astype(np.complex128)
            if not np.isfinite(e).all():
                raise ValueError(f"structure {s}: non-finite eigenvectors")
            lat.append(L), fr.append(f), ms.append(m), qs.append(q), es.append(e)
        self.n_unit = np.array([len(f) for f in fr], dtype=np.int64)
        self.n_q = np.array([len(q) for q in qs], dtype=np.int64)
        cells = self.supercells.astype(np.int64).prod(axis=1)
        self.unit_offsets = np.ascontiguousarray(np.concatenate([[0], np.cumsum(self.n_unit)]).astype(np.int64))
        self.q_offsets = np.ascontiguousarray(np.concatenate([[0], np.cumsum(self.n_q)]).astype(np.int64))
        self.offsets = np.concatenate([[0], np.cumsum(self.n_unit * cells)]).astype(np.int64)
        self.mode_offsets = np.concatenate([[0], np.cumsum(self.n_q * 3 * self.n_unit)]).astype(np.int64)
        self.N, self.M = int(self.offsets[-1]), int(self.mode_offsets[-1])
        self.lattices = np.ascontiguousarray(np.stack(lat))
        self.frac, self.masses = np.ascontiguousarray(np.concatenate(fr)), np.ascontiguousarray(np.concatenate(ms))
        self.qpoints = np.ascontiguousarray(np.concatenate(qs))
        self.eigenvectors = np.ascontiguousarray(np.concatenate([e.reshape(-1) for e in es]))
        self.sizes = _lib.M3GNmaSizes(self.N, self.S, int(self.unit_offsets[-1]), int(self.q_offsets[-1]), self.M, len(self.eigenvectors),
                                      int((self.n_q * self.n_unit * cells).sum()), int(3 * self.n_unit.max()), self.lags)
        self.params = _lib.M3GNmaParams(1 if self.remove_com else 0, 0)
        self.device = torch.device(device)
        self.lib = _lib.load_library()
        self.state = state_tensor(self.lib.m3g_nma_state_bytes, C.byref(self.sizes), device=self.device)
        with _cuda.on_device(self.device):
            _lib.check(self.lib.m3g_nma_init(C.byref(self.sizes), C.byref(self.params), self.unit_offsets.ctypes.data,
                                             self.supercells.ctypes.data, self.lattices.ctypes.data, self.frac.ctypes.data,
                                             self.masses.ctypes.data, self.q_offsets.ctypes.data, self.qpoints.ctypes.data,
                                             self.eigenvectors.ctypes.data, _ptr(self.state), self.state.numel(), _stream()))

    def read(self) -> dict:
        """The raw accumulators, copied to the host (waits for the stream): n_samples [S], kinetic_sum [S], qdot2_sum / q2_sum
        [n_modes], acf [n_modes, n_lags] complex (sums: not yet divided by lag_count), lag_count [S, n_lags], flags [S].  Modes run
        structure after structure, q after q, nu fastest (`mode_offsets`; `of_structure` cuts one structure out)."""
        S, M, G = self.S, self.M, self.lags
        return read_state(self.lib.m3g_nma_read, (C.byref(self.sizes),), self.state,
                          (("n_samples", np.int64, S), ("kinetic_sum", np.float64, S), ("qdot2_sum", np.float64, M), ("q2_sum", np.float64, M),
                           ("acf", np.complex128, (M, G)), ("lag_count", np.int64, (S, G)), ("flags", np.int32, S)))

    def frame(self):
        """(Qdot, Q) [n_modes] complex of the last sample every structure accumulated, copied to the host (waits for the stream)."""
        qdot, q = np.empty(self.M, dtype=np.complex128), np.empty(self.M, dtype=np.complex128)
        with _cuda.on_device(self.device):
            _lib.check(self.lib.m3g_nma_frame(C.byref(self.sizes), _ptr(self.state), self.state.numel(), qdot.ctypes.data, q.ctypes.data,
                                              _stream()))
        return qdot, q

    def of_structure(self, read: dict, s: int) -> dict:
        """Structure `s` of a `read()`: the per-mode arrays as [Q_s, 3 n_u] (acf [Q_s, 3 n_u, n_lags]), the others as scalars / [n_lags]."""
        a, b, shape = int(self.mode_offsets[s]), int(self.mode_offsets[s + 1]), (int(self.n_q[s]), 3 * int(self.n_unit[s]))
        return {"n_samples": int(read["n_samples"][s]), "kinetic_sum": float(read["kinetic_sum"][s]), "flags": int(read["flags"][s]),
                "qdot2_sum": read["qdot2_sum"][a:b].reshape(shape), "q2_sum": read["q2_sum"][a:b].reshape(shape),
                "acf": read["acf"][a:b].reshape(shape + (self.lags,)), "lag_count": read["lag_count"][s].copy()}


def nma_sample(state: NmaState, pos: torch.Tensor, vel: torch.Tensor, forces: torch.Tensor | None = None, kick: float = 0.0) -> None:
    """One sample of the batch (m3g_nma_sample): `pos` [N,3] fp64 (unwrapped), `vel` [N,3] fp64.  With `forces` [N,3] float32 the
    projected velocity is vel + kick * kappa * forces / m, as in `traj_sample`: give the integrator's velocities
    (`DynState.velocities`) and the forces of `pos` BEFORE the `dyn_step` of the same forces, with kick = timestep / 2 (0 before the
    first step).  Three launches queued on the current stream; no wait, capture-safe."""
    check_tensor("pos", pos, (state.N, 3), torch.float64)
    check_tensor("vel", vel, (state.N, 3), torch.float64)
    if forces is not None:
        check_tensor("forces", forces, (state.N, 3), torch.float32)
    with _cuda.on_device(state.device):
        _lib.check(state.lib.m3g_nma_sample(C.byref(state.sizes), C.byref(state.params), _ptr(state.state), state.state.numel(), _ptr(pos),
                                            _ptr(vel), _ptr(forces), float(kick), _stream()))


# ---- host post-processing (numpy) ------------------------------------------------------------------------------------------------------
def mode_statistics(read: dict, temperature: float | None = None) -> dict:
    """Per mode, from `qdot2_sum`, `q2_sum` (any shape) and `n_samples` of one structure: mode_temperatures (K) = <|Qdot|^2> / (kappa
    kB) -- every mode holds kB T of kinetic energy twice over in a classical run -- and effective_frequencies (THz) =
    sqrt(<|Qdot|^2> / <|Q|^2>) / 2 pi, the frequency of the harmonic oscillator with these two moments.  With `temperature` (K) also
    equipartition_frequencies = sqrt(kappa kB T / <|Q|^2>) / 2 pi, which needs no velocities.  Modes that never moved give NaN."""
    n = float(read["n_samples"])
    qd2, q2 = np.asarray(read["qdot2_sum"], dtype=np.float64), np.asarray(read["q2_sum"], dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = {"mode_temperatures": qd2 / n / (KAPPA * KB), "effective_frequencies": np.sqrt(qd2 / q2) / (2.0 * np.pi) * 1e3}
        if temperature is not None:
            out["equipartition_frequencies"] = np.sqrt(KAPPA * KB * positive("temperature", temperature) * n / q2) / (2.0 * np.pi) * 1e3
    return out


def spectral_energy_density(acf, dt: float) -> dict:
    """The windowed cosine transform of a mode-velocity autocorrelation C(t) (last axis: lags, `dt` fs apart), as
    `correlations_from_sums` forms the vibrational density of states: sed[k] = 2 int_0^T Re C(t) w(t) cos(2 pi f_k t) dt with
    w = (1 + cos(pi t / T)) / 2 (Hann), T the longest lag, f_k = k / (2 n_lags dt) -- `frequency` in THz.  A Lorentzian at the mode's
    frequency whose half width at half maximum is Gamma / 2 pi, broadened by the window."""
    c = np.real(np.asarray(acf))
    G = c.shape[-1]
    time = np.arange(G) * float(dt)
    freq = np.arange(G) / (2.0 * G * dt)
    window = 0.5 * (1.0 + np.cos(np.pi * time / time[-1])) if G > 1 else np.ones(1)
    kernel = np.cos(2.0 * np.pi * freq[:, None] * time[None, :])
    y = (c * window)[..., None, :] * kernel
    sed = 2.0 * (0.5 * (y[..., 1:] + y[..., :-1]) * np.diff(time)).sum(axis=-1) if G > 1 else np.zeros(c.shape[:-1] + (1,))
    return {"frequency": freq * 1e3, "sed": sed}


def _damped(t, gamma, omega):
    return np.exp(-gamma * t) * np.cos(omega * t)


def fit_damped_cosine(acf, dt: float, frequency: float | None = None, max_iterations: int = 200) -> dict:
    """Least-squares fit of y(t) = Re C(t) / C(0) to exp(-Gamma t) cos(omega t); `acf`: C at the lags 0, dt, 2 dt, ... (fs; already
    divided by lag_count).  Gauss-Newton on (Gamma, omega) with step halving, started at `frequency` (THz: the harmonic one), or at
    the peak of `spectral_energy_density` when None: omega is first moved to the best of a grid over +-20 % of the start, finer than
    the window resolves, and Gamma to the best of a logarithmic grid, so a start 10 % off lands in the right basin.  Returns
    frequency (THz), linewidth (Gamma, 1/fs: the decay rate of the mode's amplitude, the half width at half maximum of its spectral
    line in rad/fs), lifetime tau = 1 / (2 Gamma) (fs: the decay time of the mode's energy), residual (root mean square of the misfit
    of y), iterations and converged.  An autocorrelation that is not finite, has C(0) <= 0 or fewer than 4 lags gives NaN."""
    c = np.real(np.asarray(acf)).astype(np.float64).reshape(-1)
    nan = {"frequency": math.nan, "linewidth": math.nan, "lifetime": math.nan, "residual": math.nan, "iterations": 0, "converged": False}
    n = len(c)
    if n < 4 or not np.isfinite(c).all() or not c[0] > 0.0:
        return nan
    dt = positive("dt", dt)
    y, t = c / c[0], np.arange(n) * dt
    span = t[-1]
    if frequency is None or not (math.isfinite(frequency) and frequency > 0.0):
        sed = spectral_energy_density(y, dt)
        frequency = float(sed["frequency"][1 + int(np.argmax(sed["sed"][1:]))])
    w0 = 2.0 * np.pi * frequency * 1e-3
    # the basin of omega is about pi / span wide: scan at an eighth of that with the Hann-windowed transform, which a decay does not move
    grid = np.arange(0.8 * w0, 1.2 * w0 + 1e-300, np.pi / (8.0 * span))
    window = 0.5 * (1.0 + np.cos(np.pi * t / span))
    omega = float(grid[int(np.argmax(np.cos(grid[:, None] * t[None, :]) @ (y * window)))])
    gammas = 10.0 ** np.linspace(-4.0, 1.5, 45) / span
    miss = [np.sum((_damped(t, g, omega) - y) ** 2) for g in gammas]
    gamma = float(gammas[int(np.argmin(miss))])
    cost = float(np.sum((_damped(t, gamma, omega) - y) ** 2))
    converged, it = False, 0
    for it in range(1, max_iterations + 1):
        e, co, si = np.exp(-gamma * t), np.cos(omega * t), np.sin(omega * t)
        r = e * co - y
        J = np.stack([-t * e * co, -t * e * si], axis=1)
        step, *_ = np.linalg.lstsq(J, -r, rcond=None)
        scale = 1.0
        while scale > 1e-10:
            g_new, w_new = gamma + scale * step[0], omega + scale * step[1]
            c_new = float(np.sum((_damped(t, g_new, w_new) - y) ** 2)) if w_new > 0.0 else math.inf
            if c_new <= cost:
                break
            scale *= 0.5
        else:
            converged = True   # no shorter step lowers the misfit: at the minimum to rounding
            break
        moved = max(abs(g_new - gamma) / max(abs(g_new), 1e-300), abs(w_new - omega) / abs(w_new))
        gamma, omega, cost = g_new, w_new, c_new
        if moved < 1e-14:
            converged = True
            break
    with np.errstate(divide="ignore"):
        lifetime = 1.0 / (2.0 * gamma) if gamma > 0.0 else math.nan
    return {"frequency": omega / (2.0 * np.pi) * 1e3, "linewidth": gamma, "lifetime": lifetime, "residual": math.sqrt(cost / n),
            "iterations": it, "converged": converged}


def kappa_rta(volume: float, group_velocities, lifetimes, weights=None, frequencies=None, cutoff_frequency: float = 0.0):
    """The classical relaxation-time thermal conductivity (3 x 3, W / (m K)) = (1 / V) sum_modes w kB v (x) v tau, and the number of
    modes left out.  `volume` (A^3), `group_velocities` [..., 3] (THz A, as `PhononResult.group_velocities`), `lifetimes` [...] (fs),
    `weights` [...] (broadcast; default 1: then V is the volume of the MD supercell whose commensurate q-points are summed; with
    q-weights that sum to 1, the unit cell's).  Modes with a non-finite or non-positive lifetime, a non-finite velocity, or (given
    `frequencies`, THz) a frequency below `cutoff_frequency` are left out and counted.  Classical: every mode carries kB."""
    v = np.asarray(group_velocities, dtype=np.float64)
    tau = np.asarray(lifetimes, dtype=np.float64)
    if v.shape != tau.shape + (3,):
        raise ValueError(f"group_velocities must be lifetimes' shape + (3,); got {v.shape} and {tau.shape}")
    w = np.broadcast_to(np.ones(()) if weights is None else np.asarray(weights, dtype=np.float64), tau.shape)
    keep = np.isfinite(tau) & (tau > 0.0) & np.isfinite(v).all(axis=-1) & np.isfinite(w)
    if frequencies is not None:
        f = np.asarray(frequencies, dtype=np.float64)
        keep &= np.isfinite(f) & (f >= cutoff_frequency)
    vk, tk, wk = v[keep], tau[keep], w[keep]
    kappa = np.einsum("m,ma,mb->ab", wk * tk, vk, vk) * KB_THZ2_A2_FS_PER_A3_IN_W_PER_M_K / positive("volume", volume)
    return kappa, int(keep.size - keep.sum())


def exact_translations(qpoints, eigenvectors, frac, masses, least_overlap: float = 0.99) -> np.ndarray:
    """`eigenvectors` [Q, 3 n_u, 3 n_u] with the acoustic modes at every q that is a reciprocal lattice vector G (all components
    integers; Gamma) made exact.  There the three uniform translations t_a[3b + a'] = sqrt(m_b / M) exp(-2 pi i G.f_b) delta_aa' are
    null vectors of any translation-invariant dynamical matrix, but the eigenvectors of a matrix built from finite-difference fp32
    forces carry an admixture of the other modes at the level of its acoustic-sum-rule noise (1e-6), through which the centre-of-mass
    motion would leak into them and theirs into it.  The three columns that overlap most with the translations are replaced by the
    translations (in the combination closest to those columns), the other columns have the translations projected out and are made
    orthonormal again by the symmetric (Loewdin) transformation, which moves them least.  A q whose three best columns overlap
    with the translations by less than `least_overlap` each (a matrix without the sum rule) is left as it is."""
    q, e = np.asarray(qpoints, dtype=np.float64).reshape(-1, 3), np.array(eigenvectors, dtype=np.complex128)
    f, m = np.asarray(frac, dtype=np.float64), np.asarray(masses, dtype=np.float64)
    for i in np.flatnonzero(np.abs(q - np.rint(q)).max(axis=1) == 0.0):
        t = np.zeros((3 * len(m), 3), dtype=np.complex128)
        for a in range(3):
            t[a::3, a] = np.sqrt(m / m.sum()) * np.exp(-2j * np.pi * (f @ q[i]))
        overlap = (np.abs(t.conj().T @ e[i]) ** 2).sum(axis=0)
        acoustic = np.sort(np.argsort(overlap)[-3:])
        if overlap[acoustic].min() < least_overlap:
            continue
        u, _, vh = np.linalg.svd(t.conj().T @ e[i][:, acoustic])   # the unitary closest to the overlap matrix
        e[i][:, acoustic] = t @ (u @ vh)
        rest = np.setdiff1d(np.arange(e.shape[2]), acoustic)
        if len(rest):
            x = e[i][:, rest] - t @ (t.conj().T @ e[i][:, rest])
            w, v = np.linalg.eigh(x.conj().T @ x)
            e[i][:, rest] = x @ (v / np.sqrt(w)[None, :]) @ v.conj().T
    return e


class NormalModeAnalysis(Driver):
    """Anharmonic phonon frequencies, linewidths and lifetimes of a batch of crystals by normal-mode decomposition of MD.

    `model`: the `Gradient` returned by `build_model`.  For every `PhononResult` the MD supercell is built in the order of the module
    docstring, equilibrated with the Langevin thermostat (BAOAB, `friction` in 1/fs) at `temperature` (K, one value) from
    Maxwell-Boltzmann velocities, and then run in `production` "nve" or "nvt_langevin" (the same friction); every `sample_interval`
    steps the trajectory is projected on the device, before the integrator call, on the eigenvectors `PhononResult.modes` returns,
    the acoustic modes at Gamma made the exact translations (`exact_translations`: with `remove_com` they then hold nothing)
    (`n_lags` samples of autocorrelation: the time window is n_lags * sample_interval * timestep, which should span several
    lifetimes; sample_interval * timestep must resolve the highest frequency, at least four samples per period).

    A Langevin production phase damps every mode velocity at the rate friction / 2 on top of the anharmonic decay: it ADDS
    friction / 2 to every linewidth returned (the `linewidths` and `lifetimes` here are as fitted, thermostat included) -- subtract
    it, or use "nve" where the model conserves energy over the run.  A harmonic crystal under Langevin has linewidth friction / 2.

    All structures share one engine batch (see `ReverseNEMD`): only the m3g_nma_* kernels are bitwise the same for a structure alone
    or in any batch, not the whole run.  Limits: diagonal supercells, 3 n_u <= `_lib.NMA_MAX_N`, classical statistics in the
    relaxation-time conductivity."""

    def __init__(self, model: Gradient, temperature: float = 300.0, timestep: float = 1.0, friction: float = 0.01,
                 production: str = "nve", n_lags: int = 200, sample_interval: int = 5, remove_com: bool = True, skin: float = 0.5,
                 seed=0, device="cuda"):
        super().__init__(model, skin, device)
        if production not in PRODUCTION:
            raise ValueError(f"unknown production ensemble {production!r}; expected one of {PRODUCTION}")
        self.production = production
        self.temperature = positive("temperature", temperature)
        self.timestep = positive("timestep", timestep)
        self.friction = non_negative("friction", friction)
        self.n_lags = integer("n_lags", n_lags, 0)
        if self.n_lags > _lib.NMA_MAX_LAGS:
            raise ValueError(f"n_lags must be at most {_lib.NMA_MAX_LAGS}; got {n_lags}")
        self.sample_interval = integer("sample_interval", sample_interval, 1)
        self.remove_com = boolean("remove_com", remove_com)
        self.seed = seed

    def run(self, phonon_results: Sequence, supercells, steps: int, equilibration: int = 0, qpoints: Sequence | None = None,
            loginterval: int = 10) -> list:
        """`phonon_results`: one `PhononResult` of `Phonons.run` per structure (unit cell, masses, atomic numbers and `modes`);
        `supercells` [S,3] or one [3]: the MD supercells; `qpoints`: per structure [Q,3] fractional q-points (default
        `commensurate_qpoints` of its MD supercell).  `equilibration` Langevin steps, then `steps` production steps sampled at every
        step k = 0, sample_interval, ... before the integrator call, the half-step velocities completed by the sampler itself.
        Returns one dict per structure: that of `MolecularDynamics.run` for the production phase, and qpoints [Q,3];
        harmonic_frequencies, effective_frequencies, fitted_frequencies (THz), linewidths (1/fs), lifetimes (fs), mode_temperatures
        (K), fit_residuals, each [Q, 3 n_u]; acf [Q, 3 n_u, n_lags] complex (divided by lag_count), lag_count [n_lags], kinetic_sum
        (amu A^2/fs^2), n_samples, nonfinite (a sample was refused: the structure stopped accumulating), sample_time (fs between
        two lags); and, where 3 n_u <= `_lib.PH_GV_MAX_N`, thermal_conductivity_rta [3,3] (W / (m K); `kappa_rta` over the q-points
        with equal weights, group velocities of `PhononResult.group_velocities`, modes below the result's cutoff frequency left out)
        with rta_modes_excluded."""
        steps, loginterval = integer("steps", steps, 0), integer("loginterval", loginterval, 1)
        equilibration = integer("equilibration", equilibration, 0)
        S = len(phonon_results)
        if S == 0:
            raise ValueError("phonon_results must hold at least one PhononResult")
        sc = _check_supercells(supercells, S)
        if qpoints is not None and len(qpoints) != S:
            raise ValueError("qpoints: expected one array per structure")
        lat_u, frac, m_u, z_u, qs, harmonic, eig = [], [], [], [], [], [], []
        for s, ph in enumerate(phonon_results):
            z = getattr(ph, "atomic_numbers", None)
            if z is None or getattr(ph, "positions", None) is None:
                raise ValueError(f"structure {s}: the PhononResult carries no positions and atomic_numbers (results of Phonons.run do)")
            if ph.error:
                raise ValueError(f"structure {s}: the PhononResult is flagged `error` (non-finite forces)")
            if 3 * ph.n_atoms > _lib.NMA_MAX_N:
                raise ValueError(f"structure {s}: 3 n_u = {3 * ph.n_atoms} is above {_lib.NMA_MAX_N} (_lib.NMA_MAX_N)")
            q = commensurate_qpoints(sc[s]) if qpoints is None else np.asarray(qpoints[s], dtype=np.float64)
            if q.ndim != 2 or q.shape[1] != 3 or len(q) == 0:
                raise ValueError(f"structure {s}: qpoints must be [Q, 3] with Q >= 1; got {q.shape}")
            lat_u.append(np.asarray(ph.lattice, dtype=np.float64))
            frac.append(np.asarray(ph.positions, dtype=np.float64) @ np.linalg.inv(lat_u[-1]))
            m_u.append(np.asarray(ph.masses, dtype=np.float64))
            z_u.append(np.asarray(z).reshape(-1))
            qs.append(q)
        for s, ph in enumerate(phonon_results):   # (device work from here on)
            modes = ph.modes(qs[s])
            harmonic.append(modes["frequencies"])
            eig.append(exact_translations(qs[s], modes["eigenvectors"], frac[s], m_u[s]))
        nma = NmaState(lat_u, frac, m_u, sc, qs, eig, self.n_lags, self.remove_com, device=self.device)
        lat, pos, z, m = [], [], [], []
        for s in range(S):   # the MD supercells: atom j = l n_u + b at (f_b + l) L
            c = sc[s].astype(np.int64)
            cell = np.stack(np.meshgrid(*(np.arange(n) for n in c), indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float64)
            lat.append(c[:, None] * lat_u[s])
            pos.append(((frac[s][None, :, :] + cell[:, None, :]).reshape(-1, 3)) @ lat_u[s])
            z.append(np.tile(z_u[s], len(cell)))
            m.append(np.tile(m_u[s], len(cell)))
        seeds = structure_seeds(self.seed, S)
        batch = MdBatch(self.model, lat, pos, z, [(0, S)], self.skin, self.device)
        common = dict(dt=self.timestep, friction=self.friction)
        warm = langevin_warm_up(batch, m, self.temperature, seeds, equilibration, **common)
        dyn = DynState(batch.pos, batch.lattice, batch.offsets, np.concatenate(m), warm.velocities, self.temperature,
                       seeds ^ np.uint64(0x9E3779B97F4A7C15), ensemble=self.production, **common)   # (other noise than the equilibration's)

        def sample(k, out, logged):
            if k % self.sample_interval == 0:
                nma_sample(nma, batch.pos, dyn.velocities, out[K.FORCES], 0.0 if k == 0 else 0.5 * self.timestep)

        log = MdLog()
        out = md_loop(batch, dyn, steps, before=sample, log=log.of(dyn), loginterval=loginterval)
        runs = md_results(batch, dyn, out, log, "normal-mode analysis")
        acc = nma.read()
        sample_time = self.sample_interval * self.timestep
        res = []
        for s, (ph, r) in enumerate(zip(phonon_results, runs)):
            mine = nma.of_structure(acc, s)
            stats = mode_statistics(mine)
            with np.errstate(divide="ignore", invalid="ignore"):
                acf = mine["acf"] / mine["lag_count"].astype(np.float64)
            shape = harmonic[s].shape
            fits = {key: np.full(shape, np.nan) for key in ("frequency", "linewidth", "lifetime", "residual")}
            if self.n_lags >= 4 and (mine["lag_count"] > 0).all():
                for iq in range(shape[0]):
                    for nu in range(shape[1]):
                        start = float(harmonic[s][iq, nu])
                        fit = fit_damped_cosine(acf[iq, nu], sample_time, start if start > ph.cutoff_frequency else None)
                        for key in fits:
                            fits[key][iq, nu] = fit[key]
            r.update(qpoints=qs[s].copy(), harmonic_frequencies=harmonic[s], effective_frequencies=stats["effective_frequencies"],
                     fitted_frequencies=fits["frequency"], linewidths=fits["linewidth"], lifetimes=fits["lifetime"],
                     fit_residuals=fits["residual"], mode_temperatures=stats["mode_temperatures"], acf=acf, lag_count=mine["lag_count"],
                     kinetic_sum=mine["kinetic_sum"], n_samples=mine["n_samples"], nonfinite=bool(mine["flags"] & _lib.NMA_NONFINITE),
                     sample_time=sample_time)
            if shape[1] <= _lib.PH_GV_MAX_N:
                gv = ph.group_velocities(qs[s])
                kappa, left_out = kappa_rta(abs(float(np.linalg.det(lat_u[s]))), gv, fits["lifetime"], 1.0 / shape[0], harmonic[s],
                                            ph.cutoff_frequency)
                r.update(thermal_conductivity_rta=kappa, rta_modes_excluded=left_out)
            res.append(r)
        return res
