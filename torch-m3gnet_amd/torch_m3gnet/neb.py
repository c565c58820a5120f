"""Batched climbing-image nudged elastic band on the device: minimum-energy paths and barriers (C ABI: m3g_neb_*, csrc/m3g_neb.hip,
driven by m3g_fire_*).

The usual way to run a NEB with an M3GNet potential is ASE's `NEB(images, k, climb, method="improvedtangent")` under ASE's `FIRE`:
one host round trip per image per iteration, the images evaluated one at a time.  `NEB.run` takes a batch of bands instead.  The
interior images of every band are one `VerletGraph` batch; per iteration the energies and forces of all of them come from
`VerletGraph.step`, the NEB projection of the whole batch is three kernel launches (`neb_forces`) and the optimiser is the existing
device FIRE (`fire_step`, cell fixed) with one "structure" per band covering all of its interior atoms -- which is exactly ASE's FIRE
over the NEB optimizable: one dt and velocity per band, the `maxstep` clip over the norm of the whole band, converged when the
largest NEB-force row of the band's interior images is below `fmax`.  A converged band is frozen while the others go on; a band
whose projection meets a non-finite value is flagged as an error and frozen where it stands.

Semantics (include/m3gnet_hip.h, "batched nudged elastic band"): ASE's improved tangent and improved parallel spring with one k per
band; the climbing image is the interior image of highest energy, re-chosen at every iteration, the LOWEST index on ties (ASE takes the
last entry of an argsort).  Positions are never wrapped during a run: build the final image as the minimum image of the initial one
(`interpolate(..., mic=True)` does), so plain differences are minimum-image differences."""
from __future__ import annotations

from typing import Sequence

import numpy as np
import torch

from . import _cuda, _lib
from ._driver import Driver, boolean, check_tensor, integer, positive, state_tensor, structure_arrays
from .data import MaterialGraphKey as K
from .data.graph_gpu import _ptr, _stream
from .data.md import VerletGraph
from .nn.modules import Gradient
from .relax import FireState, _relax, fire_loop


def interpolate(lattice, initial_pos, final_pos, n_images: int, mic: bool = True) -> list:
    """`n_images` (M >= 3, endpoints included) position arrays [n, 3] on the straight line from `initial_pos` to `final_pos`.  mic:
    every atom of the final image is first moved to its periodic image nearest to the atom's initial position (fractional
    differences rounded to the nearest integer), so that the path never crosses the cell."""
    m = integer("n_images (endpoints included)", n_images, 3)
    L = np.asarray(lattice, dtype=np.float64).reshape(3, 3)
    p0 = np.asarray(initial_pos, dtype=np.float64)
    p1 = np.asarray(final_pos, dtype=np.float64)
    if p0.ndim != 2 or p0.shape[1] != 3 or p0.shape != p1.shape:
        raise ValueError(f"initial_pos and final_pos must both be [n, 3]; got {p0.shape} and {p1.shape}")
    d = p1 - p0
    if mic:
        frac = np.linalg.solve(L.T, d.T).T
        d = (frac - np.round(frac)) @ L
    return [p0 + (j / (m - 1)) * d for j in range(m)]


class NEBState:
    """NEB projection of a batch of bands on the device (m3g_neb_init).  `image_offsets`: I + 1 atom offsets of the interior images
    (the rows of the `pos` given to `neb_forces`); `band_images`: B + 1 offsets of every band's interior images, in path order; `k`,
    `climb`: one value or one per band; `endpoint_pos` [2 sum_b n_b, 3] float64 on the device (per band: its initial image rows, then
    its final image rows); `endpoint_energies` [B, 2] (initial, final).  `neb_forces` writes `forces` [N,3] float32 (the forces FIRE
    takes) and `rows` [I, 5] float64: |tau+|, |tau-|, F.tau_hat, spring term (0 at the climbing image), climbing flag."""

    def __init__(self, image_offsets: Sequence[int], band_images: Sequence[int], k, climb, endpoint_pos: torch.Tensor, endpoint_energies):
        self.image_offsets = np.ascontiguousarray(np.asarray(image_offsets, dtype=np.int64))
        self.band_images = np.ascontiguousarray(np.asarray(band_images, dtype=np.int32))
        self.I, self.B = len(self.image_offsets) - 1, len(self.band_images) - 1
        if self.I < 1 or self.B < 1:
            raise ValueError("image_offsets and band_images must hold at least two entries each")
        self.N = int(self.image_offsets[-1])
        self.k = np.ascontiguousarray(np.broadcast_to(np.asarray(k, dtype=np.float64), (self.B,)))
        climb = np.broadcast_to(np.asarray(climb), (self.B,))
        self.climb = np.ascontiguousarray(climb.astype(np.int32))
        self.endpoint_energies = np.ascontiguousarray(np.asarray(endpoint_energies, dtype=np.float64).reshape(-1))
        if len(self.endpoint_energies) != 2 * self.B:
            raise ValueError(f"expected {2 * self.B} endpoint energies (initial, final per band)")
        check_tensor("endpoint_pos", endpoint_pos, ("rows", 3), torch.float64)
        sizes = np.diff(self.image_offsets)[np.clip(self.band_images[:-1], 0, self.I - 1)]
        if endpoint_pos.size(0) != 2 * int(sizes.sum()):
            raise ValueError(f"endpoint_pos must hold {2 * int(sizes.sum())} rows (initial and final image of every band)")
        self.device = endpoint_pos.device
        self.lib = _lib.load_library()
        self.state = state_tensor(self.lib.m3g_neb_state_bytes, self.N, self.I, self.B, device=self.device)
        self.forces = torch.zeros(self.N, 3, dtype=torch.float32, device=self.device)
        self.rows = torch.full((self.I, _lib.NEB_ROWS), float("nan"), dtype=torch.float64, device=self.device)
        with _cuda.on_device(self.device):
            _lib.check(self.lib.m3g_neb_init(self.N, self.I, self.B, self.image_offsets.ctypes.data, self.band_images.ctypes.data,
                                             self.k.ctypes.data, self.climb.ctypes.data, _ptr(endpoint_pos), self.endpoint_energies.ctypes.data,
                                             _ptr(self.state), self.state.numel(), _stream()))

    @property
    def band_offsets(self) -> np.ndarray:
        """B + 1 atom offsets of the bands' interior atoms: the FIRE partition of the NEB optimiser."""
        return self.image_offsets[self.band_images]


def neb_forces(state: NEBState, pos: torch.Tensor, energies: torch.Tensor, forces: torch.Tensor) -> torch.Tensor:
    """NEB forces of every interior image (m3g_neb_forces) at `pos` [N,3] float64 from `energies` [I] and `forces` [N,3] (float32,
    evaluated at `pos`): written to and returned as `state.forces`; `state.rows` gets the per-image observables.  Queued on the
    current stream; no wait, capture-safe."""
    check_tensor("pos", pos, (state.N, 3), torch.float64)
    check_tensor("energies", energies, (state.I,), torch.float32)
    check_tensor("forces", forces, (state.N, 3), torch.float32)
    with _cuda.on_device(state.device):
        _lib.check(state.lib.m3g_neb_forces(state.N, state.I, state.B, _ptr(state.state), state.state.numel(), _ptr(pos), _ptr(energies),
                                            _ptr(forces), _ptr(state.forces), _ptr(state.rows), _stream()))
    return state.forces


class NEB(Driver):
    """Batched climbing-image NEB (improved tangent) under device FIRE.

    `model`: the `Gradient` returned by `build_model` (evaluated, like `Relaxer`'s, through a pair-virial engine made from its
    `Sequential`).  `k`: spring constant in eV/A^2 (ASE's default 0.1); `climb`: climbing image on (default) or off."""

    def __init__(self, model: Gradient, k: float = 0.1, climb: bool = True, skin: float = 0.5, device="cuda"):
        super().__init__(model, skin, device)
        self.k, self.climb = positive("k", k), boolean("climb", climb)

    @staticmethod
    def _bands(bands):
        if len(bands) == 0:
            raise ValueError("bands must hold at least one band")
        out = []
        for b, band in enumerate(bands):
            if len(band) != 3:
                raise ValueError(f"band {b}: expected (lattice, atomic_numbers, images)")
            lattice, z, images = band
            if len(images) < 3:
                raise ValueError(f"band {b}: a band needs at least 3 images (both endpoints and one interior image); got {len(images)}")
            lat, pos, zs = structure_arrays([lattice] * len(images), list(images), [z] * len(images))
            out.append((lat[0], zs[0], pos))
        return out

    def run(self, bands: Sequence, fmax: float = 0.05, steps: int = 500, relax_endpoints: bool = False, endpoint_fmax: float | None = None,
            endpoint_steps: int = 500) -> list:
        """Optimise every band (lattice [3,3] rows = lattice vectors, atomic_numbers [n], images: M >= 3 position arrays [n,3] in path
        order, endpoints included) until the largest NEB-force row of its interior images is below `fmax` or `steps` FIRE steps.
        The endpoints are evaluated once; with `relax_endpoints` they are first relaxed (as `Relaxer(relax_cell=False)` does, to
        `endpoint_fmax`, default `fmax`) and every interior image j of M is shifted by (1 - t) dR_0 + t dR_M-1, t = j / (M-1), with
        dR the endpoints' displacements (a straight band stays the straight band between the relaxed endpoints).
        Returns one dict per band: positions [M,n,3], energies [M], forces and neb_forces [M-2,n,3] (true and NEB forces of the
        interior images at the final positions), climbing_image (index in 0..M-1, None without climb), barrier_forward (E_max - E_0),
        barrier_backward (E_max - E_M-1), n_steps, converged, error (its projection met a non-finite value: stopped where it stood)."""
        fmax = positive("fmax", fmax)
        steps, endpoint_steps = integer("steps", steps, 0), integer("endpoint_steps", endpoint_steps, 0)
        efmax = fmax if endpoint_fmax is None else positive("endpoint_fmax", endpoint_fmax)
        bands = self._bands(bands)
        B = len(bands)
        model, dev = self.model, self.device
        cfg = model.engine.cfg
        ep_lat = [lat for lat, _, _ in bands for _ in range(2)]
        ep_z = [z for _, z, _ in bands for _ in range(2)]
        ep_pos = [p for _, _, imgs in bands for p in (imgs[0], imgs[-1])]
        if relax_endpoints:
            res = _relax(model, ep_lat, ep_pos, ep_z, relax_cell=False, fmax=efmax, steps=endpoint_steps, skin=self.skin, device=dev)
            new_pos = [r["positions"] for r in res]
            ep_e = np.array([r["total_energy"] for r in res])
            for b, (_, _, imgs) in enumerate(bands):
                d0, d1 = new_pos[2 * b] - imgs[0], new_pos[2 * b + 1] - imgs[-1]
                m = len(imgs)
                imgs[:] = [imgs[j] + (1.0 - j / (m - 1)) * d0 + (j / (m - 1)) * d1 for j in range(m)]
                imgs[0], imgs[-1] = new_pos[2 * b], new_pos[2 * b + 1]
        else:
            vg_e = VerletGraph(ep_lat, ep_z, cfg.cutoff, cfg.threebody_cutoff, skin=self.skin, device=dev)
            out = vg_e.step(model, torch.tensor(np.concatenate(ep_pos), dtype=torch.float64, device=vg_e.device))
            ep_e = out[K.TOTAL_ENERGY].double().cpu().numpy()
        # the interior images of every band: one batch
        img_lat = [lat for lat, _, imgs in bands for _ in imgs[1:-1]]
        img_z = [z for _, z, imgs in bands for _ in imgs[1:-1]]
        img_pos = [p for _, _, imgs in bands for p in imgs[1:-1]]
        vg = VerletGraph(img_lat, img_z, cfg.cutoff, cfg.threebody_cutoff, skin=self.skin, device=dev)
        pos_t = torch.tensor(np.concatenate(img_pos), dtype=torch.float64, device=vg.device)
        image_offsets = np.concatenate([[0], np.cumsum([len(z) for z in img_z])])
        band_images = np.concatenate([[0], np.cumsum([len(imgs) - 2 for _, _, imgs in bands])])
        ep_t = torch.tensor(np.concatenate([p for _, _, imgs in bands for p in (imgs[0], imgs[-1])]), dtype=torch.float64, device=vg.device)
        neb = NEBState(image_offsets, band_images, self.k, self.climb, ep_t, ep_e.reshape(B, 2))
        fire = FireState(pos_t, None, neb.band_offsets, relax_cell=False, fmax=fmax)
        # (when the loop leaves early nothing moved at the last launch: `out` and the NEB forces belong to the final positions)
        out = fire_loop(vg, model, fire, steps, project=lambda out: neb_forces(neb, pos_t, out[K.TOTAL_ENERGY], out[K.FORCES]))
        vg.raise_on_step_errors("NEB")
        st = fire.read()
        e, f = (out[key].double().cpu().numpy() for key in (K.TOTAL_ENERGY, K.FORCES))
        p_host, nf, rows = pos_t.cpu().numpy(), neb.forces.double().cpu().numpy(), neb.rows.cpu().numpy()
        res = []
        for b, (_, z, imgs) in enumerate(bands):
            i0, i1 = int(band_images[b]), int(band_images[b + 1])
            a, c = int(image_offsets[i0]), int(image_offsets[i1])
            n = len(z)
            inner = p_host[a:c].reshape(i1 - i0, n, 3)
            energies = np.concatenate([[ep_e[2 * b]], e[i0:i1], [ep_e[2 * b + 1]]])
            climbing = np.flatnonzero(rows[i0:i1, 4] == 1.0)
            e_max = float(energies.max())
            res.append({"positions": np.concatenate([imgs[0][None], inner, imgs[-1][None]]), "energies": energies,
                        "forces": f[a:c].reshape(i1 - i0, n, 3), "neb_forces": nf[a:c].reshape(i1 - i0, n, 3),
                        "climbing_image": int(climbing[0]) + 1 if len(climbing) else None,
                        "barrier_forward": e_max - float(energies[0]), "barrier_backward": e_max - float(energies[-1]),
                        "n_steps": int(st["n_steps"][b]), "converged": bool(st["flags"][b] & _lib.FIRE_CONVERGED),
                        "error": bool(st["flags"][b] & _lib.FIRE_ERROR)})
        return res
