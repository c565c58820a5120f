"""Numpy / plain-Python fp64 restatement of reverse non-equilibrium MD (torch_m3gnet.transport, C ABI m3g_rnemd_*,
csrc/m3g_rnemd.hip), one structure at a time: the yardstick of tests/test_gpu_rnemd.py.  Every rounding of the device is repeated in
its order -- no product is fused with a sum, the slab sums run over 64 consecutive rows in row order, then over the four such runs of
a chunk of 256 rows, then over the chunks in chunk order, then into the accumulator -- so the comparison is bitwise."""
import numpy as np

KAPPA = 9.648533215665e-3    # A/fs^2 per eV/(A amu)
KB = 8.617333262e-5          # eV/K
HEAT, MOMENTUM = 0, 1
CHUNK, WAVE = 256, 64
STARTED, ERROR = 1, 2        # M3G_DYN_* flag bits


def inverse_column(lattice, axis: int) -> np.ndarray:
    """Column `axis` of the inverse of `lattice` (rows = lattice vectors), from the adjugate in the library's order (inv3)."""
    L = [float(x) for x in np.asarray(lattice, dtype=np.float64).reshape(9)]
    det = L[0] * (L[4] * L[8] - L[5] * L[7]) - L[1] * (L[3] * L[8] - L[5] * L[6]) + L[2] * (L[3] * L[7] - L[4] * L[6])
    inv = [(L[4] * L[8] - L[5] * L[7]) / det, (L[2] * L[7] - L[1] * L[8]) / det, (L[1] * L[5] - L[2] * L[4]) / det,
           (L[5] * L[6] - L[3] * L[8]) / det, (L[0] * L[8] - L[2] * L[6]) / det, (L[2] * L[3] - L[0] * L[5]) / det,
           (L[3] * L[7] - L[4] * L[6]) / det, (L[1] * L[6] - L[0] * L[7]) / det, (L[0] * L[4] - L[1] * L[3]) / det]
    return np.array([inv[axis], inv[3 + axis], inv[6 + axis]])


def slabs_of(pos, g, n_slabs: int) -> np.ndarray:
    pos = np.asarray(pos, dtype=np.float64)
    f = (pos[:, 0] * g[0] + pos[:, 1] * g[1]) + pos[:, 2] * g[2]
    f = f - np.floor(f)
    return np.minimum((f * float(n_slabs)).astype(np.int64), n_slabs - 1)


def speed2(v) -> np.ndarray:
    v = np.asarray(v, dtype=np.float64)
    return (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]


class RnemdReference:
    """One structure.  `exchange(pos, v, ...)` changes `v` IN PLACE as the device changes the dyn state's velocities."""

    def __init__(self, lattice, masses, kind: int, axis: int, n_slabs: int, n_swaps: int, flow_axis: int = 0, active=None):
        self.m = np.asarray(masses, dtype=np.float64).copy()
        self.n = len(self.m)
        self.kind, self.axis, self.flow_axis, self.n_slabs, self.n_swaps = kind, axis, flow_axis, n_slabs, n_swaps
        self.g = inverse_column(lattice, axis)
        self.active = np.ones(self.n, dtype=bool) if active is None else np.asarray(active).astype(bool)
        self.n_calls = self.n_exchanged = self.n_samples = 0
        self.transferred = 0.0
        self.last_pairs = np.full((n_swaps, 2), -1, dtype=np.int32)
        self.count = np.zeros(n_slabs, dtype=np.int64)
        self.sums = np.zeros((n_slabs, 5))

    def keys(self, v) -> np.ndarray:
        return self.m * speed2(v) if self.kind == HEAT else np.asarray(v)[:, self.flow_axis].copy()

    def terms(self, v) -> np.ndarray:
        return np.stack([self.m, self.m * v[:, 0], self.m * v[:, 1], self.m * v[:, 2], self.m * speed2(v)], axis=1)

    def pairs(self, slab, key) -> list:
        """(row of slab 0, row of slab n_slabs / 2) of pair p = 0, 1, ...: the p-th entry of either list, exchanged or not."""
        ok = self.active & np.isfinite(key)
        cold = sorted((r for r in range(self.n) if ok[r] and slab[r] == 0), key=lambda r: (-key[r], r))
        hot = sorted((r for r in range(self.n) if ok[r] and slab[r] == self.n_slabs // 2), key=lambda r: (key[r], r))
        return list(zip(cold[:self.n_swaps], hot[:self.n_swaps]))

    def exchange(self, pos, v, swap: bool = True, sample: bool = True, flags: int = 0) -> None:
        if flags & (STARTED | ERROR) or not (swap or sample):
            return
        slab, key = slabs_of(pos, self.g, self.n_slabs), self.keys(v)
        if sample:   # from the velocities before the exchange
            term = self.terms(v)
            total = np.zeros((self.n_slabs, 5))
            for lo in range(0, self.n, CHUNK):
                part = np.zeros((self.n_slabs, 5))
                for first in range(lo, min(lo + CHUNK, self.n), WAVE):
                    sub = np.zeros((self.n_slabs, 5))
                    for r in range(first, min(first + WAVE, lo + CHUNK, self.n)):
                        sub[slab[r]] = sub[slab[r]] + term[r]
                        self.count[slab[r]] += 1
                    part = part + sub
                total = total + part
            self.sums = self.sums + total
            self.n_samples += 1
        if swap:
            self.last_pairs[:] = -1
            for p, (i, j) in enumerate(self.pairs(slab, key)):
                if not key[i] > key[j]:
                    continue
                self.last_pairs[p] = (i, j)
                mi, mj = float(self.m[i]), float(self.m[j])
                comps = range(3) if self.kind == HEAT else [self.flow_axis]
                before = v[i].copy()
                for k in comps:
                    a, b = float(v[i, k]), float(v[j, k])
                    if mi == mj:
                        v[i, k], v[j, k] = b, a
                    else:
                        vcm = (mi * a + mj * b) / (mi + mj)
                        v[i, k], v[j, k] = 2.0 * vcm - a, 2.0 * vcm - b
                if self.kind == HEAT:
                    self.transferred += 0.5 * mi * (float(speed2(before)) - float(speed2(v[i]))) / KAPPA
                else:
                    self.transferred += mi * (float(before[self.flow_axis]) - float(v[i, self.flow_axis]))
                self.n_exchanged += 1
        self.n_calls += 1
