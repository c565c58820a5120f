"""Plain-Python fp64 restatement of the replica-exchange decide rule and its bookkeeping (torch_m3gnet.replica_exchange / m3g_remd_*),
one ladder at a time: the yardstick of tests/test_remd_cpu.py and tests/test_gpu_remd.py.

A ladder of R replicas has ascending temperatures T[0..R); replica r starts holding index r.  Attempt a = 0, 1, ... at the energies E[r]
and the flags of the replicas (md_reference.STARTED / ERROR):

    1. E of every replica without ERROR and with a finite E joins count / mean / M2 (Welford) of the index it holds, before any swap;
    2. pairs (k, k+1) with k % 2 == a % 2: i holds k, j holds k+1, Delta = (1/(KB T_k) - 1/(KB T_{k+1})) (E_i - E_j); accepted iff
       Delta >= 0 or u < exp(Delta), u = ((w0 >> 11) + 0.5) 2^-53 of Philox4x64-10, counter (a, k, 0, 0), key (seed, 1);
    3. a pair with ERROR or STARTED on either replica, or a non-finite energy, is not attempted (not counted, nothing written);
    4. on accept the held indices and the holder map are swapped, scale[i] = sqrt(T_{k+1}/T_k), scale[j] = sqrt(T_k/T_{k+1}); every
       other replica has scale exactly 1;
    5. round trips: a replica that reaches R-1 after last touching 0, and then reaches 0 again, has completed one;
    6. the held indices are appended to the history.

`margins` collects log(u) - Delta of every attempted pair with Delta < 0: a comparison of two transcendental results is only
reproducible elsewhere when |margin| is far above their rounding."""
from __future__ import annotations

import math

import numpy as np

import md_reference as mr

KB = mr.KB
UP, DOWN = 1, 2
_BLOCK = 1024   # attempts whose uniforms are drawn in one vectorised Philox call


class LadderReference:
    def __init__(self, temperatures, seed: int):
        self.T = [float(t) for t in temperatures]
        self.R = len(self.T)
        assert self.R >= 2 and all(b > a > 0 for a, b in zip(self.T, self.T[1:]))
        self.seed = int(seed)
        R = self.R
        self.held = list(range(R))       # per replica
        self.holder = list(range(R))     # per index
        self.label = [UP] + [0] * (R - 1)
        self.round_trips = [0] * R
        self.count, self.mean, self.m2 = [0] * R, [0.0] * R, [0.0] * R
        self.attempts, self.accepts = [0] * (R - 1), [0] * (R - 1)
        self.n_attempts = 0
        self.history = [list(range(R))]  # the start, then one row per attempt
        self.margins = []
        self._u_at, self._u = -1, None

    def uniform(self, a: int, k: int) -> float:
        if a // _BLOCK != self._u_at:
            self._u_at = a // _BLOCK
            ctr = np.zeros((_BLOCK, max(self.R - 1, 1), 4), dtype=np.uint64)
            ctr[..., 0] = (np.arange(_BLOCK, dtype=np.uint64) + np.uint64(self._u_at * _BLOCK))[:, None]
            ctr[..., 1] = np.arange(ctr.shape[1], dtype=np.uint64)[None]
            w = mr.philox4x64_10(ctr, np.array([self.seed, 1], dtype=np.uint64))[..., 0]
            self._u = ((w >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53
        return float(self._u[a % _BLOCK, k])

    def exchange(self, energies, flags=None) -> list:
        """One attempt; returns the velocity scale of every replica."""
        R, T, a = self.R, self.T, self.n_attempts
        E = [float(e) for e in energies]
        fl = [0] * R if flags is None else [int(f) for f in flags]
        for k in range(R):
            r = self.holder[k]
            if (fl[r] & mr.ERROR) or not math.isfinite(E[r]):
                continue
            self.count[k] += 1
            d = E[r] - self.mean[k]
            self.mean[k] += d / self.count[k]
            self.m2[k] += d * (E[r] - self.mean[k])
        scale = [1.0] * R
        for k in range(a & 1, R - 1, 2):
            i, j = self.holder[k], self.holder[k + 1]
            if ((fl[i] | fl[j]) & (mr.ERROR | mr.STARTED)) or not (math.isfinite(E[i]) and math.isfinite(E[j])):
                continue
            delta = (1.0 / (KB * T[k]) - 1.0 / (KB * T[k + 1])) * (E[i] - E[j])
            accept = delta >= 0.0
            if not accept:
                u = self.uniform(a, k)
                self.margins.append(math.log(u) - delta)
                accept = u < math.exp(delta)
            self.attempts[k] += 1
            if not accept:
                continue
            self.accepts[k] += 1
            self.held[i], self.held[j] = k + 1, k
            self.holder[k], self.holder[k + 1] = j, i
            scale[i], scale[j] = math.sqrt(T[k + 1] / T[k]), math.sqrt(T[k] / T[k + 1])
        for r in range(R):
            if self.held[r] == 0:
                if self.label[r] == DOWN:
                    self.round_trips[r] += 1
                self.label[r] = UP
            elif self.held[r] == R - 1 and self.label[r] == UP:
                self.label[r] = DOWN
        self.history.append(list(self.held))
        self.n_attempts += 1
        return scale

    def exchange_dyn(self, energies, refs) -> list:
        """One attempt on the md_reference.DynReference objects of the ladder's replicas: the flags are theirs, and an accepted
        replica gets its new target temperature and scaled velocities.  Returns the scales."""
        scale = self.exchange(energies, [ref.flags for ref in refs])
        for r, ref in enumerate(refs):
            ref.t0 = self.T[self.held[r]]
            if scale[r] != 1.0:
                ref.v = ref.v * scale[r]
        return scale


def round_trips_of(history) -> list:
    """The round trips of every replica by a direct scan of its column of the history ([n + 1, R]: the start, then every attempt)."""
    h = np.asarray(history)
    R = h.shape[1]
    trips = []
    for r in range(R):
        n, seen_bottom, seen_top = 0, False, False
        for idx in h[:, r]:
            if idx == 0:
                if seen_bottom and seen_top:
                    n += 1
                seen_bottom, seen_top = True, False
            elif idx == R - 1 and seen_bottom:
                seen_top = True
        trips.append(n)
    return trips
