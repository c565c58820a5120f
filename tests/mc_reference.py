"""Plain-Python fp64 restatement of batched atom-swap Monte Carlo (torch_m3gnet.monte_carlo / m3g_mc_*), one structure at a time: the
yardstick of tests/test_mc_cpu.py and tests/test_gpu_mc.py.

A structure has n rows (sites) with species `types`, a site mask `active`, a temperature T and a seed.  Call a = 0, 1, ... :

    propose(E):   draws Philox4x64-10, counter (a, 0, 0, 0), key (seed, 2); u_k = ((w_k >> 11) + 0.5) 2^-53.  n_p active rows; i = the
                  active row of rank min(int(u_0 n_p), n_p - 1); m active rows of another species than i's; j = the one of rank
                  min(int(u_1 m), m - 1) among them; the species of i and j are exchanged, (i, j) and u_2 kept, PENDING set.  Not
                  attempted (only the counter advances): already PENDING (sets ERR_ORDER), dynamics flags ERROR or STARTED, E not
                  finite, or fewer than two species on the active rows (sets NO_PAIR).
    decide(E', E): for a PENDING structure dE = E' - E; a non-finite E' is rejected and counted; else accepted iff dE <= 0 or
                  u_2 < exp(-dE / (KB T)).  Reject: i and j exchanged back.  The current energy after the verdict joins count / mean /
                  M2 (Welford); row a of the history becomes (i, j, verdict), (-1, -1, -1) for a call that did not attempt.

`margins` collects log(u_2) + dE / (KB T) of every trial with dE > 0: a comparison of two transcendental results is only reproducible
elsewhere when |margin| is far above their rounding."""
from __future__ import annotations

import math

import numpy as np

import md_reference as mr

KB = mr.KB
NO_PAIR, PENDING, ERR_ORDER = 1, 2, 4
_BLOCK = 4096   # proposals whose uniforms are drawn in one vectorised Philox call


class SwapReference:
    def __init__(self, types, temperature: float, seed: int, active=None):
        self.types = [int(t) for t in types]
        n = len(self.types)
        self.active = [True] * n if active is None else [bool(x) for x in active]
        assert len(self.active) == n and temperature > 0
        self.rows = [r for r in range(n) if self.active[r]]
        self.T, self.seed = float(temperature), int(seed)
        self.flags = NO_PAIR if len(self.rows) < 2 else 0
        self.counter = self.decided = 0
        self.pair, self.u2 = (0, 0), 0.0
        self.attempts = self.accepts = self.nonfinite = self.count = 0
        self.mean = self.m2 = 0.0
        self.history = {}    # call -> (i, j, verdict)
        self.margins = []
        self._u_at, self._u = -1, None

    def uniforms(self, a: int):
        if a // _BLOCK != self._u_at:
            self._u_at = a // _BLOCK
            ctr = np.zeros((_BLOCK, 4), dtype=np.uint64)
            ctr[:, 0] = np.arange(_BLOCK, dtype=np.uint64) + np.uint64(self._u_at * _BLOCK)
            w = mr.philox4x64_10(ctr, np.array([self.seed, 2], dtype=np.uint64))
            self._u = (((w >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53).tolist()
        return self._u[a % _BLOCK]

    def propose(self, energy: float, dyn_flags: int = 0):
        """One call; returns the pair (i, j) whose species were exchanged, or None when the structure was not attempted."""
        a = self.counter
        self.counter = a + 1
        if self.flags & PENDING:
            self.flags |= ERR_ORDER
            return None
        if (dyn_flags & (mr.ERROR | mr.STARTED)) or not math.isfinite(float(energy)):
            return None
        u = self.uniforms(a)
        t, rows = self.types, self.rows
        n_p = len(rows)
        others = []
        if n_p >= 2:
            i = rows[min(int(u[0] * n_p), n_p - 1)]
            others = [r for r in rows if t[r] != t[i]]
        if not others:
            self.flags |= NO_PAIR
            return None
        m = len(others)
        j = others[min(int(u[1] * m), m - 1)]
        t[i], t[j] = t[j], t[i]
        self.pair, self.u2 = (i, j), u[2]
        self.flags |= PENDING
        return i, j

    def decide(self, trial: float, energy: float):
        """(verdict, current energy): verdict 1 / 0, or None when nothing was pending (the energy then comes back as given)."""
        a = self.counter - 1
        due = self.decided != a + 1
        verdict, current = None, energy
        if self.flags & PENDING:
            e_new, e_old = float(trial), float(energy)
            verdict = 0
            if not math.isfinite(e_new):
                self.nonfinite += 1
            else:
                dE = e_new - e_old
                if dE <= 0.0:
                    verdict = 1
                else:
                    x = -dE / (KB * self.T)
                    self.margins.append(math.log(self.u2) - x)
                    verdict = 1 if self.u2 < math.exp(x) else 0
            if verdict:
                current = trial
            else:
                i, j = self.pair
                self.types[i], self.types[j] = self.types[j], self.types[i]
            e = e_new if verdict else e_old
            self.attempts += 1
            self.accepts += verdict
            self.count += 1
            d = e - self.mean
            self.mean += d / self.count
            self.m2 += d * (e - self.mean)
            self.flags &= ~PENDING
        if due and a >= 0:
            self.history[a] = (self.pair[0], self.pair[1], verdict) if verdict is not None else (-1, -1, -1)
            self.decided = a + 1
        return verdict, current

    def propose_dyn(self, energy: float, ref):
        """propose on the md_reference.DynReference of the structure: its flags decide, and the masses and velocities of the two rows
        travel with the species."""
        pair = self.propose(energy, ref.flags)
        if pair is not None:
            _swap_rows(ref, *pair)
        return pair

    def decide_dyn(self, trial: float, energy: float, ref):
        pair = self.pair if self.flags & PENDING else None
        verdict, current = self.decide(trial, energy)
        if pair is not None and not verdict:
            _swap_rows(ref, *pair)
        return verdict, current

    def history_array(self, rows: int, fill: int) -> np.ndarray:
        """[rows, 3] int32: the rows written so far, `fill` where no decide has written."""
        h = np.full((rows, 3), fill, dtype=np.int32)
        for a, row in self.history.items():
            if a < rows:
                h[a] = row
        return h


def _swap_rows(ref, i: int, j: int) -> None:
    ref.m[[i, j]] = ref.m[[j, i]]
    ref.v[[i, j]] = ref.v[[j, i]]
