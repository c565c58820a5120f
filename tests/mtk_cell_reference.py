"""numpy fp64 restatement of the flexible-cell Martyna-Tobias-Klein NPT ensemble of batched molecular dynamics
(torch_m3gnet.dynamics MtkCellState / mtk_cell_step, C ABI m3g_mtk_*), one structure at a time: the yardstick of
tests/test_mtk_cell_cpu.py and tests/test_gpu_mtk_cell.py, with the interface of nhc_reference.NhcReference.

Units, KAPPA, KB, the 3 n temperature convention and chain_half_step are those of nhc_reference.  Positions and lattice rows are row
vectors, so a symmetric 3x3 matrix acts from the right.  Per structure: g = 3 n - 3 (fix_com) or 3 n, kT = KB T0, Q_1 = g kT taut^2,
Q_k>1 = kT taut^2.  The barostat variable is a symmetric 3x3 rate vg (1/fs), kept as a full matrix here and as 6 numbers in Voigt
order xx, yy, zz, yz, zx, xy in the chain row.  cell_mask "full": all 6 components move, n_c = 6; "orthorhombic": the diagonal only,
n_c = 3.  W_g = (g + 3) kT taup^2 / 3 (the isotropic family's W / 3: vg = veps I has the same kinetic energy); barostat chain masses
Qb_1 = n_c kT taup^2, Qb_k>1 = kT taup^2.

    G = mask o [K + W_vir - V P_ext I + (tr K / g) I] / W_g,   K = sum m v v^T / KAPPA,   W_vir = V unpack(stresses)

One step is T(h) B(h) A(dt) [forces] B(h) T(h), h = dt / 2, and one `step(forces, stresses)` with the forces at `self.pos` does what
one m3g_mtk_step call does: finish the step under way, write the observables, start the next:

    finish (started):   B(h): v = v KV + a KA, the two matrices of the start's kick (vg has not changed since)
                        vg += h G;  barostat chain half-step on W_g sum_ab vg_ab^2 against n_c kT (scales vg);  particle chain
                        half-step on tr K against g kT (v = s1 v, K = s1^2 K)
    observables:        KE, T = 2 KE / (3 n KB), P = tr (W_vir + K) / (3 V), V, extended, 0, (W_vir + K) / V in Voigt order
    start (not finish_only; finish_only clears `started` instead):
                        particle chain half-step (v = s2 v);  barostat chain half-step;  vg += h G
                        B(h): B = (vg + (tr vg / g) I) h, KV = exp(-B), KA = h phi1(-B);  fix_com: v_i -= pbar / m_i
                        A(dt): A = vg dt, x = x exp(A) + dt v phi1(A), lattice = lattice exp(A)
phi1(A) = sum_k A^k / (k + 1)!; exp and phi1 by Horner at the fixed order 12 (no eigensolver, no branch), every product of two
polynomials of the same symmetric matrix kept symmetric by computing its upper triangle only.
extended = g kT xi_1 + kT sum_k>1 xi_k + 1/2 sum Q vxi^2 + P_ext V + 1/2 W_g sum_ab vg_ab^2 + n_c kT xib_1 + kT sum_k>1 xib_k
+ 1/2 sum Qb vxib^2: e_pot + KE + extended is conserved.  Non-finite forces or stresses, or a rate max |vg_ab| dt > 0.05 at the end
of the call's thermostat arithmetic: flagged ERROR, nothing of the call kept, frozen from then on."""
from __future__ import annotations

import numpy as np

from nhc_reference import KAPPA, KB, chain_half_step

STARTED, ERROR = 1, 2
CELL_MASKS = {"full": 0, "orthorhombic": 1}
VOIGT = ((0, 0), (1, 1), (2, 2), (1, 2), (2, 0), (0, 1))
ORDER = 12
MAX_RATE = 0.05


def unpack(v6):
    m = np.empty((3, 3))
    for k, (a, b) in enumerate(VOIGT):
        m[a, b] = m[b, a] = v6[k]
    return m


def pack(m):
    return np.array([m[a, b] for a, b in VOIGT])


def sym_mul(a, q):
    """a q of two commuting symmetric matrices: the upper triangle of the product, mirrored."""
    p = np.triu(a @ q)
    return p + np.triu(p, 1).T


def exp_phi1(a):
    """(exp(a), phi1(a)) of a symmetric matrix by Horner: I + a/1 (I + a/2 (... (I + a/12))), and the same with every divisor + 1."""
    eye = np.eye(3)
    e, p = eye.copy(), eye.copy()
    for k in range(ORDER, 0, -1):
        e = eye + sym_mul(a, e) * (1.0 / k)
        p = eye + sym_mul(a, p) * (1.0 / (k + 1))
    return e, p


class MtkCellReference:
    """One structure: `pos` [n,3] (unwrapped), `lattice` [3,3] (rows = lattice vectors), `masses` [n] amu, `vel` [n,3] A/fs."""

    def __init__(self, pos, lattice, masses, vel, cell_mask="full", temperature=300.0, dt=1.0, taut=100.0, pressure=0.0, taup=1000.0,
                 chain_length=3, chain_substeps=1, fix_com=True):
        if cell_mask not in CELL_MASKS:
            raise ValueError(f"unknown cell_mask {cell_mask!r}")
        self.cell_mask = cell_mask
        self.mask = np.ones((3, 3)) if cell_mask == "full" else np.eye(3)
        self.n_cell = 6.0 if cell_mask == "full" else 3.0
        self.pos = np.array(pos, dtype=np.float64).reshape(-1, 3)
        self.lattice = np.array(lattice, dtype=np.float64).reshape(3, 3)
        self.m = np.array(masses, dtype=np.float64).reshape(-1)
        self.v = np.array(vel, dtype=np.float64).reshape(-1, 3)
        self.t0, self.dt, self.taut, self.p0, self.taup = float(temperature), dt, taut, pressure, taup
        self.M, self.n_c, self.fix_com = int(chain_length), int(chain_substeps), bool(fix_com)
        n = len(self.m)
        if not (1 <= self.M <= 8 and 1 <= self.n_c <= 8) or not self.t0 > 0.0 or (self.fix_com and n == 1):
            raise ValueError("chain_length and chain_substeps in 1..8, temperature > 0, more than one atom with fix_com")
        self.g = 3.0 * n - 3.0 if self.fix_com else 3.0 * n
        self.kt = KB * self.t0
        self.q = np.full(self.M, self.kt * taut * taut)
        self.q[0] = self.g * self.kt * taut * taut
        self.qb = np.full(self.M, self.kt * taup * taup)
        self.qb[0] = self.n_cell * self.kt * taup * taup
        self.wg = (self.g + 3.0) * self.kt * taup * taup / 3.0
        self.xi, self.vxi, self.xib, self.vxib = (np.zeros(self.M) for _ in range(4))
        self.vg = np.zeros((3, 3))
        self.kick = (np.eye(3), np.zeros((3, 3)))
        self.flags, self.n_steps = 0, 0
        self.lam = 1.0
        self.max_rate = 0.0
        self.obs = np.full(12, np.nan)

    def _volume(self):
        L = self.lattice
        return abs(L[0, 0] * (L[1, 1] * L[2, 2] - L[1, 2] * L[2, 1]) - L[0, 1] * (L[1, 0] * L[2, 2] - L[1, 2] * L[2, 0])
                   + L[0, 2] * (L[1, 0] * L[2, 1] - L[1, 1] * L[2, 0]))

    def _g(self, kt, w, vol):
        return self.mask * (kt + w + (np.trace(kt) / self.g - vol * self.p0) * np.eye(3)) / self.wg

    @staticmethod
    def _baro_chain(qb, xib, vxib, vg, wg, n_cell, kt, h, n_c):
        s, _ = chain_half_step(qb, xib, vxib, wg * (vg * vg).sum(), n_cell * kt, kt, h, n_c)
        return vg * s

    def _extended(self, xi, vxi, xib, vxib, vg, vol):
        return (self.g * self.kt * xi[0] + self.kt * xi[1:].sum() + 0.5 * (self.q * vxi * vxi).sum()
                + self.p0 * vol + 0.5 * self.wg * (vg * vg).sum()
                + self.n_cell * self.kt * xib[0] + self.kt * xib[1:].sum() + 0.5 * (self.qb * vxib * vxib).sum())

    def extended(self, vol=None):
        return self._extended(self.xi, self.vxi, self.xib, self.vxib, self.vg, self._volume() if vol is None else vol)

    def step(self, forces, stresses, finish_only: bool = False) -> None:
        if self.flags & ERROR:
            return
        f = np.asarray(forces, dtype=np.float64).reshape(-1, 3)
        s6 = np.asarray(stresses, dtype=np.float64).reshape(6)
        if not np.isfinite(f).all() or not np.isfinite(s6).all():
            self.flags |= ERROR
            return
        n, h, m = len(self.m), 0.5 * self.dt, self.m[:, None]
        a = KAPPA * f / m
        started = bool(self.flags & STARTED)
        v = self.v @ self.kick[0] + a @ self.kick[1] if started else self.v.copy()
        kt = np.einsum("i,ia,ib->ab", self.m, v, v) / KAPPA   # K: its trace is twice the kinetic energy
        mv, fsum = (m * v).sum(0), f.sum(0)
        vol = self._volume()
        w = vol * unpack(s6)
        gkt = self.g * self.kt
        # (on copies: a call that ends over the rate keeps nothing)
        xi, vxi, xib, vxib, vg = self.xi.copy(), self.vxi.copy(), self.xib.copy(), self.vxib.copy(), self.vg.copy()
        baro = lambda vg: self._baro_chain(self.qb, xib, vxib, vg, self.wg, self.n_cell, self.kt, h, self.n_c)   # noqa: E731
        s1 = 1.0
        if started:
            vg = vg + h * self._g(kt, w, vol)
            vg = baro(vg)
            s1, _ = chain_half_step(self.q, xi, vxi, np.trace(kt), gkt, self.kt, h, self.n_c)
            kt = s1 * s1 * kt
        k2 = np.trace(kt)
        pt = (w + kt) / vol
        obs = np.concatenate([[0.5 * k2, k2 / (3.0 * n * KB), np.trace(pt) / 3.0, vol, self._extended(xi, vxi, xib, vxib, vg, vol), 0.0],
                              pack(pt)])
        if not finish_only:
            s2, _ = chain_half_step(self.q, xi, vxi, k2, gkt, self.kt, h, self.n_c)
            kt = s2 * s2 * kt
            vg = baro(vg)
            vg = vg + h * self._g(kt, w, vol)
        rate = np.abs(vg).max() * self.dt
        if not rate <= MAX_RATE:
            self.flags |= ERROR
            return
        self.max_rate = max(self.max_rate, rate)
        self.xi, self.vxi, self.xib, self.vxib, self.vg, self.obs = xi, vxi, xib, vxib, vg, obs
        if finish_only:
            self.v = s1 * v
            self.flags &= ~STARTED
            return
        lam = s1 * s2
        kv, ka = exp_phi1(-(vg + np.trace(vg) / self.g * np.eye(3)) * h)
        ka = h * ka
        dx, dv = exp_phi1(vg * self.dt)
        dv = self.dt * dv
        self.lattice = self.lattice @ dx
        v = lam * v
        v = v @ kv + a @ ka
        if self.fix_com:
            v = v - ((lam * mv) @ kv + (KAPPA * fsum) @ ka) / n / m
        self.pos = self.pos @ dx + v @ dv
        self.v, self.kick, self.lam = v, (kv, ka), lam
        self.flags |= STARTED
        self.n_steps += 1

    def chain_row(self):
        """xi, vxi, xib, vxib, then vg in Voigt order: the row m3g_mtk_read returns."""
        return np.concatenate([self.xi, self.vxi, self.xib, self.vxib, pack(self.vg)])

    def reverse(self) -> None:
        """Negate every velocity (after a finish_only step): the next steps retrace the trajectory."""
        self.v, self.vxi, self.vxib, self.vg = -self.v, -self.vxi, -self.vxib, -self.vg
