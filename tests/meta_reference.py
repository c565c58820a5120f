"""Numpy fp64 restatement of collective-variable biasing (torch_m3gnet.metadynamics, C ABI m3g_meta_*, csrc/m3g_meta.hip): one
m3g_meta_bias call of one walker group, and the hill bookkeeping.  Every rounding of the device is repeated in its order -- no product
is fused with a sum; rows are summed over chunks of 256 in the fixed tree, the chunk partials lane-strided over 64 lanes in chunk order
and then by the butterfly; a COORDINATION row walks its partner rows in row order; the hills are summed lane-strided in list order and
then by the butterfly -- so everything free of `exp` is bitwise the device's.  `exp` is a parameter (numpy's by default): the tests
nudge it by one ulp to measure how far an exp that differs in its last bit moves the results."""
import numpy as np

CHUNK, WAVE = 256, 64
DISTANCE, PROJECTION, COORDINATION = 0, 1, 2
ERROR, FULL = 1, 2
COLS = 8                      # per CV and chunk: sum w, sum w x [3] over A, the same over B; COORDINATION: its sum, 7 unused
PART = 2 * COLS + 1           # ... and the number of rows that take part and are not finite


def inverse(lattice) -> np.ndarray:
    """The inverse of `lattice` (rows = lattice vectors) from the adjugate, in the library's order (inv3), flat [9]."""
    L = [float(x) for x in np.asarray(lattice, dtype=np.float64).reshape(9)]
    det = L[0] * (L[4] * L[8] - L[5] * L[7]) - L[1] * (L[3] * L[8] - L[5] * L[6]) + L[2] * (L[3] * L[7] - L[4] * L[6])
    return np.array([(L[4] * L[8] - L[5] * L[7]) / det, (L[2] * L[7] - L[1] * L[8]) / det, (L[1] * L[5] - L[2] * L[4]) / det,
                     (L[5] * L[6] - L[3] * L[8]) / det, (L[0] * L[8] - L[2] * L[6]) / det, (L[2] * L[3] - L[0] * L[5]) / det,
                     (L[3] * L[7] - L[4] * L[6]) / det, (L[1] * L[6] - L[0] * L[7]) / det, (L[0] * L[4] - L[1] * L[3]) / det])


def chunk_tree(rows: np.ndarray) -> np.ndarray:
    """[n, K] row terms -> [chunks, K]: the fixed tree over every chunk of 256 rows (rows beyond the structure contribute 0.0)."""
    n, k = rows.shape
    chunks = (n + CHUNK - 1) // CHUNK
    a = np.zeros((chunks * CHUNK, k))
    a[:n] = rows
    a = a.reshape(chunks, CHUNK, k)
    w = CHUNK // 2
    while w > 0:
        a[:, :w] = a[:, :w] + a[:, w:2 * w]
        w //= 2
    return a[:, 0].copy()


def butterfly(acc: np.ndarray) -> np.ndarray:
    """[64, ...] lane values -> the value every lane ends with (a + b on both partners)."""
    lanes = np.arange(WAVE)
    w = WAVE // 2
    while w > 0:
        acc = acc + acc[lanes ^ w]
        w //= 2
    assert (acc == acc[0]).all() or np.isnan(acc).any()
    return acc[0]


def lane_strided_sum(terms: np.ndarray) -> np.ndarray:
    """[n, ...] terms -> their sum as one wave forms it: lane l adds the terms l, l + 64, ... in order from 0.0, then the butterfly."""
    n = len(terms)
    blocks = (n + WAVE - 1) // WAVE
    a = np.zeros((blocks * WAVE,) + terms.shape[1:])
    a[:n] = terms
    acc = np.zeros((WAVE,) + terms.shape[1:])
    for b in range(blocks):
        acc = acc + a[b * WAVE:(b + 1) * WAVE]
    return butterfly(acc)


def power(x, q: int):
    """x^q by repeated multiplication, q >= 0."""
    y = np.ones_like(x)
    for k in range(q):
        y = x.copy() if k == 0 else y * x
    return y


class Cv:
    """One collective variable over n atoms: `kind`, membership [n] (0 none, 1 A, 2 B, 3 both) and the scalar parameters."""

    def __init__(self, kind: int, membership, direction=None, p: int = 3, r0: float = 1.0, r_cut: float = 2.0):
        self.kind, self.m = kind, np.asarray(membership, dtype=np.uint8)
        self.direction = None if direction is None else np.asarray(direction, dtype=np.float64)
        self.p, self.r0, self.r_cut = int(p), float(r0), float(r_cut)


def coordination(cv: Cv, pos, lattice):
    """(sum per row [n], gradient rows [n,3]) of a COORDINATION CV: row i over its partners j != i in row order."""
    pos = np.asarray(pos, dtype=np.float64)
    n = len(pos)
    inv, l = inverse(lattice), np.asarray(lattice, dtype=np.float64).reshape(9)
    with np.errstate(all="ignore"):
        f = np.stack([(pos[:, 0] * inv[a] + pos[:, 1] * inv[3 + a]) + pos[:, 2] * inv[6 + a] for a in range(3)], axis=1)
        r0sq = np.float64(cv.r0 * cv.r0)
        tc = np.float64(cv.r_cut * cv.r_cut) / r0sq
        sig_c = 1.0 / (1.0 + power(tc, cv.p - 1) * tc)
        one_m = 1.0 - sig_c
        k2 = (2.0 / r0sq) / one_m
        in_a, in_b = (cv.m & 1) != 0, (cv.m & 2) != 0
        rows = np.arange(n)
        total, g = np.zeros(n), np.zeros((n, 3))
        for j in range(n):
            d = f - f[j]
            d = d - np.rint(d)
            e = np.stack([(d[:, 0] * l[a] + d[:, 1] * l[3 + a]) + d[:, 2] * l[6 + a] for a in range(3)], axis=1)
            r2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
            r = np.sqrt(r2)
            ab, ba = in_a & bool(in_b[j]), in_b & bool(in_a[j])
            on = (ab | ba) & (r < cv.r_cut) & (rows != j)
            tt = r2 / r0sq
            tpm = power(tt, cv.p - 1)
            sig = 1.0 / (1.0 + tpm * tt)
            total = total + np.where(on & ab, (sig - sig_c) / one_m, 0.0)
            dc = -(((sig * sig) * (float(cv.p) * tpm)) * k2)
            mult = np.where(ab & ba, 2.0, 1.0)
            g = g + np.where(on[:, None], (dc[:, None] * e) * mult[:, None], 0.0)
    return total, g


def min_image_distance(pos, lattice, i: int, j: int) -> float:
    """r_ij as `coordination` forms it."""
    pos = np.asarray(pos, dtype=np.float64)
    inv, l = inverse(lattice), np.asarray(lattice, dtype=np.float64).reshape(9)
    f = np.stack([(pos[:, 0] * inv[a] + pos[:, 1] * inv[3 + a]) + pos[:, 2] * inv[6 + a] for a in range(3)], axis=1)
    d = f[i] - f[j]
    d = d - np.rint(d)
    e = [(d[0] * l[a] + d[1] * l[3 + a]) + d[2] * l[6 + a] for a in range(3)]
    return float(np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]))


def evaluate(cvs, pos, lattice, weights, origins=None):
    """k_meta_partials and the first part of k_meta_finalize for one structure: dict with s [n_cv], finite, the unit vectors u
    [n_cv,3], the group weights wa, wb [n_cv] and the gradient rows d s_k / d x_i [n_cv, n, 3] (as k_meta_apply builds them)."""
    pos, w = np.asarray(pos, dtype=np.float64), np.asarray(weights, dtype=np.float64)
    n, n_cv = len(pos), len(cvs)
    rows = np.zeros((n, PART))
    coord = {}
    any_m = np.zeros(n, dtype=bool)
    with np.errstate(all="ignore"):
        for k, cv in enumerate(cvs):
            any_m |= cv.m != 0
            if cv.kind == COORDINATION:
                rows[:, COLS * k], coord[k] = coordination(cv, pos, lattice)
                continue
            wa, wb = np.where(cv.m & 1, w, 0.0), np.where(cv.m & 2, w, 0.0)
            rows[:, COLS * k], rows[:, COLS * k + 4] = wa, wb
            for a in range(3):
                rows[:, COLS * k + 1 + a], rows[:, COLS * k + 5 + a] = wa * pos[:, a], wb * pos[:, a]
        rows[:, PART - 1] = np.where(any_m & ~np.isfinite(pos).all(axis=1), 1.0, 0.0)
        acc = lane_strided_sum(chunk_tree(rows))
        s, u, was, wbs = np.zeros(n_cv), np.zeros((n_cv, 3)), np.zeros(n_cv), np.zeros(n_cv)
        grad = np.zeros((n_cv, n, 3))
        finite = acc[PART - 1] == 0.0
        for k, cv in enumerate(cvs):
            q = acc[COLS * k:COLS * (k + 1)]
            if cv.kind == COORDINATION:
                s[k], grad[k] = q[0], coord[k]
            else:
                was[k], wbs[k] = q[0], q[4]
                cb = q[5:8] / wbs[k] if wbs[k] > 0.0 else np.zeros(3)
                d = q[1:4] / was[k] - cb
                if cv.kind == DISTANCE:
                    length = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
                    s[k] = length
                    u[k] = d / length if length > 0.0 else 0.0
                else:
                    d = d - (np.zeros(3) if origins is None else np.asarray(origins, dtype=np.float64).reshape(n_cv, 3)[k])
                    u[k] = cv.direction
                    s[k] = (d[0] * u[k][0] + d[1] * u[k][1]) + d[2] * u[k][2]
                share = np.where(cv.m & 1, w / was[k], 0.0)
                share = np.where(cv.m & 2, share - w / wbs[k], share)
                grad[k] = share[:, None] * u[k][None, :]
            finite = finite and bool(np.isfinite(s[k]))
    return {"s": s, "finite": bool(finite), "u": u, "wa": was, "wb": wbs, "grad": grad}


def hills_sum(s, centres, heights, sigma, exp=np.exp):
    """(V_hills, dV_hills/ds [n_cv], sum |term| of each of these 1 + n_cv sums, n) of the hills `centres` [n, n_cv], `heights` [n] at `s` [n_cv]."""
    s, sigma = np.asarray(s, dtype=np.float64), np.asarray(sigma, dtype=np.float64)
    n_cv = len(s)
    inv_s2 = 1.0 / (sigma * sigma)
    centres = np.asarray(centres, dtype=np.float64).reshape(-1, n_cv)
    heights = np.asarray(heights, dtype=np.float64).reshape(-1)
    d = s[None, :] - centres
    q = np.zeros(len(heights))
    for k in range(n_cv):
        q = q + (d[:, k] * d[:, k]) * inv_s2[k]
    term = heights * exp(-(0.5 * q))
    cols = np.concatenate([term[:, None], term[:, None] * (d * inv_s2[None, :])], axis=1)
    total = lane_strided_sum(cols)
    return float(total[0]), -total[1:], np.abs(cols).sum(0), len(heights)


def restraint(s, centre, kappa, walls, dv_hills):
    """(V_restraint + walls, dV/ds [n_cv] = ((dV_hills/ds + restraint) + lower wall) + upper wall) in the device's order; walls
    [n_cv, 4] = lower, its kappa, upper, its kappa."""
    n_cv = len(s)
    vr, dv = 0.0, np.array(dv_hills, dtype=np.float64)
    for k in range(n_cv):
        ds = s[k] - centre[k]
        vr = vr + (0.5 * kappa[k]) * (ds * ds)
        dv[k] = dv[k] + kappa[k] * ds
        lo, klo, hi, khi = walls[k]
        if klo > 0.0 and s[k] < lo:
            dl = s[k] - lo
            vr = vr + (0.5 * klo) * (dl * dl)
            dv[k] = dv[k] + klo * dl
        if khi > 0.0 and s[k] > hi:
            du = s[k] - hi
            vr = vr + (0.5 * khi) * (du * du)
            dv[k] = dv[k] + khi * du
    return float(vr), dv


class Group:
    """One walker group: R walkers that share a hill list.  `walkers`: one dict per walker with lattice, weights, and optional
    origins [n_cv,3], centre [n_cv], kappa [n_cv], walls [n_cv,4]; `cvs`: the CVs (one membership for every walker: the walkers
    of a group are copies of one structure here, which the device does not demand)."""

    def __init__(self, cvs, walkers, sigma, height, inv_kdt, max_hills, exp=np.exp):
        self.cvs, self.walkers, self.n_cv, self.R = cvs, walkers, len(cvs), len(walkers)
        self.sigma, self.height, self.inv_kdt, self.max_hills, self.exp = np.asarray(sigma, dtype=np.float64), float(height), float(inv_kdt), max_hills, exp
        self.centres, self.heights = np.zeros((max_hills, self.n_cv)), np.zeros(max_hills)
        self.deposits, self.flags = 0, [0] * self.R

    @property
    def n_hills(self) -> int:
        return self.deposits * self.R

    def set_hills(self, centres, heights) -> None:
        centres = np.asarray(centres, dtype=np.float64).reshape(-1, self.n_cv)
        assert len(centres) % self.R == 0 and len(centres) <= self.max_hills
        self.deposits = len(centres) // self.R
        self.centres[:len(centres)], self.heights[:len(centres)] = centres, heights

    def bias(self, positions, forces, deposit=False):
        """One call: `positions` and `forces` (float32) per walker.  Returns per walker (obs [8], forces_out float32, extras) where
        extras holds the evaluation, sum |hill term| and the number of hills summed; then appends the deposits."""
        n = self.n_hills
        out, new = [], []
        full = deposit and (self.deposits + 1) * self.R > self.max_hills
        for r, (wk, pos, f) in enumerate(zip(self.walkers, positions, forces)):
            ev = evaluate(self.cvs, pos, wk["lattice"], wk["weights"], wk.get("origins"))
            s, n_cv = ev["s"], self.n_cv
            zeros = np.zeros(n_cv)
            vh, dh, abs_sum = 0.0, zeros.copy(), np.zeros(1 + n_cv)
            if ev["finite"]:
                vh, dh, abs_sum, _ = hills_sum(s, self.centres[:n], self.heights[:n], self.sigma, self.exp)
            with np.errstate(all="ignore"):
                vr, dv = restraint(s, wk.get("centre", zeros), wk.get("kappa", zeros), wk.get("walls", np.zeros((n_cv, 4))), dh)
            if not ev["finite"]:
                self.flags[r] |= ERROR
            height = 0.0
            if deposit:
                if full:
                    self.flags[r] |= FULL
                else:
                    if ev["finite"]:
                        height = float(self.height * self.exp(np.float64(-(vh * self.inv_kdt))))
                    new.append((s.copy() if ev["finite"] else zeros, height))
            f = np.asarray(f, dtype=np.float32)
            f_out = f.copy()
            if ev["finite"]:
                b = np.zeros((len(f), 3))
                touched = np.zeros(len(f), dtype=bool)
                for k, cv in enumerate(self.cvs):
                    on = cv.m != 0
                    touched |= on
                    b = b + np.where(on[:, None], dv[k] * ev["grad"][k], 0.0)
                f_out[touched] = (f.astype(np.float64) - b).astype(np.float32)[touched]
            obs = np.zeros(8)
            obs[:n_cv] = s
            if ev["finite"]:
                obs[2], obs[3], obs[4] = vh + vr, vh, vr
                obs[5:5 + n_cv] = dv
            obs[7] = height
            out.append((obs, f_out, dict(ev, abs_sum=abs_sum, n_terms=n, dv=dv)))
        if new:
            for r, (c, h) in enumerate(new):
                self.centres[n + r], self.heights[n + r] = c, h
            self.deposits += 1
        return out


def nudged_exp(sign: int):
    """numpy's exp moved by one ulp up (+1) or down (-1): what an exp that differs in its last bit would return."""
    def exp(x):
        y = np.exp(x)
        return np.nextafter(y, np.inf if sign > 0 else -np.inf)
    return exp
