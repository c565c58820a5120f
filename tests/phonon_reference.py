"""Numpy restatement of the batched finite-displacement phonons (csrc/m3g_phonons.hip, torch_m3gnet.phonons): the yardstick of the
GPU tests.  One structure at a time, fp64, written for clarity.  The supercell positions use the kernel's operation order (no fused
multiply-add), so that they can be compared bit for bit; the force constants use the same per-entry formula."""
import itertools

import numpy as np

EV, AMU, ANGSTROM, PLANCK, BOLTZMANN = 1.602176634e-19, 1.66053906660e-27, 1e-10, 6.62607015e-34, 1.380649e-23
THZ = np.sqrt(EV / (ANGSTROM ** 2 * AMU)) / (2 * np.pi) / 1e12   # sqrt(eV / (A^2 amu)) -> THz
H_EV_THZ = PLANCK * 1e12 / EV
KB = BOLTZMANN / EV
TRANSLATIONS = np.array(list(itertools.product(range(-2, 3), repeat=3)), dtype=np.float64)


def cell_index(n):
    """[n1 n2 n3, 3] integer translations (l1, l2, l3) in the order l = (l1 n2 + l2) n3 + l3."""
    return np.array(list(itertools.product(range(n[0]), range(n[1]), range(n[2]))), dtype=np.int64)


def supercell(lattice, pos, n):
    """(supercell lattice, positions [N_s, 3]) with atom j = l n_u + b at r_b + l1 L_0 + l2 L_1 + l3 L_2."""
    L = np.asarray(lattice, dtype=np.float64)
    pos = np.asarray(pos, dtype=np.float64)
    ls = cell_index(n).astype(np.float64)
    t = ls[:, 0:1] * L[0]
    t = t + ls[:, 1:2] * L[1]
    t = t + ls[:, 2:3] * L[2]
    return np.asarray(n, dtype=np.float64)[:, None] * L, (pos[None, :, :] + t[:, None, :]).reshape(-1, 3)


def displaced(lattice, pos, n, delta):
    """Rows of the displaced batch of one structure [(1 + 6 n_u) N_s, 3]: copy 0 undisplaced, copy 1 + 6u + 2a + k the home atom u
    moved by +delta (k = 0) / -delta (k = 1) along axis a."""
    _, sp = supercell(lattice, pos, n)
    out = [sp]
    for u in range(len(pos)):
        for a in range(3):
            for sign in (1, -1):
                p = sp.copy()
                p[u, a] = p[u, a] + delta if sign > 0 else p[u, a] - delta
                out.append(p)
    return np.concatenate(out)


def force_constants(forces, n_u, delta, asr=True):
    """(Phi [n_u, N_s, 3, 3], raw sum_j Phi [n_u, 3, 3]) from the forces [(1 + 6 n_u) N_s, 3] (any float dtype) of `displaced`."""
    f = np.asarray(forces).astype(np.float64)
    ns = len(f) // (1 + 6 * n_u)
    copies = f.reshape(1 + 6 * n_u, ns, 3)
    phi = np.empty((n_u, ns, 3, 3))
    for u in range(n_u):
        for a in range(3):
            fp, fm = copies[1 + 6 * u + 2 * a], copies[2 + 6 * u + 2 * a]
            phi[u, :, a, :] = -(fp - fm) / (2.0 * delta)
    sums = phi.sum(axis=1)
    if asr:
        for u in range(n_u):
            phi[u, u] = phi[u, u] - sums[u]
    return phi, sums


def image_table(lattice, pos, n):
    """Per (u, j): the shortest vectors from home atom u to supercell atom j in the supercell's periodicity, in unit-cell fractional
    coordinates [m, 3] (supercell translations {-2..2}^3, ties within 1e-5 A)."""
    L = np.asarray(lattice, dtype=np.float64)
    pos = np.asarray(pos, dtype=np.float64)
    inv = np.linalg.inv(L)
    n_u = len(pos)
    ls = cell_index(n)
    table = {}
    for u in range(n_u):
        for j in range(len(ls) * n_u):
            l, v = divmod(j, n_u)
            f0 = (pos[v] - pos[u]) @ inv + ls[l]
            f = f0[None] + TRANSLATIONS * np.asarray(n)[None]
            r = np.linalg.norm(f @ L, axis=1)
            table[u, j] = f[r <= r.min() + 1e-5]
    return table


def dynamical_matrix(phi, table, masses, q):
    """D(q) [3 n_u, 3 n_u] complex, phonopy's convention, Hermitised."""
    n_u, ns = phi.shape[:2]
    d = np.zeros((3 * n_u, 3 * n_u), dtype=np.complex128)
    q = np.asarray(q, dtype=np.float64)
    for u in range(n_u):
        for j in range(ns):
            v = j % n_u
            img = table[u, j]
            w = np.exp(2j * np.pi * (img @ q)).sum() / len(img)
            d[3 * u:3 * u + 3, 3 * v:3 * v + 3] += phi[u, j] * w / np.sqrt(masses[u] * masses[v])
    return 0.5 * (d + d.conj().T)


def frequencies(d):
    lam = np.linalg.eigvalsh(d)
    return np.sign(lam) * np.sqrt(np.abs(lam)) * THZ


def dos(freqs, weights, grid, sigma):
    f = np.asarray(freqs).reshape(len(weights), -1)
    x = (grid[:, None, None] - f[None]) / sigma
    return (np.exp(-0.5 * x * x).sum(axis=2) * weights[None]).sum(axis=1) / (np.sqrt(2 * np.pi) * sigma)


def thermal(freqs, weights, T, cutoff=1e-3):
    """F, S, Cv, E per cell (eV, eV/K) at T > 0 (K); modes below `cutoff` THz left out."""
    f = np.asarray(freqs).reshape(len(weights), -1)
    w = np.broadcast_to(np.asarray(weights)[:, None], f.shape)[f >= cutoff]
    e = f[f >= cutoff] * H_EV_THZ
    out = {k: [] for k in ("free_energy", "entropy", "heat_capacity", "energy")}
    for t in np.atleast_1d(T):
        x = e / (KB * t)
        n = 1.0 / np.expm1(x)
        out["free_energy"].append((w * (0.5 * e + KB * t * np.log1p(-np.exp(-x)))).sum())
        out["entropy"].append((w * (-KB * np.log1p(-np.exp(-x)) + e * n / t)).sum())
        out["heat_capacity"].append((w * KB * x * x * n * (1 + n)).sum())
        out["energy"].append((w * (0.5 * e + e * n)).sum())
    return {k: np.array(v) for k, v in out.items()}
