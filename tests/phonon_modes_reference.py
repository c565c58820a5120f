"""Numpy restatement of the phonon eigenvectors and group velocities (csrc/m3g_phonons.hip: m3g_ph_dynmat_gradient,
m3g_ph_group_velocities; torch_m3gnet.phonons): the yardstick of tests/test_gpu_phonon_modes.py, with `numpy.linalg.eigh` where the
device has its own Jacobi solver.  One structure and one q-point at a time, fp64, written for clarity.  Eigenvectors are unique only
up to a phase and, in a degenerate set, up to a unitary: compare invariants (residuals, projectors, per-set traces, the eigenvalues
of W), never raw entries."""
import numpy as np

import phonon_reference as pr

THZ = pr.THZ


def cartesian_q(lattice, q_frac):
    """q in 1/A without 2 pi (rows of inv(L)^T are the reciprocal vectors), the convention of `band_structure`'s distance."""
    return np.asarray(q_frac, dtype=np.float64) @ np.linalg.inv(np.asarray(lattice, dtype=np.float64)).T


def fractional_q(lattice, q_cart):
    return np.asarray(q_cart, dtype=np.float64) @ np.asarray(lattice, dtype=np.float64).T


def dynamical_matrix_gradient(phi, table, masses, q, lattice):
    """dD / dq_alpha [3, 3 n_u, 3 n_u] for the Cartesian q: every image term of `pr.dynamical_matrix` times 2 pi i r_alpha with
    r = d L the Cartesian image vector; Hermitised like D."""
    n_u, ns = phi.shape[:2]
    L = np.asarray(lattice, dtype=np.float64)
    g = np.zeros((3, 3 * n_u, 3 * n_u), dtype=np.complex128)
    q = np.asarray(q, dtype=np.float64)
    for u in range(n_u):
        for j in range(ns):
            v = j % n_u
            img = table[u, j]
            r = img @ L                                                   # [m, 3]
            w = (2j * np.pi * r * np.exp(2j * np.pi * (img @ q))[:, None]).sum(axis=0) / len(img)   # [3]
            g[:, 3 * u:3 * u + 3, 3 * v:3 * v + 3] += w[:, None, None] * phi[u, j][None] / np.sqrt(masses[u] * masses[v])
    return 0.5 * (g + g.conj().transpose(0, 2, 1))


def degenerate_sets(freqs, tolerance):
    """[(begin, end)]: maximal runs of consecutive ascending frequencies whose neighbouring gaps are below `tolerance`."""
    sets, begin = [], 0
    for i in range(1, len(freqs) + 1):
        if i == len(freqs) or not freqs[i] - freqs[i - 1] < tolerance:
            sets.append((begin, i))
            begin = i
    return sets


def group_velocities(d, grad, direction, tolerance=1e-4, cutoff=1e-3):
    """(frequencies [n] THz, v [n, 3] THz A, sets, W eigenvalues per set) of one q-point: within a set of several modes the
    eigenvectors are rotated to those of W = E_S^H (sum_alpha direction_alpha dD_alpha) E_S (ascending); then
    v[i, alpha] = Re(e_i^H dD_alpha e_i) THZ^2 / (2 f_i), exactly 0 below the cutoff."""
    lam, e = np.linalg.eigh(d)
    f = np.sign(lam) * np.sqrt(np.abs(lam)) * THZ
    n = np.asarray(direction, dtype=np.float64)
    n = n / np.linalg.norm(n)
    gdir = np.einsum("a,aij->ij", n, grad)
    sets = degenerate_sets(f, tolerance)
    v = np.zeros((len(f), 3))
    w_eigs = []
    for b, c in sets:
        es = e[:, b:c]
        if c - b > 1:
            w, u = np.linalg.eigh(es.conj().T @ gdir @ es)
            es = es @ u
            w_eigs.append(w)
        else:
            w_eigs.append(np.real(es.conj().T @ gdir @ es).reshape(1))
        for k in range(c - b):
            if f[b + k] >= cutoff:
                v[b + k] = [np.real(es[:, k].conj() @ grad[a] @ es[:, k]) * THZ ** 2 / (2 * f[b + k]) for a in range(3)]
    return f, v, sets, w_eigs


def set_traces(v, sets):
    """[len(sets), 3]: the sum of v over each set -- independent of the basis chosen inside the set."""
    return np.array([v[b:c].sum(axis=0) for b, c in sets])


def set_projectors(e, sets):
    """E_S E_S^H of every set."""
    return [e[:, b:c] @ e[:, b:c].conj().T for b, c in sets]


def projection_weights(e, n_atoms):
    """[n_atoms, modes]: sum_a |e_ua|^2 of each mode (columns of e)."""
    return (np.abs(e) ** 2).reshape(n_atoms, 3, -1).sum(axis=1)
