"""numpy fp64 restatement of the batched finite-strain elastic constants and equation of state, one structure at a time: the yardstick
of torch_m3gnet.elasticity / m3g_el_* (tests/test_elastic_cpu.py, tests/test_gpu_elastic.py).

Conventions (include/m3gnet_hip.h): rows of a lattice are lattice vectors, L' = L D, r' = r D, D = I + eps symmetric; Voigt order
xx, yy, zz, yz, zx, xy; sigma = -(pair-virial stresses) = (1/V) dE/d eps, tension positive.  Where the GPU tests compare bits (the
deformed rows and cells, the slopes of the 36 lines) the operations are written in the kernels' order, one rounding per operation:
    r'_c = (r_0 D_0c + r_1 D_1c) + r_2 D_2c
    line through (0, y_0) and (d_m, y_m) in copy order: xb = sum x / n, yb = sum y / n, slope = sum (x - xb)(y - yb) / sum (x - xb)^2
Everything derived from the slopes (inverse, moduli, eigenvalues) and the EOS fit follow the kernels' algorithms (Gauss-Jordan with
partial pivoting, cyclic Jacobi, Householder QR) and are compared to 1e-12."""
from __future__ import annotations

import numpy as np

VOLUMETRIC = 6
VOIGT = ((0, 0), (1, 1), (2, 2), (1, 2), (2, 0), (0, 1))
EV_A3_TO_GPA = 160.21766208


def elastic_set(norm=(-0.01, -0.005, 0.005, 0.01), shear=(-0.06, -0.03, 0.03, 0.06)):
    comp = [j for j in range(3) for _ in norm] + [j for j in range(3, 6) for _ in shear]
    return np.array(comp), np.array(list(norm) * 3 + list(shear) * 3, dtype=np.float64)


def eos_set(strains=np.linspace(-0.05, 0.05, 11)):
    s = np.asarray(strains, dtype=np.float64)
    s = s[np.abs(s) > 1e-14]
    return np.full(len(s), VOLUMETRIC), s


def deformation_matrices(components, magnitudes) -> np.ndarray:
    """[1 + M, 3, 3]: D_0 = I, then D_m = I + eps_m."""
    out = [np.eye(3)]
    for c, d in zip(components, magnitudes):
        D = np.eye(3)
        if c == VOLUMETRIC:
            D[0, 0] = D[1, 1] = D[2, 2] = 1.0 + d
        elif c < 3:
            D[c, c] = 1.0 + d
        else:
            a, b = VOIGT[c]
            D[a, b] = D[b, a] = 0.5 * d
        out.append(D)
    return np.array(out)


def apply(rows, D) -> np.ndarray:
    r = np.asarray(rows, dtype=np.float64).reshape(-1, 3)
    return (r[:, 0:1] * D[0][None] + r[:, 1:2] * D[1][None]) + r[:, 2:3] * D[2][None]


def deformed(lattice, pos, components, magnitudes):
    """(rows [(1 + M) n, 3], cells [1 + M, 3, 3]) of the deformed copies of one structure."""
    Ds = deformation_matrices(components, magnitudes)
    return np.concatenate([apply(pos, D) for D in Ds]), np.array([apply(lattice, D) for D in Ds])


def fit_lines(sigma, components, magnitudes):
    """(C_raw [6,6], residuals [6,6]) from sigma [1 + M, 6] (copy 0 first)."""
    sigma = np.asarray(sigma, dtype=np.float64)
    craw, resid = np.zeros((6, 6)), np.zeros((6, 6))
    for i in range(6):
        for j in range(6):
            xs, ys = [0.0], [float(sigma[0, i])]
            for m, (c, d) in enumerate(zip(components, magnitudes)):
                if c == j:
                    xs.append(float(d))
                    ys.append(float(sigma[m + 1, i]))
            n = len(xs)
            sx = 0.0
            for x in xs[1:]:
                sx += x
            sy = ys[0]
            for y in ys[1:]:
                sy += y
            xb, yb = sx / n, sy / n
            sxx = sxy = 0.0
            for x, y in zip(xs, ys):
                dx, dy = x - xb, y - yb
                sxx += dx * dx
                sxy += dx * dy
            slope = sxy / sxx
            icpt = yb - slope * xb
            craw[i, j] = slope
            resid[i, j] = max(abs(y - (icpt + slope * x)) for x, y in zip(xs, ys))
    return craw, resid


def invert6(a) -> np.ndarray:
    a = np.array(a, dtype=np.float64)
    n = len(a)
    inv = np.eye(n)
    for k in range(n):
        piv = k + int(np.argmax(np.abs(a[k:, k])))
        if piv != k:
            a[[k, piv]] = a[[piv, k]]
            inv[[k, piv]] = inv[[piv, k]]
        d = 1.0 / a[k, k]
        a[k] *= d
        inv[k] *= d
        for i in range(n):
            if i != k:
                f = a[i, k]
                a[i] -= f * a[k]
                inv[i] -= f * inv[k]
    return inv


def jacobi_eigenvalues(a, sweeps=30) -> np.ndarray:
    """Ascending eigenvalues of a symmetric matrix by cyclic Jacobi, sweeps over (p, q), p < q, row-major."""
    a = np.array(a, dtype=np.float64)
    n = len(a)
    for _ in range(sweeps):
        off = sum(a[p, q] ** 2 for p in range(n) for q in range(p + 1, n))
        if not off > 1e-60 * (np.diag(a) ** 2).sum():
            break
        for p in range(n - 1):
            for q in range(p + 1, n):
                apq = a[p, q]
                if apq == 0.0:
                    continue
                theta = (a[q, q] - a[p, p]) / (2.0 * apq)
                t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                cp, cq = a[:, p].copy(), a[:, q].copy()
                a[:, p], a[:, q] = c * cp - s * cq, s * cp + c * cq
                rp, rq = a[p].copy(), a[q].copy()
                a[p], a[q] = c * rp - s * rq, s * rp + c * rq
    return np.sort(np.diag(a))


def moduli(C) -> dict:
    """Everything m3g_el_fit_elastic derives from the symmetric C (eV/A^3)."""
    C = np.asarray(C, dtype=np.float64)
    S = invert6(C)
    c_d, c_o, c_s = C[0, 0] + C[1, 1] + C[2, 2], C[0, 1] + C[1, 2] + C[0, 2], C[3, 3] + C[4, 4] + C[5, 5]
    s_d, s_o, s_s = S[0, 0] + S[1, 1] + S[2, 2], S[0, 1] + S[1, 2] + S[0, 2], S[3, 3] + S[4, 4] + S[5, 5]
    kv, gv = (c_d + 2.0 * c_o) / 9.0, (c_d - c_o + 3.0 * c_s) / 15.0
    kr, gr = 1.0 / (s_d + 2.0 * s_o), 15.0 / (4.0 * s_d - 4.0 * s_o + 3.0 * s_s)
    kh, gh = 0.5 * (kv + kr), 0.5 * (gv + gr)
    eig = jacobi_eigenvalues(C)
    return {"compliance": S, "k_voigt": kv, "k_reuss": kr, "k_hill": kh, "g_voigt": gv, "g_reuss": gr, "g_hill": gh,
            "youngs_modulus": 9.0 * kh * gh / (3.0 * kh + gh), "poisson_ratio": (3.0 * kh - 2.0 * gh) / (2.0 * (3.0 * kh + gh)),
            "universal_anisotropy": 5.0 * gv / gr + kv / kr - 6.0, "eigenvalues": eig, "stable": bool(eig[0] > 0.0)}


def elastic_fit(sigma, components, magnitudes) -> dict:
    """What one row of m3g_el_fit_elastic holds, from sigma [1 + M, 6]."""
    sigma = np.asarray(sigma, dtype=np.float64)
    if not np.isfinite(sigma).all():
        return {"nonfinite": int((~np.isfinite(sigma)).sum())}
    craw, resid = fit_lines(sigma, components, magnitudes)
    C = 0.5 * (craw + craw.T)
    return {"nonfinite": 0, "C_raw": craw, "C": C, "asymmetry": float(np.abs(craw - craw.T).max()), "fit_residual": float(resid.max()),
            "residual_stress": sigma[0].copy(), **moduli(C)}


def householder_lstsq(A, b) -> np.ndarray:
    A, b = np.array(A, dtype=np.float64), np.array(b, dtype=np.float64)
    n, k = A.shape
    for j in range(k):
        nrm = np.sqrt((A[j:, j] ** 2).sum())
        alpha = -nrm if A[j, j] > 0.0 else nrm
        v = A[j:, j].copy()
        v[0] -= alpha
        vv = (v * v).sum()
        for c in range(j + 1, k):
            A[j:, c] -= 2.0 * (v * A[j:, c]).sum() / vv * v
        b[j:] -= 2.0 * (v * b[j:]).sum() / vv * v
        A[j:, j] = 0.0
        A[j, j] = alpha
    x = np.zeros(k)
    for j in range(k - 1, -1, -1):
        x[j] = (b[j] - (A[j, j + 1:] * x[j + 1:]).sum()) / A[j, j]
    return x


def eos_fit(v_ref, strains, energies) -> dict:
    """What one row of m3g_el_fit_eos holds: `strains` [M] linear strains of copies 1..M, `energies` [1 + M] (copy 0 first)."""
    e = np.asarray(energies, dtype=np.float64)
    s = np.asarray(strains, dtype=np.float64)
    if not np.isfinite(e).all():
        return {"error": 1}
    t = np.concatenate([[0.0], 1.0 / ((1.0 + s) * (1.0 + s)) - 1.0])
    ts = np.abs(t).max()
    u = t / ts
    c = householder_lstsq(np.stack([np.ones_like(u), u, u * u, u * u * u], axis=1), e - e[0])
    poly = lambda x: ((c[3] * x + c[2]) * x + c[1]) * x + c[0]
    out = {"error": 0, "rms_residual": float(np.sqrt(((poly(u) - (e - e[0])) ** 2).sum() / len(e))), "v_ref": float(v_ref), "n": len(e)}
    u0 = np.nan
    disc = c[2] * c[2] - 3.0 * c[3] * c[1]
    if abs(c[3]) <= 1e-14 * abs(c[2]):
        if c[2] > 0:
            u0 = -c[1] / (2.0 * c[2])
    elif disc > 0:
        q = -(c[2] + (np.sqrt(disc) if c[2] >= 0 else -np.sqrt(disc)))
        roots = [r for r in (q / (3.0 * c[3]), c[1] / q) if 2.0 * c[2] + 6.0 * c[3] * r > 0]
        if roots:
            u0 = min(roots, key=abs)
    t0 = u0 * ts
    if not (t.min() <= t0 <= t.max()):
        out["error"] = 2
        return out
    g = 1.0 + t0
    v0 = v_ref / (g * np.sqrt(g))
    e2, e3 = (2.0 * c[2] + 6.0 * c[3] * u0) / ts ** 2, 6.0 * c[3] / ts ** 3
    a2, a3 = 0.5 * e2 * g * g, e3 * g ** 3 / 6.0
    out.update(v0=float(v0), e0=float(e[0] + poly(u0)), b0=float(8.0 * a2 / (9.0 * v0)), b0_prime=float(4.0 + 2.0 * a3 / a2), t0=float(t0))
    return out


def birch_murnaghan(v, v0, e0, b0, b0p):
    y = (v0 / np.asarray(v, dtype=np.float64)) ** (2.0 / 3.0) - 1.0
    return e0 + 9.0 * v0 * b0 / 16.0 * (y ** 3 * b0p + y ** 2 * (6.0 - 4.0 * (y + 1.0)))


def voigt6(w) -> np.ndarray:
    return np.array([w[a][b] for a, b in VOIGT])


def evaluate_copies(lattice, pos, components, magnitudes, energy_forces_virial, relax_atoms=False, fmax=1e-3, steps=2000):
    """(energies [1 + M], sigma [1 + M, 6], converged [1 + M]) of the deformed copies under `energy_forces_virial(pos, lattice) ->
    (E, forces, W = -dE/d eps)`, the ions of every copy relaxed with tests/fire_reference.py at fixed cell when `relax_atoms`."""
    import fire_reference as fr

    n = len(np.asarray(pos).reshape(-1, 3))
    rows, cells = deformed(lattice, pos, components, magnitudes)
    e, sg, ok = [], [], []
    for c, L in enumerate(cells):
        p = rows[c * n:(c + 1) * n]
        if relax_atoms:
            ref, ev = fr.relax(p, L, energy_forces_virial, relax_cell=False, fmax=fmax, steps=steps)
            ok.append(ref.converged)
        else:
            ev = energy_forces_virial(p, L)
            ok.append(True)
        e.append(ev[0])
        sg.append(-voigt6(ev[2]) / abs(np.linalg.det(L)))
    return np.array(e), np.array(sg), np.array(ok)
