// The library's Hermitian eigensolver for small matrices: cyclic Jacobi with complex rotations in fp64 over a matrix in LDS
// (include/m3gnet_hip.h, "batched Hermitian eigensolver").  A device function, called by the batched kernel (m3g_eigh.hip: one
// workgroup per matrix) and by the group-velocity kernel (m3g_phonons.hip: on the blocks W of degenerate sets).
//
// Order: the round-robin (circle) pairing of m = n rounded up to even players, m - 1 rounds of m / 2 disjoint pairs per sweep:
// player m - 1 stays, round r pairs it with r, and (r + k) mod (m - 1) with (r - k) mod (m - 1), k = 1 .. m / 2 - 1; a pair with
// an index >= n (odd n) sits the round out.  The pairs of a round touch disjoint rows and columns, so a round is three phases over
// the workgroup: the rotations from the matrix as it stands, every column pair (A J and V J), every row pair (J^H A).  Every
// element is updated by one thread from LDS values only, so the result does not depend on the number of threads.
//
// Rotation of (p, q), g = a_pq = |g| w: theta = (a_qq - a_pp) / (2 |g|), t = sign(theta) / (|theta| + sqrt(theta^2 + 1)),
// c = 1 / sqrt(t^2 + 1), s = t c, J = [[c, s w], [-s conj(w), c]]; a_pp -= t |g|, a_qq += t |g|, a_pq = 0 are written as such.
// Skipped when |g| <= DBL_EPSILON ||H||_F / n, the norm taken once up front over the entries read (not the relative criterion
// against sqrt(|a_pp a_qq|): that one cannot settle the zero eigenvalues of a Gamma-point dynamical matrix).
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>

#include "m3g_internal.h"

namespace m3g {
constexpr int kEighMaxN = M3G_EIGH_MAX_N;
constexpr int kEighMaxSweeps = M3G_EIGH_MAX_SWEEPS;

// LDS scratch of one solve, n <= NCAP
template <int NCAP>
struct EighScratch {
  double rot[6 * ((NCAP + 1) / 2)];   // per pair of the round: c, s, Re w, Im w (s == 0: skipped), the new a_pp and a_qq
  double d[NCAP];                     // row norms first, the eigenvalues in index order at the end
  double norm;
  int order[NCAP];                    // order[k]: the index of the k-th smallest eigenvalue (stable)
  int rotated, bad;
};

// Pair k of round r for m players (m even): p < q.
__device__ inline void eigh_pair(int m, int r, int k, int& p, int& q) {
  int a, b;
  if (k == 0) {
    a = m - 1;
    b = r;
  } else {
    a = (r + k) % (m - 1);
    b = (r - k + (m - 1)) % (m - 1);
  }
  p = a < b ? a : b;
  q = a < b ? b : a;
}

// Diagonalises the Hermitian n x n matrix A (LDS, interleaved complex, row-major, leading dimension n; the upper triangle and the
// real part of the diagonal are read, the whole of it is overwritten).  V (LDS, same layout) receives the eigenvectors as columns in
// INDEX order, or is nullptr.  On return sc.d[i] is eigenvalue i, sc.order the ascending stable order, and the value returned (the
// same in every thread) is the info word.  A flagged matrix: sc.d is NaN, V is not defined.  Every thread of the workgroup must
// call it (it synchronises); tid in [0, nthreads).
template <int NCAP>
__device__ inline int eigh_jacobi_lds(double* A, double* V, int n, EighScratch<NCAP>& sc, int tid, int nthreads) {
#pragma clang fp contract(off)
  // mirror the upper triangle, drop the diagonal's imaginary part, V = I, the row norms and the finiteness of what is read
  if (tid == 0) { sc.bad = 0; sc.rotated = 0; }
  __syncthreads();
  for (int i = tid; i < n; i += nthreads) {
    double sum = 0.0;
    bool bad = false;
    const double dii = A[2 * (i * n + i)];
    bad = bad || !std::isfinite(dii);
    sum += dii * dii;
    A[2 * (i * n + i) + 1] = 0.0;
    for (int j = i + 1; j < n; ++j) {
      const double re = A[2 * (i * n + j)], im = A[2 * (i * n + j) + 1];
      bad = bad || !std::isfinite(re) || !std::isfinite(im);
      sum += 2.0 * (re * re + im * im);
      A[2 * (j * n + i)] = re;
      A[2 * (j * n + i) + 1] = -im;
    }
    sc.d[i] = sum;
    if (bad) sc.bad = 1;   // (every writer writes the same value)
  }
  if (V != nullptr)
    for (int e = tid; e < n * n; e += nthreads) {
      V[2 * e] = (e / n == e % n) ? 1.0 : 0.0;
      V[2 * e + 1] = 0.0;
    }
  __syncthreads();
  if (tid == 0) {
    double sum = 0.0;
    for (int i = 0; i < n; ++i) sum += sc.d[i];
    sc.norm = sqrt(sum);
    if (!std::isfinite(sc.norm)) sc.bad = 1;
  }
  __syncthreads();
  int info = 0;
  if (sc.bad) {
    info = M3G_EIGH_NONFINITE;
  } else {
    const double threshold = DBL_EPSILON * sc.norm / (double)n;
    const int m = (n + 1) & ~1, half = m / 2;
    int sweeps = 0;
    bool converged = (n == 1);
    for (int sweep = 0; sweep < kEighMaxSweeps && !converged; ++sweep) {   // (an integer bound: no comparison a NaN could defeat)
      for (int r = 0; r < m - 1; ++r) {
        // phase 0: the rotations of the round
        for (int k = tid; k < half; k += nthreads) {
          int p, q;
          eigh_pair(m, r, k, p, q);
          double c = 1.0, s = 0.0, wr = 1.0, wi = 0.0;
          if (q < n) {
            const double gr = A[2 * (p * n + q)], gi = A[2 * (p * n + q) + 1];
            const double g = hypot(gr, gi);
            if (g > threshold) {
              const double app = A[2 * (p * n + p)], aqq = A[2 * (q * n + q)];
              const double theta = (aqq - app) / (2.0 * g);
              const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
              c = 1.0 / sqrt(t * t + 1.0);
              s = t * c;
              wr = gr / g;
              wi = gi / g;
              if (s != 0.0) {
                sc.rotated = 1;
                sc.rot[6 * k + 4] = app - t * g;
                sc.rot[6 * k + 5] = aqq + t * g;
              } else {   // the rotation is the identity to working precision: the entry is below what the diagonal gap resolves
                A[2 * (p * n + q)] = 0.0; A[2 * (p * n + q) + 1] = 0.0;
                A[2 * (q * n + p)] = 0.0; A[2 * (q * n + p) + 1] = 0.0;
              }
            }
          }
          sc.rot[6 * k] = c; sc.rot[6 * k + 1] = s; sc.rot[6 * k + 2] = wr; sc.rot[6 * k + 3] = wi;
        }
        __syncthreads();
        // phase 1: columns, X[i, p] = c X[i, p] - s conj(w) X[i, q], X[i, q] = s w X[i, p] + c X[i, q] for X = A and V
        for (int e = tid; e < half * n; e += nthreads) {
          const int k = e % half, i = e / half;
          const double s = sc.rot[6 * k + 1];
          if (s == 0.0) continue;
          const double c = sc.rot[6 * k], wr = sc.rot[6 * k + 2], wi = sc.rot[6 * k + 3];
          int p, q;
          eigh_pair(m, r, k, p, q);
          const double swr = s * wr, swi = s * wi;
          for (int which = 0; which < 2; ++which) {
            double* X = which == 0 ? A : V;
            if (X == nullptr) continue;
            double* xp = X + 2 * (i * n + p);
            double* xq = X + 2 * (i * n + q);
            const double pr = xp[0], pi = xp[1], qr = xq[0], qi = xq[1];
            // s conj(w) x_q = (swr - i swi)(qr + i qi); s w x_p = (swr + i swi)(pr + i pi)
            xp[0] = c * pr - (swr * qr + swi * qi);
            xp[1] = c * pi - (swr * qi - swi * qr);
            xq[0] = (swr * pr - swi * pi) + c * qr;
            xq[1] = (swr * pi + swi * pr) + c * qi;
          }
        }
        __syncthreads();
        // phase 2: rows, A[p, j] = c A[p, j] - s w A[q, j], A[q, j] = s conj(w) A[p, j] + c A[q, j]; then the 2 x 2 block as such
        for (int e = tid; e < half * n; e += nthreads) {
          const int j = e % n, k = e / n;
          const double s = sc.rot[6 * k + 1];
          if (s == 0.0) continue;
          const double c = sc.rot[6 * k], wr = sc.rot[6 * k + 2], wi = sc.rot[6 * k + 3];
          int p, q;
          eigh_pair(m, r, k, p, q);
          const double swr = s * wr, swi = s * wi;
          double* ap = A + 2 * (p * n + j);
          double* aq = A + 2 * (q * n + j);
          const double pr = ap[0], pi = ap[1], qr = aq[0], qi = aq[1];
          ap[0] = c * pr - (swr * qr - swi * qi);
          ap[1] = c * pi - (swr * qi + swi * qr);
          aq[0] = (swr * pr + swi * pi) + c * qr;
          aq[1] = (swr * pi - swi * pr) + c * qi;
        }
        __syncthreads();
        for (int k = tid; k < half; k += nthreads) {
          const double s = sc.rot[6 * k + 1];
          if (s == 0.0) continue;
          int p, q;
          eigh_pair(m, r, k, p, q);
          // the diagonal from the rotation's own formula (more exact than the two products), the pair's entry exactly zero
          A[2 * (p * n + p)] = sc.rot[6 * k + 4]; A[2 * (p * n + p) + 1] = 0.0;
          A[2 * (q * n + q)] = sc.rot[6 * k + 5]; A[2 * (q * n + q) + 1] = 0.0;
          A[2 * (p * n + q)] = 0.0; A[2 * (p * n + q) + 1] = 0.0;
          A[2 * (q * n + p)] = 0.0; A[2 * (q * n + p) + 1] = 0.0;
        }
        __syncthreads();
      }
      sweeps = sweep + 1;
      converged = sc.rotated == 0;
      __syncthreads();
      if (tid == 0) sc.rotated = 0;
      __syncthreads();
    }
    info = sweeps | (converged ? 0 : M3G_EIGH_NOT_CONVERGED);
  }
  const bool failed = (info & ~M3G_EIGH_SWEEPS_MASK) != 0;
  for (int i = tid; i < n; i += nthreads) {
    sc.d[i] = failed ? (double)NAN : A[2 * (i * n + i)];
    sc.order[i] = i;   // (every entry defined whatever the ranks below: a NaN on the diagonal ranks nowhere)
  }
  __syncthreads();
  // stable ascending order by rank counting
  for (int i = tid; i < n; i += nthreads) {
    int rank = 0;
    if (!failed) {
      const double di = sc.d[i];
      for (int j = 0; j < n; ++j) rank += (sc.d[j] < di || (sc.d[j] == di && j < i)) ? 1 : 0;
    } else {
      rank = i;
    }
    sc.order[rank] = i;
  }
  __syncthreads();
  return info;
}
}  // namespace m3g
