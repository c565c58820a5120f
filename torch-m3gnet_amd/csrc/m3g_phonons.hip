// Batched finite-displacement phonons (phonopy's method: diagonal supercell, no symmetry reduction; phonopy's
// produce_force_constants / get_dynamical_matrix_at_q over an ASE calculator).  Without it, every displaced supercell is one host
// round trip to a calculator.  Here the displaced supercells of every structure of a batch are one batch of the engine, and the three
// stages around that evaluation are one launch each:
//   k_ph_displace          a thread per row of the displaced batch: the supercell position of the row, written from the unit cells in
//                          the state straight into the fp64 `pos` the engine reads;
//   k_ph_force_constants   one workgroup per (structure, home atom u): Phi[u, j] from the + and - force rows of u's six displaced
//                          copies, the nine row sums over j (lane-strided, then a fixed tree), the ASR self term, and the count of
//                          non-finite forces of the whole structure (every workgroup of the structure counts the same rows in the same
//                          order; a structure with one gets NaN force constants);
//   k_ph_dynmat            a thread per (q, u <= v): the two 3x3 blocks D(u,v), D(v,u) over the image table (one sincospi per image for
//                          all nine entries, q.d reduced mod 1 first), mass weighting, Hermitisation, blocks (u,v) and (v,u) written.
// On top of the dynamical matrices, for eigenvectors from the library's Hermitian solver (m3g_eigh.h; phonopy's GroupVelocity over
// DerivativeOfDynamicalMatrix):
//   k_ph_dynmat<true>      the thread map of k_ph_dynmat, three workgroups (alpha) for each of its own: dD / dq_alpha for the Cartesian
//                          q (1/A, no 2 pi) -- every image term times 2 pi i r_alpha -- through the same dyn_block;
//   k_ph_group_velocities  one workgroup per q-point: degenerate sets rotated to the eigenvectors of their block of the derivative
//                          along `direction`, v = Re(e^H dD_alpha e) THZ^2 / (2 f), lane-strided sums and the fixed tree.
// No atomics: every result depends on its structure's own inputs only, so it is bitwise the same alone or in any batch.  No allocation,
// copy or wait in the compute calls (capture-safe).
//
// Layouts (structure s: n_u unit atoms, supercell n1 x n2 x n3, N_s = n_u n1 n2 n3 supercell atoms).  Supercell atom j = l n_u + b with
// l = (l1 n2 + l2) n3 + l3, at r_b + l1 L_0 + l2 L_1 + l3 L_2.  The displaced batch holds per structure 1 + 6 n_u copies of N_s rows:
// copy 0 undisplaced, copy 1 + 6u + 2a + k the home atom u (j = u) moved by +delta (k = 0) or -delta (k = 1) along axis a.
// Phi [sum_s n_u N_s, 3, 3]: structure s from 9 pair_off[s], row u N_s + j.
#include <cmath>
#include <vector>

#include "m3g_chunks.h"
#include "m3g_eigh.h"
#include "m3g_internal.h"

namespace m3g {
namespace {
constexpr int kMaxMult = M3G_PH_MAX_MULTIPLICITY;   // shortest images per (u, j) pair kept in the table
constexpr int kFcThreads = kChunkRows;   // the workgroup of chunk_tree_reduce (m3g_chunks.h)
constexpr int kDynThreads = 64;

struct PhView {
  int64_t S, U, rows;
  const int64_t *row_off, *unit_off, *pair_off;   // [S+1]: displaced rows, unit atoms, (u, j) pairs
  const int32_t* dims;                            // [S, 3]
  const double* lat;                              // [S, 9] rows = lattice vectors
  const double* unit_pos;                         // [U, 3]
  const double* mass;                             // [U]
  const int32_t* unit_struct;                     // [U]
  const double* delta;                            // [1]
  const int32_t* img_count;                       // [P]
  const double* img_d;                            // [P, kMaxMult, 3] unit-cell fractional
};
Carved<PhView> ph_view(const m3g_ph_sizes& z, const void* state) {
  Carve c{state};
  const int64_t S = z.n_structs, U = z.n_unit_atoms, P = z.n_pairs;
  PhView st{S, U, 6 * P + z.n_super_atoms};
  st.row_off = c.take<int64_t>(S + 1);
  st.unit_off = c.take<int64_t>(S + 1);
  st.pair_off = c.take<int64_t>(S + 1);
  st.dims = c.take<int32_t>(3 * S);
  st.lat = c.take<double>(9 * S);
  st.unit_pos = c.take<double>(3 * U);
  st.mass = c.take<double>(U);
  st.unit_struct = c.take<int32_t>(U);
  st.delta = c.take<double>(1);
  st.img_count = c.take<int32_t>(P);
  st.img_d = c.take<double>(3 * kMaxMult * P);
  return {st, c.off};
}

__global__ void __launch_bounds__(256) k_ph_displace(PhView st, double* __restrict__ pos) {
#pragma clang fp contract(off)
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= st.rows) return;
  int64_t lo = 0, hi = st.S - 1;   // the structure of row r: the last s with row_off[s] <= r
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) / 2;
    if (st.row_off[mid] <= r) lo = mid; else hi = mid - 1;
  }
  const int64_t s = lo;
  const int64_t nu = st.unit_off[s + 1] - st.unit_off[s];
  const int n1 = st.dims[3 * s], n2 = st.dims[3 * s + 1], n3 = st.dims[3 * s + 2];
  const int64_t ns = nu * n1 * n2 * n3;
  const int64_t local = r - st.row_off[s];
  const int64_t copy = local / ns, j = local % ns;
  const int64_t l = j / nu, b = j % nu;
  const double l1 = (double)(l / ((int64_t)n2 * n3)), l2 = (double)((l / n3) % n2), l3 = (double)(l % n3);
  const double* L = st.lat + 9 * s;
  const double* rb = st.unit_pos + 3 * (st.unit_off[s] + b);
  double x[3];
  for (int c = 0; c < 3; ++c) {
    double t = l1 * L[c];
    t = t + l2 * L[3 + c];
    t = t + l3 * L[6 + c];
    x[c] = rb[c] + t;
  }
  if (copy > 0) {
    const int64_t k = copy - 1, u = k / 6;
    const int a = (int)((k % 6) / 2);
    if (j == u) x[a] = (k % 2 == 0) ? x[a] + st.delta[0] : x[a] - st.delta[0];
  }
  for (int c = 0; c < 3; ++c) pos[3 * r + c] = x[c];
}

__global__ void __launch_bounds__(kFcThreads) k_ph_force_constants(PhView st, const float* __restrict__ forces, int asr,
                                                                    double* __restrict__ phi, double* __restrict__ sums,
                                                                    int32_t* __restrict__ nonfinite) {
#pragma clang fp contract(off)
  __shared__ double sh[10][kFcThreads];
  const int64_t g = blockIdx.x;   // global unit atom = (structure, home atom)
  const int t = threadIdx.x;
  const int s = st.unit_struct[g];
  const int64_t u = g - st.unit_off[s];
  const int64_t nu = st.unit_off[s + 1] - st.unit_off[s];
  const int64_t ns = nu * st.dims[3 * s] * st.dims[3 * s + 1] * st.dims[3 * s + 2];
  const int64_t r0 = st.row_off[s];
  const double two_delta = 2.0 * st.delta[0];
  double acc[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // the nine row sums, then the non-finite count
  // non-finite forces anywhere in the structure's 1 + 6 n_u copies (the same count in every workgroup of the structure)
  const int64_t nvals = 3 * (st.row_off[s + 1] - r0);
  for (int64_t i = t; i < nvals; i += kFcThreads) acc[9] += std::isfinite(forces[3 * r0 + i]) ? 0.0 : 1.0;
  const int64_t plus0 = r0 + (1 + 6 * u) * ns;   // first row of copy (u, a = 0, +)
  double* out = phi + 9 * (st.pair_off[s] + u * ns);
  for (int64_t j = t; j < ns; j += kFcThreads) {
    for (int a = 0; a < 3; ++a) {
      const float* fp = forces + 3 * (plus0 + 2 * a * ns + j);
      const float* fm = forces + 3 * (plus0 + (2 * a + 1) * ns + j);
      for (int c = 0; c < 3; ++c) {
        const double v = -((double)fp[c] - (double)fm[c]) / two_delta;
        acc[3 * a + c] += v;
        if (!(asr && j == u)) out[9 * j + 3 * a + c] = v;
      }
    }
  }
  chunk_tree_reduce<10>(sh, acc, t);   // (the order depends on the thread index only)
  const bool failed = sh[9][0] != 0.0;
  if (t < 9) {
    const int a = t / 3, c = t % 3;
    sums[9 * g + t] = sh[t][0];
    if (asr) {
      const float* fp = forces + 3 * (plus0 + 2 * a * ns + u);
      const float* fm = forces + 3 * (plus0 + (2 * a + 1) * ns + u);
      const double self = -((double)fp[c] - (double)fm[c]) / two_delta;
      out[9 * u + t] = self - sh[t][0];
    }
  }
  if (t == 0 && u == 0) nonfinite[s] = (int32_t)sh[9][0];
  if (failed) {
    __syncthreads();   // (failed is uniform over the workgroup)
    for (int64_t i = t; i < 9 * ns; i += kFcThreads) out[i] = NAN;
    if (t < 9) sums[9 * g + t] = NAN;
  }
}

// the 3x3 block sum_l sum_m w_m Phi[u, l n_u + v] exp(2 pi i q.d_m) of structure s (re, im); kGrad: every image term times
// 2 pi i r_alpha, r = d L the Cartesian image vector -- the derivative with respect to the Cartesian q_alpha (1/A, no 2 pi)
template <bool kGrad = false>
__device__ inline void dyn_block(const PhView& st, const double* __restrict__ phi, int64_t s, int64_t u, int64_t v, int64_t nu,
                                 int64_t ns, const double q[3], double re[9], double im[9], int alpha = 0) {
  for (int k = 0; k < 9; ++k) re[k] = im[k] = 0.0;
  const int64_t row = st.pair_off[s] + u * ns;
  for (int64_t j = v; j < ns; j += nu) {
    const int64_t p = row + j;
    const int m = st.img_count[p];
    const double* d = st.img_d + 3 * kMaxMult * p;
    double wc = 0.0, ws = 0.0;
    for (int i = 0; i < m; ++i) {
      const double x = q[0] * d[3 * i] + q[1] * d[3 * i + 1] + q[2] * d[3 * i + 2];
      const double y = x - rint(x);   // q.d mod 1, in [-1/2, 1/2]
      double sn, cs;
      sincospi(2.0 * y, &sn, &cs);
      if constexpr (kGrad) {   // 2 pi i r (cs + i sn)
        const double* L = st.lat + 9 * s;
        const double r = 2.0 * M_PI * (d[3 * i] * L[alpha] + d[3 * i + 1] * L[3 + alpha] + d[3 * i + 2] * L[6 + alpha]);
        wc -= r * sn;
        ws += r * cs;
      } else {
        wc += cs;
        ws += sn;
      }
    }
    const double w = 1.0 / (double)m;
    wc *= w;
    ws *= w;
    const double* f = phi + 9 * p;
    for (int k = 0; k < 9; ++k) {
      re[k] += f[k] * wc;
      im[k] += f[k] * ws;
    }
  }
}

// kGrad: the grid holds three workgroups (alpha = 0, 1, 2) for each one of the plain kernel, out is [Q, 3, dim, dim]
template <bool kGrad>
__global__ void __launch_bounds__(kDynThreads) k_ph_dynmat(PhView st, int64_t n_q, int64_t blocks_per_q, const double* __restrict__ qs,
                                                           const int32_t* __restrict__ q_struct, int32_t max_nu,
                                                           const double* __restrict__ phi, double* __restrict__ out) {
  const int64_t slot = kGrad ? blockIdx.x / 3 : blockIdx.x;
  const int alpha = kGrad ? (int)(blockIdx.x % 3) : 0;
  const int64_t q_i = slot / blocks_per_q;
  const int64_t p = (slot % blocks_per_q) * kDynThreads + threadIdx.x;
  if (q_i >= n_q) return;
  const int64_t s = q_struct[q_i];
  if (s < 0 || s >= st.S) return;
  const int64_t nu = st.unit_off[s + 1] - st.unit_off[s];
  if (nu > max_nu || p >= nu * (nu + 1) / 2) return;
  int64_t u = 0, rem = p;   // p -> (u, v), u <= v, row-major over the upper triangle
  while (rem >= nu - u) { rem -= nu - u; ++u; }
  const int64_t v = u + rem;
  const int64_t ns = nu * st.dims[3 * s] * st.dims[3 * s + 1] * st.dims[3 * s + 2];
  const double q[3] = {qs[3 * q_i], qs[3 * q_i + 1], qs[3 * q_i + 2]};
  const double* m = st.mass + st.unit_off[s];
  const double inv = 1.0 / sqrt(m[u] * m[v]);
  double are[9], aim[9], bre[9], bim[9];
  dyn_block<kGrad>(st, phi, s, u, v, nu, ns, q, are, aim, alpha);
  if (u != v) {
    dyn_block<kGrad>(st, phi, s, v, u, nu, ns, q, bre, bim, alpha);
  } else {
    for (int k = 0; k < 9; ++k) { bre[k] = are[k]; bim[k] = aim[k]; }
  }
  // H(u,v)[a][b] = (A[a][b] + conj(B[b][a])) / 2; H(v,u) = H(u,v)^H
  const int64_t dim = 3 * (int64_t)max_nu;
  double* o = out + 2 * dim * dim * (kGrad ? 3 * q_i + alpha : q_i);
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      const double hr = 0.5 * (are[3 * a + b] + bre[3 * b + a]) * inv;
      const double hi = 0.5 * (aim[3 * a + b] - bim[3 * b + a]) * inv;
      const int64_t ia = 3 * u + a, jb = 3 * v + b;
      o[2 * (ia * dim + jb)] = hr;
      o[2 * (ia * dim + jb) + 1] = hi;
      o[2 * (jb * dim + ia)] = hr;
      o[2 * (jb * dim + ia) + 1] = -hi;
    }
}

// Group velocities of one q-point per workgroup (include/m3gnet_hip.h, "phonon group velocities").  Degenerate sets one after the
// other, in LDS only the set's eigenvectors X [m][n], a second block Y [m][n] (G_dir X first, then the rotated X U) and the
// m x m blocks W and U: 512 n bytes of dynamic LDS for kGvSet = 16, whatever the width of the matrix.
constexpr int kGvSet = M3G_PH_GV_MAX_SET;
constexpr int kGvThreads = kChunkRows;
inline size_t gv_lds_bytes(int n) { return sizeof(double) * ((size_t)4 * n * kGvSet + n); }

__global__ void __launch_bounds__(kGvThreads) k_ph_group_velocities(int n, const double* __restrict__ lam, const double* __restrict__ E,
                                                                    const double* __restrict__ G, double tol, double cutoff, double d0,
                                                                    double d1, double d2, double* __restrict__ vout) {
#pragma clang fp contract(off)
  extern __shared__ double gv_lds[];
  __shared__ double W[2 * kGvSet * kGvSet];
  __shared__ double U[2 * kGvSet * kGvSet];
  __shared__ EighScratch<kGvSet> sc;
  __shared__ double sh[3][kGvThreads];
  __shared__ int bad;
  double* X = gv_lds;
  double* Y = X + 2 * (size_t)n * kGvSet;
  double* f = Y + 2 * (size_t)n * kGvSet;
  const int64_t q = blockIdx.x;
  const int t = threadIdx.x;
  const int64_t nn = (int64_t)n * n;
  const double* lq = lam + (int64_t)n * q;
  const double* Eq = E + 2 * nn * q;
  const double* Gq = G + 6 * nn * q;
  double* out = vout + 3 * (int64_t)n * q;
  constexpr double thz = M3G_PH_THZ;
  if (t == 0) bad = 0;
  __syncthreads();
  for (int i = t; i < n; i += kGvThreads) {
    const double l = lq[i];
    if (!std::isfinite(l)) bad = 1;   // (every writer writes the same value)
    f[i] = (l < 0.0 ? -1.0 : (l > 0.0 ? 1.0 : 0.0)) * sqrt(fabs(l)) * thz;
  }
  __syncthreads();
  if (bad) {   // (uniform over the workgroup)
    for (int i = t; i < 3 * n; i += kGvThreads) out[i] = NAN;
    return;
  }
  for (int begin = 0; begin < n;) {   // (every thread walks the same sets)
    int end = begin + 1;
    while (end < n && f[end] - f[end - 1] < tol) ++end;
    const int m = end - begin;
    if (m > kGvSet || f[end - 1] < cutoff) {   // too large a set: NaN; every mode of it below the cutoff: exactly 0
      const double fill = m > kGvSet ? (double)NAN : 0.0;
      for (int i = 3 * begin + t; i < 3 * end; i += kGvThreads) out[i] = fill;
      begin = end;
      continue;
    }
    for (int e = t; e < n * m; e += kGvThreads) {
      const int k = e / n, a = e % n;
      X[2 * e] = Eq[2 * ((int64_t)a * n + begin + k)];
      X[2 * e + 1] = Eq[2 * ((int64_t)a * n + begin + k) + 1];
    }
    __syncthreads();
    const double* Z = X;
    bool failed = false;
    if (m > 1) {
      for (int e = t; e < n * m; e += kGvThreads) {   // Y[k][a] = sum_b (sum_alpha d_alpha dD_alpha)[a, b] X[k][b]
        const int k = e / n, a = e % n;
        const double* g0 = Gq + 2 * (int64_t)a * n;
        const double* g1 = g0 + 2 * nn;
        const double* g2 = g1 + 2 * nn;
        const double* x = X + 2 * (size_t)k * n;
        double yr = 0.0, yi = 0.0;
        for (int b = 0; b < n; ++b) {
          const double gr = (d0 * g0[2 * b] + d1 * g1[2 * b]) + d2 * g2[2 * b];
          const double gi = (d0 * g0[2 * b + 1] + d1 * g1[2 * b + 1]) + d2 * g2[2 * b + 1];
          yr += gr * x[2 * b] - gi * x[2 * b + 1];
          yi += gr * x[2 * b + 1] + gi * x[2 * b];
        }
        Y[2 * e] = yr;
        Y[2 * e + 1] = yi;
      }
      __syncthreads();
      for (int e = t; e < m * m; e += kGvThreads) {   // W[j, k] = sum_a conj(X[j][a]) Y[k][a]
        const int j = e / m, k = e % m;
        const double* x = X + 2 * (size_t)j * n;
        const double* y = Y + 2 * (size_t)k * n;
        double wr = 0.0, wi = 0.0;
        for (int a = 0; a < n; ++a) {
          wr += x[2 * a] * y[2 * a] + x[2 * a + 1] * y[2 * a + 1];
          wi += x[2 * a] * y[2 * a + 1] - x[2 * a + 1] * y[2 * a];
        }
        W[2 * e] = wr;
        W[2 * e + 1] = wi;
      }
      __syncthreads();
      const int status = eigh_jacobi_lds<kGvSet>(W, U, m, sc, t, kGvThreads);
      failed = (status & ~M3G_EIGH_SWEEPS_MASK) != 0;
      for (int e = t; e < n * m; e += kGvThreads) {   // Y[k][a] = sum_j X[j][a] U[j, order[k]]
        const int k = e / n, a = e % n;
        const int col = sc.order[k];
        double yr = 0.0, yi = 0.0;
        for (int j = 0; j < m; ++j) {
          const double xr = X[2 * ((size_t)j * n + a)], xi = X[2 * ((size_t)j * n + a) + 1];
          const double ur = U[2 * (j * m + col)], ui = U[2 * (j * m + col) + 1];
          yr += xr * ur - xi * ui;
          yi += xr * ui + xi * ur;
        }
        Y[2 * e] = yr;
        Y[2 * e + 1] = yi;
      }
      __syncthreads();
      Z = Y;
    }
    for (int k = 0; k < m; ++k) {   // v[i, alpha] = Re(z^H dD_alpha z) thz^2 / (2 f_i): lane-strided over the rows, then the fixed tree
      const double* z = Z + 2 * (size_t)k * n;
      double acc[3] = {0.0, 0.0, 0.0};
      for (int a = t; a < n; a += kGvThreads)
        for (int c = 0; c < 3; ++c) {
          const double* g = Gq + 2 * (c * nn + (int64_t)a * n);
          double tr = 0.0, ti = 0.0;
          for (int b = 0; b < n; ++b) {
            tr += g[2 * b] * z[2 * b] - g[2 * b + 1] * z[2 * b + 1];
            ti += g[2 * b] * z[2 * b + 1] + g[2 * b + 1] * z[2 * b];
          }
          acc[c] += z[2 * a] * tr + z[2 * a + 1] * ti;
        }
      chunk_tree_reduce<3>(sh, acc, t);
      if (t < 3) {
        const double fi = f[begin + k];
        out[3 * (begin + k) + t] = failed ? (double)NAN : (fi < cutoff ? 0.0 : sh[t][0] * (thz * thz) / (2.0 * fi));
      }
      __syncthreads();
    }
    begin = end;
  }
}

bool ph_sizes_ok(const m3g_ph_sizes* z) {
  return z && z->n_structs >= 1 && z->n_unit_atoms >= z->n_structs && z->n_super_atoms >= z->n_unit_atoms &&
         z->n_pairs >= z->n_super_atoms && z->n_unit_atoms <= INT32_MAX && z->n_structs <= INT32_MAX &&
         6 * z->n_pairs + z->n_super_atoms <= (int64_t)INT32_MAX * 256;
}

// the shortest images of supercell atom j seen from home atom u, in unit-cell fractional coordinates; false if more than kMaxMult tie
bool shortest_images(const double L[9], const int n[3], const double* ru, const double* rv, const int l[3], std::vector<double>& d) {
  // fractional difference in unit-cell coordinates: frac(r_v) - frac(r_u) + l
  double inv[9];
  inv3(L, inv);
  double f0[3];   // (r_v - r_u) inv(L): row vector times the inverse of the row-vector lattice
  for (int c = 0; c < 3; ++c) f0[c] = (rv[0] - ru[0]) * inv[c] + (rv[1] - ru[1]) * inv[3 + c] + (rv[2] - ru[2]) * inv[6 + c] + l[c];
  double best = INFINITY;
  double cand[125][4];
  int k = 0;
  for (int t0 = -2; t0 <= 2; ++t0)
    for (int t1 = -2; t1 <= 2; ++t1)
      for (int t2 = -2; t2 <= 2; ++t2) {
        const double f[3] = {f0[0] + t0 * n[0], f0[1] + t1 * n[1], f0[2] + t2 * n[2]};
        double x[3];
        for (int c = 0; c < 3; ++c) x[c] = f[0] * L[c] + f[1] * L[3 + c] + f[2] * L[6 + c];
        const double r = std::sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
        cand[k][0] = f[0]; cand[k][1] = f[1]; cand[k][2] = f[2]; cand[k][3] = r;
        best = std::fmin(best, r);
        ++k;
      }
  d.clear();
  for (int i = 0; i < 125; ++i)
    if (cand[i][3] <= best + 1e-5) d.insert(d.end(), cand[i], cand[i] + 3);
  return (int)d.size() / 3 <= kMaxMult;
}
}  // namespace
}  // namespace m3g

using namespace m3g;

extern "C" int m3g_ph_state_bytes(const m3g_ph_sizes* sizes, size_t* bytes) {
  if (!bytes || !ph_sizes_ok(sizes)) {
    set_error("m3g_ph_state_bytes: bad sizes (need 1 <= n_structs <= n_unit_atoms <= n_super_atoms <= n_pairs)");
    return M3G_ERR_VALUE;
  }
  *bytes = ph_view(*sizes, nullptr).bytes;
  return M3G_OK;
}

extern "C" int m3g_ph_init(const m3g_ph_sizes* sizes, const int64_t* host_unit_offsets, const int32_t* host_supercells,
                           const double* host_lattices, const double* host_positions, const double* host_masses, double delta, void* state,
                           size_t state_bytes, void* stream_) {
  if (!ph_sizes_ok(sizes) || !host_unit_offsets || !host_supercells || !host_lattices || !host_positions || !host_masses || !state) {
    set_error("m3g_ph_init: null argument or bad sizes (need 1 <= n_structs <= n_unit_atoms <= n_super_atoms <= n_pairs)");
    return M3G_ERR_VALUE;
  }
  const m3g_ph_sizes z = *sizes;
  const int64_t S = z.n_structs, U = z.n_unit_atoms;
  if (!offsets_ok("m3g_ph_init", host_unit_offsets, U, S, "unit offsets", "n_unit_atoms")) return M3G_ERR_VALUE;
  if (!finite_positive(delta)) { set_error("m3g_ph_init: delta must be finite and > 0"); return M3G_ERR_VALUE; }
  std::vector<int64_t> row_off(S + 1, 0), pair_off(S + 1, 0);
  std::vector<int32_t> unit_struct(U);
  int64_t n_super = 0;
  for (int64_t s = 0; s < S; ++s) {
    const int32_t* n = host_supercells + 3 * s;
    if (n[0] < 1 || n[1] < 1 || n[2] < 1 || (int64_t)n[0] * n[1] * n[2] > (1 << 20)) {
      set_error("m3g_ph_init: supercell of structure %lld must have dims >= 1 (and at most 2^20 cells)", (long long)s);
      return M3G_ERR_VALUE;
    }
    if (!lattice_ok("m3g_ph_init", host_lattices + 9 * s, s)) return M3G_ERR_VALUE;
    const int64_t nu = host_unit_offsets[s + 1] - host_unit_offsets[s];
    const int64_t ns = nu * n[0] * n[1] * n[2];
    for (int64_t g = host_unit_offsets[s]; g < host_unit_offsets[s + 1]; ++g) {
      unit_struct[g] = (int32_t)s;
      if (!finite_positive(host_masses[g])) { set_error("m3g_ph_init: mass of unit atom %lld must be finite and > 0", (long long)g); return M3G_ERR_VALUE; }
      for (int c = 0; c < 3; ++c)
        if (!std::isfinite(host_positions[3 * g + c])) { set_error("m3g_ph_init: position of unit atom %lld is not finite", (long long)g); return M3G_ERR_VALUE; }
    }
    row_off[s + 1] = row_off[s] + (1 + 6 * nu) * ns;
    pair_off[s + 1] = pair_off[s] + nu * ns;
    n_super += ns;
  }
  if (n_super != z.n_super_atoms || pair_off[S] != z.n_pairs) {
    set_error("m3g_ph_init: sizes do not match the offsets and supercells (n_super_atoms %lld, n_pairs %lld expected)", (long long)n_super,
              (long long)pair_off[S]);
    return M3G_ERR_VALUE;
  }
  // the image table, fp64 on the host
  std::vector<int32_t> img_count(z.n_pairs);
  std::vector<double> img_d((size_t)3 * kMaxMult * z.n_pairs, 0.0), d;
  for (int64_t s = 0; s < S; ++s) {
    const int32_t* n = host_supercells + 3 * s;
    const int64_t o = host_unit_offsets[s], nu = host_unit_offsets[s + 1] - o;
    const int64_t ns = nu * n[0] * n[1] * n[2];
    for (int64_t u = 0; u < nu; ++u)
      for (int64_t j = 0; j < ns; ++j) {
        const int64_t lc = j / nu, v = j % nu;
        const int l[3] = {(int)(lc / ((int64_t)n[1] * n[2])), (int)((lc / n[2]) % n[1]), (int)(lc % n[2])};
        const int nn[3] = {n[0], n[1], n[2]};
        if (!shortest_images(host_lattices + 9 * s, nn, host_positions + 3 * (o + u), host_positions + 3 * (o + v), l, d)) {
          set_error("m3g_ph_init: structure %lld: %zu shortest images tie for pair (%lld, %lld), above the image table capacity %d",
                    (long long)s, d.size() / 3, (long long)u, (long long)j, kMaxMult);
          return M3G_ERR_VALUE;
        }
        const int64_t p = pair_off[s] + u * ns + j;
        img_count[p] = (int32_t)(d.size() / 3);
        std::copy(d.begin(), d.end(), img_d.begin() + 3 * kMaxMult * p);
      }
  }
  const auto [st, total] = ph_view(z, state);
  if (!state_fits("m3g_ph_init", state_bytes, total, true)) return M3G_ERR_SIZE;
  hipStream_t s = (hipStream_t)stream_;
  M3G_HIP_CHECK(hipMemcpyAsync((void*)st.row_off, row_off.data(), 8 * (S + 1), hipMemcpyHostToDevice, s));
  M3G_HIP_CHECK(hipMemcpyAsync((void*)st.unit_off, host_unit_offsets, 8 * (S + 1), hipMemcpyHostToDevice, s));
  M3G_HIP_CHECK(hipMemcpyAsync((void*)st.pair_off, pair_off.data(), 8 * (S + 1), hipMemcpyHostToDevice, s));
  M3G_HIP_CHECK(hipMemcpyAsync((void*)st.dims, host_supercells, 4 * 3 * S, hipMemcpyHostToDevice, s));
  M3G_HIP_CHECK(hipMemcpyAsync((void*)st.lat, host_lattices, 8 * 9 * S, hipMemcpyHostToDevice, s));
  M3G_HIP_CHECK(hipMemcpyAsync((void*)st.unit_pos, host_positions, 8 * 3 * U, hipMemcpyHostToDevice, s));
  M3G_HIP_CHECK(hipMemcpyAsync((void*)st.mass, host_masses, 8 * U, hipMemcpyHostToDevice, s));
  M3G_HIP_CHECK(hipMemcpyAsync((void*)st.unit_struct, unit_struct.data(), 4 * U, hipMemcpyHostToDevice, s));
  M3G_HIP_CHECK(hipMemcpyAsync((void*)st.delta, &delta, 8, hipMemcpyHostToDevice, s));
  M3G_HIP_CHECK(hipMemcpyAsync((void*)st.img_count, img_count.data(), 4 * z.n_pairs, hipMemcpyHostToDevice, s));
  M3G_HIP_CHECK(hipMemcpyAsync((void*)st.img_d, img_d.data(), 8 * img_d.size(), hipMemcpyHostToDevice, s));
  M3G_HIP_CHECK(hipStreamSynchronize(s));   // (the host tables above go out of scope)
  return M3G_OK;
}

extern "C" int m3g_ph_displace(const m3g_ph_sizes* sizes, const void* state, size_t state_bytes, double* pos, void* stream_) {
  if (!ph_sizes_ok(sizes) || !state || !pos) { set_error("m3g_ph_displace: null argument or bad sizes"); return M3G_ERR_VALUE; }
  const auto [st, total] = ph_view(*sizes, state);
  if (!state_fits("m3g_ph_displace", state_bytes, total)) return M3G_ERR_SIZE;
  hipLaunchKernelGGL(k_ph_displace, grid_for(st.rows, 256), dim3(256), 0, (hipStream_t)stream_, st, pos);
  M3G_RETURN_LAUNCH_STATUS();
}

extern "C" int m3g_ph_force_constants(const m3g_ph_sizes* sizes, const void* state, size_t state_bytes, const float* forces, int32_t asr,
                                      double* phi, double* sums, int32_t* nonfinite, void* stream_) {
  if (!ph_sizes_ok(sizes) || !state || !forces || !phi || !sums || !nonfinite || (asr != 0 && asr != 1)) {
    set_error("m3g_ph_force_constants: null argument, bad sizes or asr not 0 / 1");
    return M3G_ERR_VALUE;
  }
  const auto [st, total] = ph_view(*sizes, state);
  if (!state_fits("m3g_ph_force_constants", state_bytes, total)) return M3G_ERR_SIZE;
  hipLaunchKernelGGL(k_ph_force_constants, dim3((unsigned)st.U), dim3(kFcThreads), 0, (hipStream_t)stream_, st, forces, (int)asr, phi, sums,
                     nonfinite);
  M3G_RETURN_LAUNCH_STATUS();
}

namespace {
// the checks and the launch of m3g_ph_dynmat and m3g_ph_dynmat_gradient (three workgroups per one of the plain kernel)
template <bool kGrad>
int dynmat_call(const char* fn, const m3g_ph_sizes* sizes, const void* state, size_t state_bytes, const double* phi, int64_t n_q,
                const double* q, const int32_t* q_struct, int32_t max_unit_atoms, double* out, void* stream_) {
  if (!ph_sizes_ok(sizes) || !state || !phi || n_q < 0 || (n_q > 0 && (!q || !q_struct || !out)) || max_unit_atoms < 1 ||
      max_unit_atoms > sizes->n_unit_atoms) {
    set_error("%s: null argument, bad sizes, n_q < 0 or max_unit_atoms outside [1, n_unit_atoms]", fn);
    return M3G_ERR_VALUE;
  }
  const auto [st, total] = ph_view(*sizes, state);
  if (!state_fits(fn, state_bytes, total)) return M3G_ERR_SIZE;
  if (n_q == 0) return M3G_OK;
  const int64_t pairs = (int64_t)max_unit_atoms * (max_unit_atoms + 1) / 2;
  const int64_t per_q = (pairs + kDynThreads - 1) / kDynThreads;
  const int64_t blocks = n_q * per_q * (kGrad ? 3 : 1);
  if (blocks > (int64_t(1) << 26)) { set_error("%s: too many q-points for one launch", fn); return M3G_ERR_VALUE; }
  hipLaunchKernelGGL(k_ph_dynmat<kGrad>, dim3((unsigned)blocks), dim3(kDynThreads), 0, (hipStream_t)stream_, st, n_q, per_q, q, q_struct,
                     max_unit_atoms, phi, out);
  M3G_RETURN_LAUNCH_STATUS();
}
}  // namespace

extern "C" int m3g_ph_dynmat(const m3g_ph_sizes* sizes, const void* state, size_t state_bytes, const double* phi, int64_t n_q, const double* q,
                             const int32_t* q_struct, int32_t max_unit_atoms, double* dynmat, void* stream_) {
  return dynmat_call<false>("m3g_ph_dynmat", sizes, state, state_bytes, phi, n_q, q, q_struct, max_unit_atoms, dynmat, stream_);
}

extern "C" int m3g_ph_dynmat_gradient(const m3g_ph_sizes* sizes, const void* state, size_t state_bytes, const double* phi, int64_t n_q,
                                      const double* q, const int32_t* q_struct, int32_t max_unit_atoms, double* gradient, void* stream_) {
  return dynmat_call<true>("m3g_ph_dynmat_gradient", sizes, state, state_bytes, phi, n_q, q, q_struct, max_unit_atoms, gradient, stream_);
}

extern "C" int m3g_ph_group_velocities(int64_t n_q, int32_t n, const double* eigenvalues, const double* eigenvectors, const double* gradient,
                                       double degeneracy_tolerance, double cutoff_frequency, const double* direction, double* velocities,
                                       void* stream_) {
  if (n_q < 0 || n_q > INT32_MAX || n < 1 || n > M3G_PH_GV_MAX_N) {
    set_error("m3g_ph_group_velocities: need 0 <= n_q < 2^31 and 1 <= n <= %d (M3G_PH_GV_MAX_N); got n_q %lld, n %d", M3G_PH_GV_MAX_N,
              (long long)n_q, (int)n);
    return M3G_ERR_VALUE;
  }
  if (!direction || (n_q > 0 && (!eigenvalues || !eigenvectors || !gradient || !velocities))) {
    set_error("m3g_ph_group_velocities: null argument");
    return M3G_ERR_VALUE;
  }
  if (!(std::isfinite(degeneracy_tolerance) && degeneracy_tolerance >= 0.0 && std::isfinite(cutoff_frequency) && cutoff_frequency >= 0.0)) {
    set_error("m3g_ph_group_velocities: degeneracy_tolerance and cutoff_frequency must be finite and >= 0");
    return M3G_ERR_VALUE;
  }
  const double norm = std::sqrt(direction[0] * direction[0] + direction[1] * direction[1] + direction[2] * direction[2]);
  if (!(std::fabs(norm - 1.0) <= 1e-12)) {   // (a NaN or an infinity fails the comparison too)
    set_error("m3g_ph_group_velocities: direction must be a finite unit vector");
    return M3G_ERR_VALUE;
  }
  if (n_q == 0) return M3G_OK;
  const size_t lds = gv_lds_bytes(n);
  if (lds > 48 * 1024) M3G_HIP_CHECK(hipFuncSetAttribute((const void*)k_ph_group_velocities, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k_ph_group_velocities, dim3((unsigned)n_q), dim3(kGvThreads), lds, (hipStream_t)stream_, (int)n, eigenvalues, eigenvectors,
                     gradient, degeneracy_tolerance, cutoff_frequency, direction[0], direction[1], direction[2], velocities);
  M3G_RETURN_LAUNCH_STATUS();
}
