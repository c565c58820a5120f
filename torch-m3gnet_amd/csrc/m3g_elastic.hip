// Batched finite-strain elastic constants and Birch-Murnaghan equation of state (pymatgen's DeformedStructureSet + ElasticTensor
// .from_independent_strains / matcalc's ElasticityCalc and EOSCalc over an ASE calculator).  Without it every deformed cell is one host
// round trip to a calculator and the fits run in numpy.  Here the deformed copies of every structure of a batch are one batch of the
// engine, and the stages around that evaluation are one launch each:
//   k_el_deform        a thread per row of the deformed batch: the row's structure by binary search over the row offsets, its copy,
//                      r D_m from the unit cell in the state, written straight into the fp64 `pos` the engine reads; the first
//                      3 (1 + M) S threads also write one row of a deformed lattice each;
//   k_el_fit_elastic   one wave per structure: lanes 0..35 fit the 36 stress-strain lines (sums in copy order), the 64 lanes count the
//                      non-finite stresses, then lane 0 symmetrises, inverts (Gauss-Jordan, partial pivoting), runs cyclic Jacobi and
//                      writes the moduli;
//   k_el_fit_eos       a thread per structure: Householder QR of the cubic in t = (V / V_ref)^(-2/3) - 1, the minimum, closed forms.
// No atomics: every result depends on its structure's own inputs only, so it is bitwise the same alone or in any batch.  No allocation,
// copy or wait in the three compute calls (capture-safe).  The semantics are stated in include/m3gnet_hip.h.
#include <cmath>
#include <vector>

#include "m3g_chunks.h"
#include "m3g_internal.h"

namespace m3g {
namespace {
constexpr int kMaxDeform = M3G_EL_MAX_DEFORM;
constexpr int kJacobiSweeps = 30;

struct ElView {
  int64_t S, U, rows, copies;   // copies = (1 + M) S
  int32_t M;
  const int64_t *row_off, *unit_off;   // [S+1]: deformed rows, atoms
  const double* lat;                   // [S, 9] rows = lattice vectors
  const double* unit_pos;              // [U, 3]
  const double* dmat;                  // [1 + M, 9]: D_0 = I, D_m
  const int32_t* comp;                 // [M]
  const double* mag;                   // [M]
};
Carved<ElView> el_view(const m3g_el_sizes& z, const void* state) {
  Carve c{state};
  const int64_t S = z.n_structs, U = z.n_atoms, M = z.n_deform;
  ElView st{S, U, (1 + M) * U, (1 + M) * S, z.n_deform};
  st.row_off = c.take<int64_t>(S + 1);
  st.unit_off = c.take<int64_t>(S + 1);
  st.lat = c.take<double>(9 * S);
  st.unit_pos = c.take<double>(3 * U);
  st.dmat = c.take<double>(9 * (M + 1));
  st.comp = c.take<int32_t>(M);
  st.mag = c.take<double>(M);
  return {st, c.off};
}

__global__ void __launch_bounds__(256) k_el_deform(ElView st, double* __restrict__ pos, double* __restrict__ lattices) {
#pragma clang fp contract(off)
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r < 3 * st.copies) {   // row a of the cell of copy c of structure s
    const int64_t k = r / 3, a = r % 3;
    const int64_t s = k / (1 + st.M), c = k % (1 + st.M);
    const double* L = st.lat + 9 * s + 3 * a;
    const double* D = st.dmat + 9 * c;
    for (int x = 0; x < 3; ++x) lattices[3 * r + x] = (L[0] * D[x] + L[1] * D[3 + x]) + L[2] * D[6 + x];
  }
  if (r >= st.rows) return;
  int64_t lo = 0, hi = st.S - 1;   // the structure of row r: the last s with row_off[s] <= r
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) / 2;
    if (st.row_off[mid] <= r) lo = mid; else hi = mid - 1;
  }
  const int64_t s = lo;
  const int64_t n = st.unit_off[s + 1] - st.unit_off[s];
  const int64_t local = r - st.row_off[s];
  const int64_t c = local / n, b = local % n;
  const double* p = st.unit_pos + 3 * (st.unit_off[s] + b);
  const double* D = st.dmat + 9 * c;
  for (int x = 0; x < 3; ++x) pos[3 * r + x] = (p[0] * D[x] + p[1] * D[3 + x]) + p[2] * D[6 + x];
}

// eigenvalues of the symmetric 6 x 6 `a` (destroyed) by cyclic Jacobi: sweeps over (p, q), p < q, row-major; ascending into w
__device__ void jacobi6(double* a, double* w) {
  for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
    double off = 0.0, diag = 0.0;
    for (int p = 0; p < 6; ++p) {
      diag += a[7 * p] * a[7 * p];
      for (int q = p + 1; q < 6; ++q) off += a[6 * p + q] * a[6 * p + q];
    }
    if (!(off > 1e-60 * diag)) break;   // (also leaves on NaN)
    for (int p = 0; p < 5; ++p)
      for (int q = p + 1; q < 6; ++q) {
        const double apq = a[6 * p + q];
        if (apq == 0.0) continue;
        const double theta = (a[7 * q] - a[7 * p]) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
        for (int k = 0; k < 6; ++k) {   // columns p, q
          const double akp = a[6 * k + p], akq = a[6 * k + q];
          a[6 * k + p] = c * akp - sn * akq;
          a[6 * k + q] = sn * akp + c * akq;
        }
        for (int k = 0; k < 6; ++k) {   // rows p, q
          const double apk = a[6 * p + k], aqk = a[6 * q + k];
          a[6 * p + k] = c * apk - sn * aqk;
          a[6 * q + k] = sn * apk + c * aqk;
        }
      }
  }
  for (int p = 0; p < 6; ++p) w[p] = a[7 * p];
  for (int i = 1; i < 6; ++i) {   // insertion sort, ascending
    const double v = w[i];
    int j = i - 1;
    while (j >= 0 && w[j] > v) { w[j + 1] = w[j]; --j; }
    w[j + 1] = v;
  }
}

// inverse of the 6 x 6 `a` (destroyed) into `inv` by Gauss-Jordan with partial pivoting; a singular matrix leaves inf / NaN
__device__ void invert6(double* a, double* inv) {
  for (int i = 0; i < 36; ++i) inv[i] = (i / 6 == i % 6) ? 1.0 : 0.0;
  for (int k = 0; k < 6; ++k) {
    int piv = k;
    for (int i = k + 1; i < 6; ++i)
      if (fabs(a[6 * i + k]) > fabs(a[6 * piv + k])) piv = i;
    if (piv != k)
      for (int j = 0; j < 6; ++j) {
        double t = a[6 * k + j]; a[6 * k + j] = a[6 * piv + j]; a[6 * piv + j] = t;
        t = inv[6 * k + j]; inv[6 * k + j] = inv[6 * piv + j]; inv[6 * piv + j] = t;
      }
    const double d = 1.0 / a[7 * k];
    for (int j = 0; j < 6; ++j) { a[6 * k + j] *= d; inv[6 * k + j] *= d; }
    for (int i = 0; i < 6; ++i) {
      if (i == k) continue;
      const double f = a[6 * i + k];
      for (int j = 0; j < 6; ++j) { a[6 * i + j] -= f * a[6 * k + j]; inv[6 * i + j] -= f * inv[6 * k + j]; }
    }
  }
}

__global__ void __launch_bounds__(kWave) k_el_fit_elastic(ElView st, const float* __restrict__ stresses, double* __restrict__ rows,
                                                          int32_t* __restrict__ nonfinite) {
#pragma clang fp contract(off)
  __shared__ double craw[36], resid[36], work[36], sym[36], inv[36], eig[6];
  __shared__ int32_t bad[kWave];
  const int64_t s = blockIdx.x;
  const int t = threadIdx.x;
  const int M = st.M;
  const float* sg = stresses + 6 * (1 + (int64_t)M) * s;   // [1 + M, 6] of this structure; sigma = -stresses
  int32_t nb = 0;
  for (int i = t; i < 6 * (1 + M); i += kWave) nb += std::isfinite(sg[i]) ? 0 : 1;
  bad[t] = nb;
  if (t < 36) {
    const int i = t / 6, j = t % 6;
    const double y0 = -(double)sg[i];
    // the straight line through (0, y0) and the copies of component j in copy order: centred sums
    double sx = 0.0, sy = y0;
    int n = 1;
    for (int m = 0; m < M; ++m)
      if (st.comp[m] == j) { sx += st.mag[m]; sy += -(double)sg[6 * (m + 1) + i]; ++n; }
    const double xb = sx / (double)n, yb = sy / (double)n;
    double sxx = (0.0 - xb) * (0.0 - xb), sxy = (0.0 - xb) * (y0 - yb);
    for (int m = 0; m < M; ++m)
      if (st.comp[m] == j) {
        const double dx = st.mag[m] - xb, dy = -(double)sg[6 * (m + 1) + i] - yb;
        sxx += dx * dx;
        sxy += dx * dy;
      }
    const double slope = sxy / sxx, icpt = yb - slope * xb;
    double worst = fabs(y0 - icpt);
    for (int m = 0; m < M; ++m)
      if (st.comp[m] == j) worst = fmax(worst, fabs(-(double)sg[6 * (m + 1) + i] - (icpt + slope * st.mag[m])));
    craw[t] = slope;
    resid[t] = worst;
  }
  __syncthreads();
  if (t != 0) return;
  double* out = rows + (int64_t)M3G_EL_ROW * s;
  int32_t total = 0;
  for (int i = 0; i < kWave; ++i) total += bad[i];
  nonfinite[s] = total;
  if (total != 0) {
    for (int i = 0; i < M3G_EL_ROW; ++i) out[i] = NAN;
    return;
  }
  double asym = 0.0, fit = 0.0;
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) {
      const double c = 0.5 * (craw[6 * i + j] + craw[6 * j + i]);
      sym[6 * i + j] = c;
      asym = fmax(asym, fabs(craw[6 * i + j] - craw[6 * j + i]));
      fit = fmax(fit, resid[6 * i + j]);
    }
  for (int i = 0; i < 36; ++i) { out[M3G_EL_ROW_CRAW + i] = craw[i]; out[M3G_EL_ROW_C + i] = sym[i]; work[i] = sym[i]; }
  invert6(work, inv);
  for (int i = 0; i < 36; ++i) { out[M3G_EL_ROW_S + i] = inv[i]; work[i] = sym[i]; }
  jacobi6(work, eig);
  for (int i = 0; i < 6; ++i) { out[M3G_EL_ROW_SIGMA0 + i] = -(double)sg[i]; out[M3G_EL_ROW_EIG + i] = eig[i]; }
  const double* c = sym;
  const double* q = inv;
  const double c_d = (c[0] + c[7]) + c[14], c_o = (c[1] + c[8]) + c[2], c_s = (c[21] + c[28]) + c[35];
  const double s_d = (q[0] + q[7]) + q[14], s_o = (q[1] + q[8]) + q[2], s_s = (q[21] + q[28]) + q[35];
  const double kv = (c_d + 2.0 * c_o) / 9.0, gv = ((c_d - c_o) + 3.0 * c_s) / 15.0;
  const double kr = 1.0 / (s_d + 2.0 * s_o), gr = 15.0 / ((4.0 * s_d - 4.0 * s_o) + 3.0 * s_s);
  const double kh = 0.5 * (kv + kr), gh = 0.5 * (gv + gr);
  out[M3G_EL_ROW_ASYMMETRY] = asym;
  out[M3G_EL_ROW_FIT_RESIDUAL] = fit;
  out[M3G_EL_ROW_KV] = kv; out[M3G_EL_ROW_KR] = kr; out[M3G_EL_ROW_KH] = kh;
  out[M3G_EL_ROW_GV] = gv; out[M3G_EL_ROW_GR] = gr; out[M3G_EL_ROW_GH] = gh;
  out[M3G_EL_ROW_YOUNG] = 9.0 * kh * gh / (3.0 * kh + gh);
  out[M3G_EL_ROW_POISSON] = (3.0 * kh - 2.0 * gh) / (2.0 * (3.0 * kh + gh));
  out[M3G_EL_ROW_ANISOTROPY] = (5.0 * gv / gr + kv / kr) - 6.0;
  out[M3G_EL_ROW_STABLE] = eig[0] > 0.0 ? 1.0 : 0.0;
}

__global__ void __launch_bounds__(kWave) k_el_fit_eos(ElView st, const float* __restrict__ energies, double* __restrict__ rows,
                                                      int32_t* __restrict__ error) {
#pragma clang fp contract(off)
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= st.S) return;
  const int M = st.M, n = 1 + M;
  const float* e = energies + (int64_t)n * s;
  double* out = rows + (int64_t)M3G_EL_EOS_ROW * s;
  const double* L = st.lat + 9 * s;
  const double vref = fabs(L[0] * (L[4] * L[8] - L[5] * L[7]) - L[1] * (L[3] * L[8] - L[5] * L[6]) + L[2] * (L[3] * L[7] - L[4] * L[6]));
  int32_t err = 0;
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(e[i])) err |= M3G_EL_EOS_NONFINITE;
  if (err) {
    for (int i = 0; i < M3G_EL_EOS_ROW; ++i) out[i] = NAN;
    error[s] = err;
    return;
  }
  // t of every point, its scale, and the design matrix [1, u, u^2, u^3] with the right-hand side E - E(copy 0)
  // (390 doubles, 3.1 KB, of private memory per thread, on purpose: one thread per structure, launch-bound; LDS or a workspace in
  // the state would buy nothing here)
  double a[(kMaxDeform + 1) * 4], b[kMaxDeform + 1], tt[kMaxDeform + 1];
  double ts = 0.0, tmin = 0.0, tmax = 0.0;
  tt[0] = 0.0;
  for (int m = 0; m < M; ++m) {
    const double f = 1.0 + st.mag[m];
    tt[m + 1] = 1.0 / (f * f) - 1.0;
    ts = fmax(ts, fabs(tt[m + 1]));
    tmin = fmin(tmin, tt[m + 1]);
    tmax = fmax(tmax, tt[m + 1]);
  }
  const double eref = (double)e[0];
  for (int i = 0; i < n; ++i) {
    const double u = tt[i] / ts;
    a[4 * i] = 1.0; a[4 * i + 1] = u; a[4 * i + 2] = u * u; a[4 * i + 3] = u * u * u;
    b[i] = (double)e[i] - eref;
  }
  for (int k = 0; k < 4; ++k) {   // Householder: H_k = I - 2 v v^T / v^T v zeroes column k below the diagonal
    double nrm = 0.0;
    for (int i = k; i < n; ++i) nrm += a[4 * i + k] * a[4 * i + k];
    nrm = sqrt(nrm);
    const double alpha = a[4 * k + k] > 0.0 ? -nrm : nrm;
    a[4 * k + k] -= alpha;   // column k from row k on now holds v
    double vv = 0.0;
    for (int i = k; i < n; ++i) vv += a[4 * i + k] * a[4 * i + k];
    for (int j = k + 1; j < 4; ++j) {
      double d = 0.0;
      for (int i = k; i < n; ++i) d += a[4 * i + k] * a[4 * i + j];
      const double f = 2.0 * d / vv;
      for (int i = k; i < n; ++i) a[4 * i + j] -= f * a[4 * i + k];
    }
    double d = 0.0;
    for (int i = k; i < n; ++i) d += a[4 * i + k] * b[i];
    const double f = 2.0 * d / vv;
    for (int i = k; i < n; ++i) b[i] -= f * a[4 * i + k];
    a[4 * k + k] = alpha;   // R's diagonal (v is not needed again)
  }
  double c[4];
  for (int k = 3; k >= 0; --k) {
    double v = b[k];
    for (int j = k + 1; j < 4; ++j) v -= a[4 * k + j] * c[j];
    c[k] = v / a[4 * k + k];
  }
  double ss = 0.0;
  for (int i = 0; i < n; ++i) {
    const double u = tt[i] / ts;
    const double d = (((c[3] * u + c[2]) * u + c[1]) * u + c[0]) - ((double)e[i] - eref);
    ss += d * d;
  }
  out[4] = sqrt(ss / (double)n);
  out[5] = vref;
  out[7] = (double)n;
  // dE/du = c1 + 2 c2 u + 3 c3 u^2 = 0 at a minimum (E'' = 2 c2 + 6 c3 u > 0)
  double u0 = NAN;
  const double disc = c[2] * c[2] - 3.0 * c[3] * c[1];
  if (fabs(c[3]) <= 1e-14 * fabs(c[2])) {
    if (c[2] > 0.0) u0 = -c[1] / (2.0 * c[2]);
  } else if (disc > 0.0) {
    const double q = -(c[2] + (c[2] >= 0.0 ? sqrt(disc) : -sqrt(disc)));
    const double r1 = q / (3.0 * c[3]), r2 = c[1] / q;
    const bool m1 = 2.0 * c[2] + 6.0 * c[3] * r1 > 0.0, m2 = 2.0 * c[2] + 6.0 * c[3] * r2 > 0.0;
    if (m1 && m2) u0 = fabs(r1) <= fabs(r2) ? r1 : r2;   // (a double root only: the nearer to t = 0)
    else if (m1) u0 = r1;
    else if (m2) u0 = r2;
  }
  const double t0 = u0 * ts;
  if (!(t0 >= tmin && t0 <= tmax)) {
    out[0] = out[1] = out[2] = out[3] = out[6] = NAN;
    error[s] = M3G_EL_EOS_NO_MINIMUM;
    return;
  }
  const double g = 1.0 + t0;
  const double v0 = vref / (g * sqrt(g));
  const double e2 = (2.0 * c[2] + 6.0 * c[3] * u0) / (ts * ts), e3 = 6.0 * c[3] / (ts * ts * ts);
  const double a2 = 0.5 * e2 * g * g, a3 = e3 * g * g * g / 6.0;
  out[0] = v0;
  out[1] = eref + (((c[3] * u0 + c[2]) * u0 + c[1]) * u0 + c[0]);
  out[2] = 8.0 * a2 / (9.0 * v0);
  out[3] = 4.0 + 2.0 * a3 / a2;
  out[6] = t0;
  error[s] = 0;
}

bool el_sizes_ok(const m3g_el_sizes* z) {
  return z && z->n_structs >= 1 && z->n_atoms >= z->n_structs && z->n_deform >= 1 && z->n_deform <= kMaxDeform &&
         (z->mode == M3G_EL_MODE_ELASTIC || z->mode == M3G_EL_MODE_EOS) && z->n_structs <= INT32_MAX / (3 * (kMaxDeform + 1)) &&
         z->n_atoms <= ((int64_t)INT32_MAX * 256) / (kMaxDeform + 1);
}
constexpr const char* kSizesMsg = "bad sizes (need 1 <= n_structs <= n_atoms, 1 <= n_deform <= M3G_EL_MAX_DEFORM, mode 0 / 1)";

// the checks every compute call shares; M3G_OK, or the status to return
int el_call_ok(const char* name, const m3g_el_sizes* sizes, const void* state, size_t state_bytes, bool pointers, int mode) {
  if (!el_sizes_ok(sizes) || !state || !pointers) { set_error("%s: null argument or %s", name, kSizesMsg); return M3G_ERR_VALUE; }
  if (mode >= 0 && sizes->mode != mode) { set_error("%s: the state was made for the other mode (M3G_EL_MODE_*)", name); return M3G_ERR_VALUE; }
  return state_fits(name, state_bytes, el_view(*sizes, nullptr).bytes) ? M3G_OK : M3G_ERR_SIZE;
}
}  // namespace
}  // namespace m3g

using namespace m3g;

extern "C" int m3g_el_state_bytes(const m3g_el_sizes* sizes, size_t* bytes) {
  if (!bytes || !el_sizes_ok(sizes)) { set_error("m3g_el_state_bytes: %s", kSizesMsg); return M3G_ERR_VALUE; }
  *bytes = el_view(*sizes, nullptr).bytes;
  return M3G_OK;
}

extern "C" int m3g_el_init(const m3g_el_sizes* sizes, const int64_t* host_offsets, const double* host_lattices, const double* host_positions,
                           const int32_t* host_components, const double* host_magnitudes, void* state, size_t state_bytes, void* stream_) {
  if (!el_sizes_ok(sizes) || !host_offsets || !host_lattices || !host_positions || !host_components || !host_magnitudes || !state) {
    set_error("m3g_el_init: null argument or %s", kSizesMsg);
    return M3G_ERR_VALUE;
  }
  const m3g_el_sizes z = *sizes;
  const int64_t S = z.n_structs, U = z.n_atoms;
  const int M = z.n_deform;
  if (!offsets_ok("m3g_el_init", host_offsets, U, S)) return M3G_ERR_VALUE;
  for (int64_t s = 0; s < S; ++s)
    if (!lattice_ok("m3g_el_init", host_lattices + 9 * s, s)) return M3G_ERR_VALUE;
  for (int64_t i = 0; i < 3 * U; ++i)
    if (!std::isfinite(host_positions[i])) { set_error("m3g_el_init: position of atom %lld is not finite", (long long)(i / 3)); return M3G_ERR_VALUE; }
  for (int m = 0; m < M; ++m) {
    const double d = host_magnitudes[m];
    if (!(std::isfinite(d) && d != 0.0 && std::fabs(d) < M3G_EL_MAX_STRAIN)) {
      set_error("m3g_el_init: magnitude %d must be finite, non-zero and below %g in size", m, (double)M3G_EL_MAX_STRAIN);
      return M3G_ERR_VALUE;
    }
    const int32_t c = host_components[m];
    if (z.mode == M3G_EL_MODE_ELASTIC ? (c < 0 || c > 5) : c != M3G_EL_VOLUMETRIC) {
      set_error("m3g_el_init: component %d is %d (elastic mode: 0..5, EOS mode: M3G_EL_VOLUMETRIC)", m, (int)c);
      return M3G_ERR_VALUE;
    }
  }
  auto distinct = [&](int comp) {   // distinct magnitudes of one component
    int n = 0;
    for (int m = 0; m < M; ++m) {
      if (host_components[m] != comp) continue;
      bool seen = false;
      for (int k = 0; k < m; ++k) seen = seen || (host_components[k] == comp && host_magnitudes[k] == host_magnitudes[m]);
      n += seen ? 0 : 1;
    }
    return n;
  };
  if (z.mode == M3G_EL_MODE_ELASTIC) {
    for (int j = 0; j < 6; ++j)
      if (distinct(j) < 2) { set_error("m3g_el_init: component %d needs at least two distinct magnitudes", j); return M3G_ERR_VALUE; }
  } else if (1 + distinct(M3G_EL_VOLUMETRIC) < 5) {
    set_error("m3g_el_init: an equation of state needs at least 5 distinct volumes (the undeformed cell counted)");
    return M3G_ERR_VALUE;
  }
  std::vector<int64_t> row_off(S + 1);
  for (int64_t s = 0; s <= S; ++s) row_off[s] = (1 + (int64_t)M) * host_offsets[s];
  std::vector<double> dmat(9 * (size_t)(M + 1), 0.0);
  dmat[0] = dmat[4] = dmat[8] = 1.0;
  static const int kVoigt[6][2] = {{0, 0}, {1, 1}, {2, 2}, {1, 2}, {2, 0}, {0, 1}};
  for (int m = 0; m < M; ++m) {
    double* D = dmat.data() + 9 * (m + 1);
    const double d = host_magnitudes[m];
    const int32_t c = host_components[m];
    D[0] = D[4] = D[8] = (c == M3G_EL_VOLUMETRIC) ? 1.0 + d : 1.0;
    if (c < 3) D[4 * c] = 1.0 + d;
    else if (c < 6) D[3 * kVoigt[c][0] + kVoigt[c][1]] = D[3 * kVoigt[c][1] + kVoigt[c][0]] = 0.5 * d;
  }
  const auto [st, total] = el_view(z, state);
  if (!state_fits("m3g_el_init", state_bytes, total, true)) return M3G_ERR_SIZE;
  hipStream_t s = (hipStream_t)stream_;
  M3G_HIP_CHECK(hipMemcpyAsync((void*)st.row_off, row_off.data(), 8 * (S + 1), hipMemcpyHostToDevice, s));
  M3G_HIP_CHECK(hipMemcpyAsync((void*)st.unit_off, host_offsets, 8 * (S + 1), hipMemcpyHostToDevice, s));
  M3G_HIP_CHECK(hipMemcpyAsync((void*)st.lat, host_lattices, 8 * 9 * S, hipMemcpyHostToDevice, s));
  M3G_HIP_CHECK(hipMemcpyAsync((void*)st.unit_pos, host_positions, 8 * 3 * U, hipMemcpyHostToDevice, s));
  M3G_HIP_CHECK(hipMemcpyAsync((void*)st.dmat, dmat.data(), 8 * dmat.size(), hipMemcpyHostToDevice, s));
  M3G_HIP_CHECK(hipMemcpyAsync((void*)st.comp, host_components, 4 * (size_t)M, hipMemcpyHostToDevice, s));
  M3G_HIP_CHECK(hipMemcpyAsync((void*)st.mag, host_magnitudes, 8 * (size_t)M, hipMemcpyHostToDevice, s));
  M3G_HIP_CHECK(hipStreamSynchronize(s));   // (the host tables above go out of scope)
  return M3G_OK;
}

extern "C" int m3g_el_deform(const m3g_el_sizes* sizes, const void* state, size_t state_bytes, double* pos, double* lattices, void* stream_) {
  if (const int rc = el_call_ok("m3g_el_deform", sizes, state, state_bytes, pos && lattices, -1)) return rc;
  const ElView st = el_view(*sizes, state).view;
  const int64_t threads = st.rows > 3 * st.copies ? st.rows : 3 * st.copies;
  hipLaunchKernelGGL(k_el_deform, grid_for(threads, 256), dim3(256), 0, (hipStream_t)stream_, st, pos, lattices);
  M3G_RETURN_LAUNCH_STATUS();
}

extern "C" int m3g_el_fit_elastic(const m3g_el_sizes* sizes, const void* state, size_t state_bytes, const float* stresses, double* rows,
                                  int32_t* nonfinite, void* stream_) {
  if (const int rc = el_call_ok("m3g_el_fit_elastic", sizes, state, state_bytes, stresses && rows && nonfinite, M3G_EL_MODE_ELASTIC)) return rc;
  const ElView st = el_view(*sizes, state).view;
  hipLaunchKernelGGL(k_el_fit_elastic, dim3((unsigned)st.S), dim3(kWave), 0, (hipStream_t)stream_, st, stresses, rows, nonfinite);
  M3G_RETURN_LAUNCH_STATUS();
}

extern "C" int m3g_el_fit_eos(const m3g_el_sizes* sizes, const void* state, size_t state_bytes, const float* energies, double* rows,
                              int32_t* error, void* stream_) {
  if (const int rc = el_call_ok("m3g_el_fit_eos", sizes, state, state_bytes, energies && rows && error, M3G_EL_MODE_EOS)) return rc;
  const ElView st = el_view(*sizes, state).view;
  hipLaunchKernelGGL(k_el_fit_eos, grid_for(st.S, kWave), dim3(kWave), 0, (hipStream_t)stream_, st, energies, rows, error);
  M3G_RETURN_LAUNCH_STATUS();
}
