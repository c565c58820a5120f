// Batched collective-variable biasing: metadynamics (Laio, Parrinello, PNAS 99, 12562 (2002); well-tempered: Barducci, Bussi,
// Parrinello, PRL 100, 020603 (2008); multiple walkers: Raiteri et al., J. Phys. Chem. B 110, 3533 (2006)) and umbrella restraints
// (Torrie, Valleau 1977), as PLUMED's METAD, RESTRAINT, LOWER_WALLS and UPPER_WALLS.  A bias layer, not an MD family: one
// m3g_meta_bias takes the integrator's unwrapped positions and the engine's forces and writes the biased forces, which go to
// m3g_dyn_step (or m3g_nhc_step) unchanged -- as m3g_remd_* and m3g_rnemd_* sit over an m3g_dyn_* batch.  The S structures are cut
// into G walker groups; the walkers of a group share one hill list.  Up to two collective variables (CVs) per call: DISTANCE and
// PROJECTION of weighted centres of two atom sets, COORDINATION of two atom sets under the minimum image of a fixed cell.
// One call is three launches for the whole batch:
//   k_meta_partials  one workgroup per chunk of the chunk table (m3g_chunks.h): the chunk sums of w, w x over A and B of every
//                    centre CV in a fixed tree; for COORDINATION every row walks the rows of its own structure, in row order,
//                    through 256-row LDS tiles of fractional positions, writes its own gradient row into the state and adds its
//                    own sum of switching functions to the chunk partial (every pair is computed from both ends: no atomics);
//   k_meta_finalize  one wave per structure: the chunk partials in chunk order, the CVs, the group's hills lane-strided in list
//                    order and a fixed butterfly, restraint and walls, the deposit, flags, the obs row, the coefficients of the apply;
//   k_meta_apply     one workgroup per chunk: d s_k / d x_i of every row and forces_out = forces - sum_k (dV/ds_k) d s_k / d x_i.
// All arithmetic is fp64 and no product is contracted with a sum (every kernel switches contraction off, lexically); the one f32
// operation is the final rounding of forces_out.  A deposit reads the slots below c R and walker r writes slot c R + r (c: the
// deposit count the walker carries, R: the walkers of its group), so no slot is read and written in one launch.  Every result of a
// group depends on its own rows and hills only: bitwise the same alone or in any batch.  No allocation, copy or wait in
// m3g_meta_bias (capture-safe: counts and hills live on the device).
#include <cmath>
#include <cstring>
#include <vector>

#include "m3g_chunks.h"

namespace m3g {
namespace {
constexpr int kMaxCv = M3G_META_MAX_CV;
constexpr int kCvCols = 8;                          // per CV: sum w, sum w x [3] over A, the same over B; COORDINATION: its sum, 7 unused
constexpr int kMetaPart = kMaxCv * kCvCols + 1;     // ... and the rows of the chunk that take part and are not finite
constexpr int kCvCoef = 7;                          // per CV: dV/ds, the unit vector [3], the weights of A and of B, unused
constexpr int kMetaCoef = 1 + kMaxCv * kCvCoef;     // per structure: biased?, then the CVs
constexpr int kMaxPower = 6;
static_assert(kMaxCv == 2 && M3G_META_OBS == 8, "the obs row holds two CVs");

struct MetaView {
  int64_t N, S, max_hills;
  int32_t n_cv;
  ChunkView ch;
  int64_t* group_offsets;          // [G+1]: the structures of every group
  int32_t* struct_group;           // [S]
  uint8_t* membership;             // [n_cv, N]: bit 0 = A, bit 1 = B
  double *weights, *lat, *inv;     // [N], [S,9], [S,9] (fractional = cartesian . inv)
  double *origin, *centre, *kappa, *walls;   // [S,n_cv,3], [S,n_cv], [S,n_cv], [S,n_cv,4] = lower, its kappa, upper, its kappa
  double *sigma, *height, *inv_kdt;          // [G,n_cv], [G], [G]
  int64_t* deposits;               // [S]: the deposits a walker has made (the same for every walker of a group)
  int32_t* flags;                  // [S]
  double *partial, *grad, *coef;   // [chunks, kMetaPart], [n_cv, N, 3], [S, kMetaCoef]
  double *hill_centres, *hill_heights;   // [G, max_hills, n_cv], [G, max_hills]
};
Carved<MetaView> meta_view(int64_t N, int64_t S, int64_t G, int32_t n_cv, int64_t max_hills, void* state) {
  Carve c{state};
  MetaView st{N, S, max_hills, n_cv};
  st.ch = chunk_view(N, S, c);
  st.group_offsets = c.take<int64_t>(G + 1);
  st.struct_group = c.take<int32_t>(S);
  st.membership = c.take<uint8_t>(n_cv * N);
  st.weights = c.take<double>(N);
  st.lat = c.take<double>(9 * S);
  st.inv = c.take<double>(9 * S);
  st.origin = c.take<double>(3 * n_cv * S);
  st.centre = c.take<double>(n_cv * S);
  st.kappa = c.take<double>(n_cv * S);
  st.walls = c.take<double>(4 * n_cv * S);
  st.sigma = c.take<double>(n_cv * G);
  st.height = c.take<double>(G);
  st.inv_kdt = c.take<double>(G);
  st.deposits = c.take<int64_t>(S);
  st.flags = c.take<int32_t>(S);
  st.partial = c.take<double>(kMetaPart * chunk_bound(N, S));
  st.grad = c.take<double>(3 * n_cv * N);
  st.coef = c.take<double>(kMetaCoef * S);
  st.hill_centres = c.take<double>(G * max_hills * n_cv);
  st.hill_heights = c.take<double>(G * max_hills);
  return {st, c.off};
}

// x^q, q = 0 .. kMaxPower - 1, by repeated multiplication
__device__ inline double meta_power(double x, int q) {
  double y = 1.0;
  for (int k = 0; k < q; ++k) y = k == 0 ? x : y * x;
  return y;
}

// One workgroup per chunk, thread t on row t of the chunk.
__global__ void __launch_bounds__(kChunkRows) k_meta_partials(MetaView st, m3g_meta_params p, const double* __restrict__ pos) {
#pragma clang fp contract(off)   // (every weighted term, the minimum image and the switching function round as they are written)
  __shared__ double sh[kMetaPart][kChunkRows];
  __shared__ double sh_f[3][kChunkRows];          // the fractional positions of a tile of partner rows
  __shared__ uint8_t sh_m[kMaxCv][kChunkRows];    // their membership, 0 beyond the structure
  const int c = blockIdx.x, t = threadIdx.x;
  if (c >= st.ch.n_chunks()) return;
  const int s = st.ch.structure(c);
  const int64_t i = st.ch.row(c, t);
  const bool here = st.ch.holds(s, i);
  const int n_cv = st.n_cv;
  double val[kMetaPart];
  for (int j = 0; j < kMetaPart; ++j) val[j] = 0.0;
  double x[3] = {0.0, 0.0, 0.0};
  int m[kMaxCv] = {0, 0};
  bool coordination = false;
#pragma unroll
  for (int k = 0; k < kMaxCv; ++k)
    if (k < n_cv) coordination = coordination || p.kind[k] == M3G_CV_COORDINATION;
  if (here) {
    for (int a = 0; a < 3; ++a) x[a] = pos[3 * i + a];
    const double w = st.weights[i];
    int any = 0;
#pragma unroll
    for (int k = 0; k < kMaxCv; ++k) {
      if (k >= n_cv) break;
      m[k] = st.membership[(int64_t)k * st.N + i];
      any |= m[k];
      if (p.kind[k] == M3G_CV_COORDINATION) continue;
      const double wa = (m[k] & 1) ? w : 0.0, wb = (m[k] & 2) ? w : 0.0;
      val[kCvCols * k] = wa;
      val[kCvCols * k + 4] = wb;
      for (int a = 0; a < 3; ++a) {
        val[kCvCols * k + 1 + a] = wa * x[a];
        val[kCvCols * k + 5 + a] = wb * x[a];
      }
    }
    if (any && !(std::isfinite(x[0]) && std::isfinite(x[1]) && std::isfinite(x[2]))) val[kMetaPart - 1] = 1.0;
  }
  if (coordination) {   // (the same in every thread: the barriers below are met by all)
    const double* inv = st.inv + 9 * (int64_t)s;
    const double* l = st.lat + 9 * (int64_t)s;
    const int64_t lo = st.ch.offsets[s], hi = st.ch.offsets[s + 1];
    double fi[3];
    for (int a = 0; a < 3; ++a) fi[a] = (x[0] * inv[a] + x[1] * inv[3 + a]) + x[2] * inv[6 + a];
    double r0sq[kMaxCv], sig_c[kMaxCv], one_m[kMaxCv], k2[kMaxCv], sum[kMaxCv] = {0.0, 0.0}, g[kMaxCv][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
#pragma unroll
    for (int k = 0; k < kMaxCv; ++k) {
      if (k >= n_cv) break;
      r0sq[k] = p.r0[k] * p.r0[k];
      const double tc = (p.r_cut[k] * p.r_cut[k]) / r0sq[k];
      sig_c[k] = 1.0 / (1.0 + meta_power(tc, p.power[k] - 1) * tc);
      one_m[k] = 1.0 - sig_c[k];
      k2[k] = (2.0 / r0sq[k]) / one_m[k];
    }
    for (int64_t t0 = lo; t0 < hi; t0 += kChunkRows) {   // the structure's own chunks, in order
      const int64_t j = t0 + t;
      __syncthreads();   // (the tile before has been read)
      if (j < hi) {
        const double y[3] = {pos[3 * j], pos[3 * j + 1], pos[3 * j + 2]};
        for (int a = 0; a < 3; ++a) sh_f[a][t] = (y[0] * inv[a] + y[1] * inv[3 + a]) + y[2] * inv[6 + a];
      }
      for (int k = 0; k < kMaxCv; ++k) sh_m[k][t] = (k < n_cv && j < hi) ? st.membership[(int64_t)k * st.N + j] : (uint8_t)0;
      __syncthreads();
      const int rows = (int)min((int64_t)kChunkRows, hi - t0);
      if (!here) continue;
      for (int u = 0; u < rows; ++u) {
        if (t0 + u == i) continue;
        double d[3];
        for (int a = 0; a < 3; ++a) {
          d[a] = fi[a] - sh_f[a][u];
          d[a] -= rint(d[a]);   // the minimum image of every pair closer than half the smallest perpendicular width
        }
        const double e[3] = {(d[0] * l[0] + d[1] * l[3]) + d[2] * l[6], (d[0] * l[1] + d[1] * l[4]) + d[2] * l[7],
                             (d[0] * l[2] + d[1] * l[5]) + d[2] * l[8]};
        const double r2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
        const double r = sqrt(r2);
#pragma unroll
        for (int k = 0; k < kMaxCv; ++k) {
          if (k >= n_cv) break;
          if (p.kind[k] != M3G_CV_COORDINATION) continue;
          const int mj = sh_m[k][u];
          const bool ab = (m[k] & 1) && (mj & 2), ba = (m[k] & 2) && (mj & 1);
          if (!(ab || ba) || !(r < p.r_cut[k])) continue;   // (a pair at r_cut exactly, and a non-finite distance, contribute nothing)
          const double tt = r2 / r0sq[k];
          const double tpm = meta_power(tt, p.power[k] - 1);
          const double sig = 1.0 / (1.0 + tpm * tt);
          if (ab) sum[k] += (sig - sig_c[k]) / one_m[k];
          const double dc = -(((sig * sig) * ((double)p.power[k] * tpm)) * k2[k]);   // s'(r) / r
          const double mult = (ab && ba) ? 2.0 : 1.0;
          for (int a = 0; a < 3; ++a) g[k][a] += (dc * e[a]) * mult;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < kMaxCv; ++k) {
      if (k >= n_cv || !here) break;
      if (p.kind[k] != M3G_CV_COORDINATION) continue;
      val[kCvCols * k] = sum[k];
      if (m[k])
        for (int a = 0; a < 3; ++a) st.grad[3 * ((int64_t)k * st.N + i) + a] = g[k][a];
    }
  }
  chunk_tree_reduce<kMetaPart>(sh, val, t);
  if (t < kMetaPart) st.partial[kMetaPart * (int64_t)c + t] = sh[t][0];
}

// One wave per structure, kFinalizeWaves structures per workgroup (no barrier: the waves share nothing).  Every lane carries the
// same scalars; lane 0 stores.
__global__ void __launch_bounds__(kFinalizeWaves * kWave) k_meta_finalize(MetaView st, m3g_meta_params p, int deposit, double* __restrict__ obs) {
#pragma clang fp contract(off)   // (the centres, the hill exponents and every energy term round as they are written)
  const int64_t s = (int64_t)blockIdx.x * kFinalizeWaves + threadIdx.x / kWave;
  const int lane = threadIdx.x % kWave;
  if (s >= st.S) return;   // (whole waves: s is uniform across a wave)
  double acc[kMetaPart];
  wave_chunk_sum<kMetaPart>(st.ch, s, st.partial, lane, acc);
  const int n_cv = st.n_cv;
  const int64_t g = st.struct_group[s];
  const int64_t g0 = st.group_offsets[g], R = st.group_offsets[g + 1] - g0, r = s - g0, c = st.deposits[s];
  double sv[kMaxCv] = {0.0, 0.0}, u[kMaxCv][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}}, wa[kMaxCv] = {0.0, 0.0}, wb[kMaxCv] = {0.0, 0.0};
  bool finite = acc[kMetaPart - 1] == 0.0;
#pragma unroll
  for (int k = 0; k < kMaxCv; ++k) {
    if (k >= n_cv) break;
    const double* q = acc + kCvCols * k;
    if (p.kind[k] == M3G_CV_COORDINATION) {
      sv[k] = q[0];
    } else {
      wa[k] = q[0];
      wb[k] = q[4];
      double d[3];
      for (int a = 0; a < 3; ++a) {
        const double cb = wb[k] > 0.0 ? q[5 + a] / wb[k] : 0.0;   // (an empty B: the origin)
        d[a] = q[1 + a] / wa[k] - cb;
      }
      if (p.kind[k] == M3G_CV_DISTANCE) {
        const double len = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
        sv[k] = len;
        for (int a = 0; a < 3; ++a) u[k][a] = len > 0.0 ? d[a] / len : 0.0;   // (coincident centres: no direction, no force)
      } else {
        const double* o = st.origin + 3 * (s * n_cv + k);
        for (int a = 0; a < 3; ++a) {
          d[a] -= o[a];
          u[k][a] = p.direction[k][a];
        }
        sv[k] = (d[0] * u[k][0] + d[1] * u[k][1]) + d[2] * u[k][2];
      }
    }
    finite = finite && std::isfinite(sv[k]);
  }
  const int64_t n_hills = c * R;
  double inv_s2[kMaxCv] = {0.0, 0.0}, vh = 0.0, dh[kMaxCv] = {0.0, 0.0};
#pragma unroll
  for (int k = 0; k < kMaxCv; ++k) {
    if (k >= n_cv) break;
    const double sg = st.sigma[g * n_cv + k];
    inv_s2[k] = 1.0 / (sg * sg);
  }
  if (finite) {   // (uniform across the wave)
    const double* hc = st.hill_centres + g * st.max_hills * n_cv;
    const double* hh = st.hill_heights + g * st.max_hills;
    for (int64_t h = lane; h < n_hills; h += kWave) {
      double d[kMaxCv] = {0.0, 0.0}, q = 0.0;
#pragma unroll
      for (int k = 0; k < kMaxCv; ++k) {
        if (k >= n_cv) break;
        d[k] = sv[k] - hc[h * n_cv + k];
        q += (d[k] * d[k]) * inv_s2[k];
      }
      const double term = hh[h] * exp(-(0.5 * q));
      vh += term;
#pragma unroll
      for (int k = 0; k < kMaxCv; ++k)
        if (k < n_cv) dh[k] += term * (d[k] * inv_s2[k]);
    }
  }
#pragma unroll
  for (int w = kWave / 2; w > 0; w >>= 1) {   // a + b on both partners: every lane ends with the same bits
    vh += __shfl_xor(vh, w, kWave);
    for (int k = 0; k < kMaxCv; ++k) dh[k] += __shfl_xor(dh[k], w, kWave);
  }
  double vr = 0.0, dv[kMaxCv] = {0.0, 0.0};
#pragma unroll
  for (int k = 0; k < kMaxCv; ++k) {
    if (k >= n_cv) break;
    const int64_t at = s * n_cv + k;
    const double kap = st.kappa[at], ds = sv[k] - st.centre[at];
    const double* wall = st.walls + 4 * at;
    dv[k] = -dh[k];
    vr += (0.5 * kap) * (ds * ds);
    dv[k] += kap * ds;
    if (wall[1] > 0.0 && sv[k] < wall[0]) {
      const double dl = sv[k] - wall[0];
      vr += (0.5 * wall[1]) * (dl * dl);
      dv[k] += wall[1] * dl;
    }
    if (wall[3] > 0.0 && sv[k] > wall[2]) {
      const double du = sv[k] - wall[2];
      vr += (0.5 * wall[3]) * (du * du);
      dv[k] += wall[3] * du;
    }
  }
  int fl = st.flags[s];
  if (!finite) fl |= M3G_META_ERROR;
  double deposited = 0.0;
  if (deposit) {
    if ((c + 1) * R > st.max_hills) {
      fl |= M3G_META_FULL;   // sticky; nothing is deposited and the count stays
    } else {
      if (finite) deposited = st.height[g] * exp(-(vh * st.inv_kdt[g]));
      if (lane == 0) {
        const int64_t slot = g * st.max_hills + (c * R + r);
#pragma unroll
        for (int k = 0; k < kMaxCv; ++k)
          if (k < n_cv) st.hill_centres[slot * n_cv + k] = finite ? sv[k] : 0.0;
        st.hill_heights[slot] = deposited;
        st.deposits[s] = c + 1;
      }
    }
  }
  if (lane != 0) return;
  st.flags[s] = fl;
  double* coef = st.coef + kMetaCoef * s;
  coef[0] = finite ? 1.0 : 0.0;
  for (int k = 0; k < kMaxCv; ++k) {
    double* ck = coef + 1 + kCvCoef * k;
    ck[0] = dv[k];
    for (int a = 0; a < 3; ++a) ck[1 + a] = u[k][a];
    ck[4] = wa[k];
    ck[5] = wb[k];
    ck[6] = 0.0;
  }
  if (obs) {
    double* o = obs + M3G_META_OBS * s;
    o[0] = sv[0];
    o[1] = sv[1];
    o[2] = finite ? vh + vr : 0.0;
    o[3] = finite ? vh : 0.0;
    o[4] = finite ? vr : 0.0;
    o[5] = finite ? dv[0] : 0.0;
    o[6] = finite ? dv[1] : 0.0;
    o[7] = deposited;
  }
}

// One workgroup per chunk, thread t on row t.  forces_out may be forces: every thread reads its own row before it writes it.
__global__ void __launch_bounds__(kChunkRows) k_meta_apply(MetaView st, m3g_meta_params p, const float* forces, float* forces_out) {
#pragma clang fp contract(off)   // (dV/ds_k times the gradient, then the sum over the CVs, then the one subtraction)
  const int c = blockIdx.x;
  if (c >= st.ch.n_chunks()) return;
  const int s = st.ch.structure(c);
  const int64_t i = st.ch.row(c, threadIdx.x);
  if (!st.ch.holds(s, i)) return;
  const double* coef = st.coef + kMetaCoef * (int64_t)s;
  double f[3], b[3] = {0.0, 0.0, 0.0};
  for (int a = 0; a < 3; ++a) f[a] = (double)forces[3 * i + a];
  bool biased = false;
  if (coef[0] != 0.0) {
    const double w = st.weights[i];
    for (int k = 0; k < st.n_cv; ++k) {
      const int m = st.membership[(int64_t)k * st.N + i];
      if (!m) continue;
      biased = true;
      const double* ck = coef + 1 + kCvCoef * k;
      double grad[3];
      if (p.kind[k] == M3G_CV_COORDINATION) {
        for (int a = 0; a < 3; ++a) grad[a] = st.grad[3 * ((int64_t)k * st.N + i) + a];
      } else {
        double share = 0.0;
        if (m & 1) share = w / ck[4];
        if (m & 2) share -= w / ck[5];
        for (int a = 0; a < 3; ++a) grad[a] = share * ck[1 + a];
      }
      for (int a = 0; a < 3; ++a) b[a] += ck[0] * grad[a];
    }
  }
  for (int a = 0; a < 3; ++a) forces_out[3 * i + a] = biased ? (float)(f[a] - b[a]) : forces[3 * i + a];   // untouched rows: the bits pass through
}

bool meta_sizes_ok(int64_t N, int64_t S, int64_t G, int32_t n_cv, int64_t max_hills) {
  return batch32_sizes_ok(N, S) && G >= 1 && G <= S && n_cv >= 1 && n_cv <= kMaxCv && max_hills >= 0 &&
         max_hills <= (int64_t)1 << 40;
}

// the parameters alone (the checks that need the batch are m3g_meta_init's)
bool meta_params_ok(const char* fn, const m3g_meta_params* p) {
  if (p->n_cv < 1 || p->n_cv > kMaxCv) { set_error("%s: n_cv must be 1 .. %d", fn, kMaxCv); return false; }
  if (p->max_hills < 0) { set_error("%s: max_hills must be >= 0", fn); return false; }
  for (int k = 0; k < p->n_cv; ++k) {
    switch (p->kind[k]) {
      case M3G_CV_DISTANCE: break;
      case M3G_CV_PROJECTION: {
        const double* n = p->direction[k];
        const double len2 = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
        if (!(std::fabs(len2 - 1.0) <= 1e-12)) { set_error("%s: the direction of CV %d is not a unit vector", fn, k); return false; }
        break;
      }
      case M3G_CV_COORDINATION:
        if (p->power[k] < 1 || p->power[k] > kMaxPower) { set_error("%s: the power p of CV %d must be 1 .. %d", fn, k, kMaxPower); return false; }
        if (!finite_positive(p->r0[k])) { set_error("%s: r0 of CV %d must be finite and > 0", fn, k); return false; }
        if (!finite_positive(p->r_cut[k])) { set_error("%s: r_cut of CV %d must be finite and > 0", fn, k); return false; }
        break;
      default: set_error("%s: unknown kind %d of CV %d", fn, p->kind[k], k); return false;
    }
  }
  return true;
}

// the smallest perpendicular width of a cell: V / max |a_j x a_k|
double min_width(const double* L) {
  double widest = 0.0;
  for (int a = 0; a < 3; ++a) {
    const double* b = L + 3 * ((a + 1) % 3);
    const double* c = L + 3 * ((a + 2) % 3);
    const double n[3] = {b[1] * c[2] - b[2] * c[1], b[2] * c[0] - b[0] * c[2], b[0] * c[1] - b[1] * c[0]};
    widest = std::fmax(widest, std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]));
  }
  return std::fabs(det3(L)) / widest;
}

// what every call after m3g_meta_init checks before it carves the view
int meta_call_ok(const char* fn, const m3g_meta_params* p, int64_t N, int64_t S, int64_t G, const void* state) {
  if (!p || !state || !meta_sizes_ok(N, S, G, p->n_cv, p->max_hills)) { set_error("%s: null argument or bad sizes", fn); return M3G_ERR_VALUE; }
  return meta_params_ok(fn, p) ? M3G_OK : M3G_ERR_VALUE;
}
}  // namespace
}  // namespace m3g

using namespace m3g;

extern "C" int m3g_meta_state_bytes(int64_t n_atoms, int64_t n_structs, int64_t n_groups, int32_t n_cv, int64_t max_hills, size_t* bytes) {
  if (!bytes || !meta_sizes_ok(n_atoms, n_structs, n_groups, n_cv, max_hills)) {
    set_error("m3g_meta_state_bytes: null argument or bad sizes (1 <= n_groups <= n_structs <= n_atoms, n_cv 1 .. %d, max_hills >= 0)", kMaxCv);
    return M3G_ERR_VALUE;
  }
  *bytes = meta_view(n_atoms, n_structs, n_groups, n_cv, max_hills, nullptr).bytes;
  return M3G_OK;
}

extern "C" int m3g_meta_state_view(int64_t n_atoms, int64_t n_structs, int64_t n_groups, int32_t n_cv, int64_t max_hills, size_t* gradient_offset) {
  if (!gradient_offset || !meta_sizes_ok(n_atoms, n_structs, n_groups, n_cv, max_hills)) {
    set_error("m3g_meta_state_view: null argument or bad sizes");
    return M3G_ERR_VALUE;
  }
  *gradient_offset = carve_offset(meta_view(n_atoms, n_structs, n_groups, n_cv, max_hills, nullptr).view.grad);   // (over a null state: the offsets)
  return M3G_OK;
}

extern "C" int m3g_meta_init(const m3g_meta_params* params, int64_t n_atoms, int64_t n_structs, int64_t n_groups, const int64_t* host_offsets,
                             const int64_t* host_group_offsets, const double* host_lattices, const uint8_t* host_membership,
                             const double* host_weights, const double* host_origins, const double* host_centres, const double* host_kappas,
                             const double* host_walls, const double* host_sigmas, const double* host_heights, const double* host_inv_kdt,
                             void* state, size_t state_bytes, void* stream_) {
  const char* fn = "m3g_meta_init";
  const int64_t N = n_atoms, S = n_structs, G = n_groups;
  if (!params || !host_offsets || !host_group_offsets || !host_lattices || !host_membership || !host_weights || !host_sigmas || !host_heights ||
      !host_inv_kdt || !state) {
    set_error("%s: null argument", fn);
    return M3G_ERR_VALUE;
  }
  if (!meta_params_ok(fn, params)) return M3G_ERR_VALUE;
  if (!meta_sizes_ok(N, S, G, params->n_cv, params->max_hills)) { set_error("%s: bad sizes (1 <= n_groups <= n_structs <= n_atoms)", fn); return M3G_ERR_VALUE; }
  const int n_cv = params->n_cv;
  if (!offsets_ok(fn, host_offsets, N, S)) return M3G_ERR_VALUE;
  if (!offsets_ok(fn, host_group_offsets, S, G, "group_offsets", "n_structs")) return M3G_ERR_VALUE;
  for (int64_t i = 0; i < N; ++i)
    if (!(std::isfinite(host_weights[i]) && host_weights[i] >= 0.0)) { set_error("%s: weight of atom %lld is not finite and >= 0", fn, (long long)i); return M3G_ERR_VALUE; }
  for (int64_t q = 0; q < n_cv * N; ++q)
    if (host_membership[q] > 3) { set_error("%s: membership must be 0 (none), 1 (A), 2 (B) or 3 (both)", fn); return M3G_ERR_VALUE; }
  for (int64_t s = 0; s < S; ++s) {
    if (!lattice_ok(fn, host_lattices + 9 * s, s)) return M3G_ERR_VALUE;
    for (int k = 0; k < n_cv; ++k) {
      int64_t count[2] = {0, 0};
      double total[2] = {0.0, 0.0};
      for (int64_t i = host_offsets[s]; i < host_offsets[s + 1]; ++i)
        for (int side = 0; side < 2; ++side)
          if (host_membership[k * N + i] & (1 << side)) { count[side] += 1; total[side] += host_weights[i]; }
      const bool centres = params->kind[k] != M3G_CV_COORDINATION, needs_b = params->kind[k] != M3G_CV_PROJECTION;
      if (count[0] == 0 || (needs_b && count[1] == 0)) {
        set_error("%s: CV %d of structure %lld has an empty group %s", fn, k, (long long)s, count[0] == 0 ? "A" : "B");
        return M3G_ERR_VALUE;
      }
      if (centres && (!(total[0] > 0.0) || (count[1] > 0 && !(total[1] > 0.0)))) {
        set_error("%s: CV %d of structure %lld has a group whose total weight is not > 0", fn, k, (long long)s);
        return M3G_ERR_VALUE;
      }
      if (params->kind[k] == M3G_CV_COORDINATION && params->r_cut[k] > 0.5 * min_width(host_lattices + 9 * s)) {
        set_error("%s: r_cut %g of CV %d exceeds half the smallest perpendicular width %g of the cell of structure %lld", fn, params->r_cut[k], k,
                  min_width(host_lattices + 9 * s), (long long)s);
        return M3G_ERR_VALUE;
      }
      const int64_t at = s * n_cv + k;
      if (host_origins)
        for (int a = 0; a < 3; ++a)
          if (!std::isfinite(host_origins[3 * at + a])) { set_error("%s: the origin of CV %d of structure %lld is not finite", fn, k, (long long)s); return M3G_ERR_VALUE; }
      if (host_kappas && !(std::isfinite(host_kappas[at]) && host_kappas[at] >= 0.0)) {
        set_error("%s: kappa of CV %d of structure %lld is not finite and >= 0", fn, k, (long long)s);
        return M3G_ERR_VALUE;
      }
      if (host_kappas && host_kappas[at] > 0.0 && !(host_centres && std::isfinite(host_centres[at]))) {
        set_error("%s: the restraint of CV %d of structure %lld has no finite centre", fn, k, (long long)s);
        return M3G_ERR_VALUE;
      }
      if (host_walls)
        for (int side = 0; side < 2; ++side) {
          const double at_s = host_walls[4 * at + 2 * side], kap = host_walls[4 * at + 2 * side + 1];
          if (!(std::isfinite(kap) && kap >= 0.0) || (kap > 0.0 && !std::isfinite(at_s))) {
            set_error("%s: a wall of CV %d of structure %lld needs a finite position and a finite kappa >= 0", fn, k, (long long)s);
            return M3G_ERR_VALUE;
          }
        }
    }
  }
  for (int64_t g = 0; g < G; ++g) {
    for (int k = 0; k < n_cv; ++k)
      if (!finite_positive(host_sigmas[g * n_cv + k])) { set_error("%s: sigma of CV %d of group %lld is not finite and > 0", fn, k, (long long)g); return M3G_ERR_VALUE; }
    if (!(std::isfinite(host_heights[g]) && host_heights[g] >= 0.0)) { set_error("%s: the hill height of group %lld is not finite and >= 0", fn, (long long)g); return M3G_ERR_VALUE; }
    if (!(std::isfinite(host_inv_kdt[g]) && host_inv_kdt[g] >= 0.0)) { set_error("%s: inv_kdt of group %lld is not finite and >= 0", fn, (long long)g); return M3G_ERR_VALUE; }
  }
  const auto [st, total] = meta_view(N, S, G, n_cv, params->max_hills, state);
  if (!state_fits(fn, state_bytes, total, true)) return M3G_ERR_SIZE;
  // the host image of everything between the chunk table and the per-call regions; deposit counts and flags start at zero
  std::vector<char> image(carve_offset(meta_view(N, S, G, n_cv, params->max_hills, nullptr).view.partial), 0);
  const MetaView im = meta_view(N, S, G, n_cv, params->max_hills, image.data()).view;
  std::memcpy(im.group_offsets, host_group_offsets, 8 * (G + 1));
  for (int64_t g = 0; g < G; ++g)
    for (int64_t s = host_group_offsets[g]; s < host_group_offsets[g + 1]; ++s) im.struct_group[s] = (int32_t)g;
  std::memcpy(im.membership, host_membership, n_cv * N);
  std::memcpy(im.weights, host_weights, 8 * N);
  std::memcpy(im.lat, host_lattices, 8 * 9 * S);
  for (int64_t s = 0; s < S; ++s) inv3(host_lattices + 9 * s, im.inv + 9 * s);   // rows = lattice vectors: fractional = cartesian . inverse
  if (host_origins) std::memcpy(im.origin, host_origins, 8 * 3 * n_cv * S);
  if (host_centres) std::memcpy(im.centre, host_centres, 8 * n_cv * S);
  if (host_kappas) std::memcpy(im.kappa, host_kappas, 8 * n_cv * S);
  if (host_walls) std::memcpy(im.walls, host_walls, 8 * 4 * n_cv * S);
  std::memcpy(im.sigma, host_sigmas, 8 * n_cv * G);
  std::memcpy(im.height, host_heights, 8 * G);
  std::memcpy(im.inv_kdt, host_inv_kdt, 8 * G);
  hipStream_t s = (hipStream_t)stream_;
  const size_t hills_begin = carve_offset(meta_view(N, S, G, n_cv, params->max_hills, nullptr).view.hill_centres);
  if (total > hills_begin) M3G_HIP_CHECK(hipMemsetAsync(st.hill_centres, 0, total - hills_begin, s));   // an empty list reads as zeros
  return upload_image(image, state, st.group_offsets, st.partial, st.ch, host_offsets, s);
}

extern "C" int m3g_meta_bias(const m3g_meta_params* params, int64_t n_atoms, int64_t n_structs, int64_t n_groups, void* state, size_t state_bytes,
                             const double* pos, const float* forces, float* forces_out, int32_t deposit, double* obs, void* stream_) {
  const int64_t N = n_atoms, S = n_structs, G = n_groups;
  if (int rc = meta_call_ok("m3g_meta_bias", params, N, S, G, state)) return rc;
  if (!pos || !forces || !forces_out) { set_error("m3g_meta_bias: missing pos, forces or forces_out"); return M3G_ERR_VALUE; }
  const auto [st, total] = meta_view(N, S, G, params->n_cv, params->max_hills, state);
  if (!state_fits("m3g_meta_bias", state_bytes, total)) return M3G_ERR_SIZE;
  hipStream_t s = (hipStream_t)stream_;
  const dim3 grid((unsigned)chunk_bound(N, S));   // workgroups beyond the table's chunk count return at once
  hipLaunchKernelGGL(k_meta_partials, grid, dim3(kChunkRows), 0, s, st, *params, pos);
  hipLaunchKernelGGL(k_meta_finalize, grid_for(S, kFinalizeWaves), dim3(kFinalizeWaves * kWave), 0, s, st, *params, deposit ? 1 : 0, obs);
  hipLaunchKernelGGL(k_meta_apply, grid, dim3(kChunkRows), 0, s, st, *params, forces, forces_out);
  M3G_RETURN_LAUNCH_STATUS();
}

extern "C" int m3g_meta_set_hills(const m3g_meta_params* params, int64_t n_atoms, int64_t n_structs, int64_t n_groups, void* state,
                                  size_t state_bytes, const int64_t* host_group_offsets, const int64_t* host_counts, const double* host_centres,
                                  const double* host_heights, void* stream_) {
  const char* fn = "m3g_meta_set_hills";
  const int64_t N = n_atoms, S = n_structs, G = n_groups;
  if (int rc = meta_call_ok(fn, params, N, S, G, state)) return rc;
  if (!host_group_offsets || !host_counts || !host_centres || !host_heights) { set_error("%s: null argument", fn); return M3G_ERR_VALUE; }
  if (!offsets_ok(fn, host_group_offsets, S, G, "group_offsets", "n_structs")) return M3G_ERR_VALUE;
  const int n_cv = params->n_cv;
  const int64_t H = params->max_hills;
  std::vector<int64_t> deposits(S);
  for (int64_t g = 0; g < G; ++g) {
    const int64_t R = host_group_offsets[g + 1] - host_group_offsets[g];
    if (host_counts[g] < 0 || host_counts[g] > H || host_counts[g] % R) {
      set_error("%s: the hill count of group %lld must be a multiple of its %lld walkers in 0 .. max_hills", fn, (long long)g, (long long)R);
      return M3G_ERR_VALUE;
    }
    for (int64_t h = 0; h < host_counts[g]; ++h) {
      bool ok = std::isfinite(host_heights[g * H + h]);
      for (int k = 0; k < n_cv; ++k) ok = ok && std::isfinite(host_centres[(g * H + h) * n_cv + k]);
      if (!ok) { set_error("%s: hill %lld of group %lld is not finite", fn, (long long)h, (long long)g); return M3G_ERR_VALUE; }
    }
    for (int64_t q = host_group_offsets[g]; q < host_group_offsets[g + 1]; ++q) deposits[q] = host_counts[g] / R;
  }
  const auto [st, total] = meta_view(N, S, G, n_cv, H, state);
  if (!state_fits(fn, state_bytes, total)) return M3G_ERR_SIZE;
  hipStream_t s = (hipStream_t)stream_;
  M3G_HIP_CHECK(hipMemcpyAsync(st.deposits, deposits.data(), 8 * S, hipMemcpyHostToDevice, s));
  if (G * H > 0) {
    M3G_HIP_CHECK(hipMemcpyAsync(st.hill_centres, host_centres, 8 * G * H * n_cv, hipMemcpyHostToDevice, s));
    M3G_HIP_CHECK(hipMemcpyAsync(st.hill_heights, host_heights, 8 * G * H, hipMemcpyHostToDevice, s));
  }
  M3G_HIP_CHECK(hipStreamSynchronize(s));   // (the caller's host arrays and the counts above)
  return M3G_OK;
}

extern "C" int m3g_meta_read(const m3g_meta_params* params, int64_t n_atoms, int64_t n_structs, int64_t n_groups, const void* state,
                             size_t state_bytes, int32_t* host_flags, int64_t* host_deposits, int64_t* host_hill_counts, double* host_centres,
                             double* host_heights, void* stream_) {
  const int64_t N = n_atoms, S = n_structs, G = n_groups;
  if (int rc = meta_call_ok("m3g_meta_read", params, N, S, G, state)) return rc;
  const auto [st, total] = meta_view(N, S, G, params->n_cv, params->max_hills, (void*)state);
  if (!state_fits("m3g_meta_read", state_bytes, total)) return M3G_ERR_SIZE;
  hipStream_t s = (hipStream_t)stream_;
  std::vector<int64_t> deposits(S), groups(G + 1);
  M3G_HIP_CHECK(read_back(host_flags, (const int32_t*)st.flags, S, s));
  M3G_HIP_CHECK(read_back(deposits.data(), (const int64_t*)st.deposits, S, s));
  M3G_HIP_CHECK(read_back(groups.data(), (const int64_t*)st.group_offsets, G + 1, s));
  M3G_HIP_CHECK(read_back(host_centres, (const double*)st.hill_centres, G * params->max_hills * params->n_cv, s));
  M3G_HIP_CHECK(read_back(host_heights, (const double*)st.hill_heights, G * params->max_hills, s));
  M3G_HIP_CHECK(hipStreamSynchronize(s));
  if (host_deposits) std::memcpy(host_deposits, deposits.data(), 8 * S);
  if (host_hill_counts)
    for (int64_t g = 0; g < G; ++g) host_hill_counts[g] = deposits[groups[g]] * (groups[g + 1] - groups[g]);   // (every walker of a group carries the same count)
  return M3G_OK;
}
