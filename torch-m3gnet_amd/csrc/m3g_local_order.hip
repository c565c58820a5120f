// Local-order observables of a batch, accumulated on the device while it is integrated (or fed any frames): per atom the Steinhardt
// bond-orientational order parameters q_l, their neighbour average qbar_l (Lechner-Dellago), the solid-like bonds of ten Wolde and
// Frenkel, and the connected clusters of solid-like atoms (definitions: include/m3gnet_hip.h, restated in
// tests/local_order_reference.py).  Positions and cells only.  Everything is fp64.  One m3g_lo_sample is, over the chunk table of
// m3g_chunks.h:
//   k_lo_neighbours  one workgroup per chunk, thread t on row t: the structure's 256-atom tiles in ascending order, staged in LDS as
//                    fractional coordinates; minimum image by rounding the fractional difference; r^2 of eight pairs at a time
//                    without a branch between them, the square root only where one of them may be in range; per pair with r < r_cut
//                    the neighbour's structure-local index and the unit bond vector into the atom's list (ascending j, at most
//                    M3G_LO_MAX_NEIGHBORS entries, the count uncapped).  Judges the cell (kMinDet, as m3g_scattering.hip), r_cut against
//                    half the smallest perpendicular width (as k_traj_rdf) and every distance: the flags of this sample, one word per
//                    chunk;
//   k_lo_qlm         one thread per atom: Y_lm of every bond from the Cartesian unit vector -- (x + i y)^m by repeated complex
//                    multiplication, P_l^m(z) / (1 - z^2)^(m/2) by its upward recurrence in l, the normalisation from a table of the
//                    init call; no trigonometric call and no division by 1 - z^2, so a bond along +-z is an ordinary input -- summed in
//                    list order in registers (a template per degree: 2 (l + 1) doubles); q_lm, q_l and the norm of solid_degree;
//   k_lo_average     one thread per atom, over its list: qbar_lm -> qbar_l per degree, then s_ij, n_conn, the solid flag and the
//                    starting label;
//   k_lo_cluster     one workgroup per structure: min-label propagation over the solid-solid list entries, the labels double-buffered
//                    in the state (every sweep reads one buffer and writes the other), with one pointer jump per atom and sweep (the
//                    label of its label), until a sweep changes nothing or n_s + 1 sweeps are done (plain min-propagation has
//                    converged by then on any graph, and the jump only lowers labels further); cluster sizes by integer atomics;
//   k_lo_accumulate  one workgroup per chunk of a structure without a flag: integer histograms of q_l, qbar_l and N_b (64-bit integer
//                    atomics: order-free), the sums of q_l, q_l^2, qbar_l, qbar_l^2 per species and degree and of N_b q_lm per degree
//                    in the fixed tree order of chunk_tree_reduce: one partial per chunk;
//   k_lo_series      one thread per structure: the chunk partials in chunk order into the moment sums, Q_l and the mean qbar_l into the
//                    series row `n_samples` (while it is below series_cap), the flags (sticky), n_samples or n_skipped.
// (The issue's five launches plus k_lo_series: the sums "in chunk order" need every chunk's partial, so they follow the launch that
// forms them.)  The tile loop of k_lo_neighbours is not cut into segments: profiles/local_order.txt has the timing that says why.
// No float atomics: every number depends on the structure's own rows only, so it is bitwise the same alone or in any batch.  The
// sample count lives in the state buffer (the two counters of m3g_trajectory.hip: every kernel reads one and at most one thread
// writes the other), hence no allocation, copy or wait in m3g_lo_sample: capture-safe.
#include <cmath>

#include "m3g_chunks.h"
#include "m3g_internal.h"

namespace m3g {
namespace {
constexpr int kMaxDegree = M3G_LO_MAX_DEGREE, kMaxDegrees = M3G_LO_MAX_DEGREES, kMaxNb = M3G_LO_MAX_NEIGHBORS;
constexpr int kMaxSpecies = M3G_LO_MAX_SPECIES, kMaxBins = M3G_LO_MAX_BINS, kMaxSeries = M3G_LO_MAX_SERIES;
constexpr int kOrders = kMaxDegree + 1;        // m = 0 .. 12: the row of one degree in the norm table and in a q_lm entry
constexpr int kQlm = 2 * kOrders;              // doubles of one (atom, degree) q_lm entry: (re, im) of every m
constexpr int kMoments = 4;                    // sums of q_l, q_l^2, qbar_l, qbar_l^2
constexpr int kClusterThreads = 1024;          // threads of k_lo_cluster: one workgroup walks a whole structure
constexpr int kPairBatch = 8;                  // pairs of k_lo_neighbours in flight per thread
constexpr int kNbBins = kMaxNb + 1;            // the coordination histogram: 0 .. 32
constexpr double kMinDet = 1e-12;              // a cell below it is singular to lattice_ok (m3g_chunks.h) as well
constexpr double kFourPi = 12.566370614359172;
enum { kDone = 0, kBegun = 1, kCounters = 4 };   // int64 words: samples finished, samples begun

struct LoView {
  int64_t N;
  int32_t M, D, B, K;
  ChunkView ch;
  const int32_t* species;   // [N]
  const double* r_cut;      // [S]
  const double* norm;       // [13][13]: sqrt((2l+1)/(4 pi) (l-m)!/(l+m)!) at [l][m]
  int64_t* ctr;
  int32_t* flags;           // [S]
  int64_t *n_samples, *n_skipped;
  unsigned long long *hist_q, *hist_qbar;   // [S][M][D][B]
  unsigned long long* hist_nb;              // [S][M][33]
  double* moments;          // [S][M][D][4]
  int64_t* series_counts;   // [S][K][3]
  double* series_order;     // [S][K][2][D]
  // what one sample writes before it reads it (nothing here is cleared by the init call)
  int32_t* chunk_flags;     // [C]: the flags this sample raised in the chunk
  int32_t* nb_count;        // [N], uncapped
  int32_t* nb_index;        // [32][N]: structure-local j of list entry k of atom i at [k][i]
  double* nb_unit;          // [32][3][N]
  double* qlm;              // [N][D][13][2]
  double *ql, *qbar;        // [N][D]
  double* norm_solid;       // [N]: |q_L(i)| of solid_degree
  int32_t *n_conn, *solid;  // [N]
  int32_t* label[2];        // [N] each: the two buffers of the propagation
  int32_t* label_out;       // [N]: the labels of the last sample
  int32_t* cluster_size;    // [N]: atoms of the cluster whose label is the row
  int32_t* cluster_counts;  // [S][3]: n_solid, n_clusters, largest_cluster of this sample
  double* partial;          // [C][M D 4 + D 26]
  unsigned long long* partial_nb;   // [C]: sum of N_b over the chunk
  __host__ __device__ int partial_stride() const { return M * D * kMoments + D * kQlm; }
};
Carved<LoView> lo_view(const m3g_lo_sizes& z, void* state) {
  const int64_t N = z.n_atoms, S = z.n_structs, M = z.max_species, D = z.n_degrees, B = z.hist_bins, K = z.series_cap;
  const int64_t C = chunk_bound(N, S);
  Carve c{state};
  LoView st{N, z.max_species, z.n_degrees, z.hist_bins, z.series_cap};
  st.ch = chunk_view(N, S, c);
  st.species = c.take<int32_t>(N);
  st.r_cut = c.take<double>(S);
  st.norm = c.take<double>(kOrders * kOrders);
  st.ctr = c.take<int64_t>(kCounters);   // the accumulators from here up to `chunk_flags` are cleared by the init call
  st.flags = c.take<int32_t>(S);
  st.n_samples = c.take<int64_t>(S);
  st.n_skipped = c.take<int64_t>(S);
  st.hist_q = c.take<unsigned long long>(S * M * D * B);
  st.hist_qbar = c.take<unsigned long long>(S * M * D * B);
  st.hist_nb = c.take<unsigned long long>(S * M * kNbBins);
  st.moments = c.take<double>(S * M * D * kMoments);
  st.series_counts = c.take<int64_t>(S * K * 3);
  st.series_order = c.take<double>(S * K * 2 * D);
  st.chunk_flags = c.take<int32_t>(C);
  st.nb_count = c.take<int32_t>(N);
  st.nb_index = c.take<int32_t>(kMaxNb * N);
  st.nb_unit = c.take<double>(3 * kMaxNb * N);
  st.qlm = c.take<double>(N * D * kQlm);
  st.ql = c.take<double>(N * D);
  st.qbar = c.take<double>(N * D);
  st.norm_solid = c.take<double>(N);
  st.n_conn = c.take<int32_t>(N);
  st.solid = c.take<int32_t>(N);
  st.label[0] = c.take<int32_t>(N);
  st.label[1] = c.take<int32_t>(N);
  st.label_out = c.take<int32_t>(N);
  st.cluster_size = c.take<int32_t>(N);
  st.cluster_counts = c.take<int32_t>(3 * S);
  st.partial = c.take<double>(C * st.partial_stride());
  st.partial_nb = c.take<unsigned long long>(C);
  return {st, c.off};
}

// the degrees of a sample, by value to every kernel
struct LoDegrees {
  int32_t l[kMaxDegrees];
  int32_t solid_slot, solid_bonds;   // the place of solid_degree among them
  double threshold;
};

// q_l (or |q_l| with scale = 1) from the m >= 0 half of q_lm: sqrt(scale (|q_l0|^2 + 2 sum_{m>0} |q_lm|^2))
template <int L>
__device__ inline double invariant(const double (&re)[L + 1], const double (&im)[L + 1], double scale) {
  double sum = 0.0;
#pragma unroll
  for (int m = L; m > 0; --m) sum += re[m] * re[m] + im[m] * im[m];
  return sqrt(scale * (re[0] * re[0] + im[0] * im[0] + 2.0 * sum));
}

// += Y_lm(x, y, z) for m = 0 .. L; nrm: the row of degree L in the norm table
template <int L>
__device__ inline void add_ylm(double x, double y, double z, const double* __restrict__ nrm, double (&re)[L + 1], double (&im)[L + 1]) {
  double cr = 1.0, ci = 0.0;   // (x + i y)^m = sin^m(theta) exp(i m phi)
  double pmm = 1.0;            // P_m^m / sin^m(theta) = (-1)^m (2m - 1)!!
#pragma unroll
  for (int m = 0; m <= L; ++m) {
    double p = pmm;            // P_l^m / sin^m upward in l from l = m
    if (m < L) {
      double prev = pmm;
      p = z * (double)(2 * m + 1) * pmm;
#pragma unroll
      for (int l = m + 2; l <= L; ++l) {
        const double next = ((double)(2 * l - 1) * z * p - (double)(l + m - 1) * prev) / (double)(l - m);
        prev = p;
        p = next;
      }
    }
    const double w = nrm[m] * p;
    re[m] += w * cr;
    im[m] += w * ci;
    const double nr = cr * x - ci * y;
    ci = cr * y + ci * x;
    cr = nr;
    pmm *= -(double)(2 * m + 1);
  }
}

__global__ void __launch_bounds__(kChunkRows) k_lo_neighbours(LoView st, const double* __restrict__ pos, const double* __restrict__ lattice) {
  __shared__ double fj[3][kChunkRows];
  const int c = blockIdx.x, t = threadIdx.x;
  if (c == 0 && t == 0) st.ctr[kBegun] = st.ctr[kDone] + 1;
  if (c >= st.ch.n_chunks()) return;
  const int s = st.ch.structure(c);
  const int64_t begin = st.ch.offsets[s], end = st.ch.offsets[s + 1], N = st.N;
  const double r_cut = st.r_cut[s];
  double l[9], cof[9];   // rows of l: the lattice vectors a0 a1 a2; rows of cof: a1 x a2, a2 x a0, a0 x a1
  for (int k = 0; k < 9; ++k) l[k] = lattice[9 * s + k];
  for (int k = 0; k < 3; ++k) {
    const double* u = l + 3 * ((k + 1) % 3);
    const double* v = l + 3 * ((k + 2) % 3);
    cof[3 * k] = u[1] * v[2] - u[2] * v[1];
    cof[3 * k + 1] = u[2] * v[0] - u[0] * v[2];
    cof[3 * k + 2] = u[0] * v[1] - u[1] * v[0];
  }
  const double det = l[0] * cof[0] + l[1] * cof[1] + l[2] * cof[2];
  const int64_t i = st.ch.row(c, t);
  const bool mine = st.ch.holds(s, i);
  int flags = 0;   // the same word in every thread so far
  if (!(isfinite(det) && fabs(det) >= kMinDet)) {   // no fractional coordinate exists: nobody has a neighbour
    if (mine) st.nb_count[i] = 0;
    if (t == 0) st.chunk_flags[c] = M3G_LO_CELL;
    return;
  }
  {
    double widest = 0.0;   // max |a_j x a_k|
    for (int k = 0; k < 3; ++k) widest = fmax(widest, sqrt(cof[3 * k] * cof[3 * k] + cof[3 * k + 1] * cof[3 * k + 1] + cof[3 * k + 2] * cof[3 * k + 2]));
    // (1 + 1e-12: the rounding of the width itself, so r_cut = a / 2 of a cubic cell passes; a NaN cell sets the flag too)
    if (!(r_cut <= 0.5 * (fabs(det) / widest) * (1.0 + 1e-12))) flags |= M3G_LO_RANGE;
  }
  double fi[3] = {0.0, 0.0, 0.0};
  if (mine) {   // fractional coordinates: r = f0 a0 + f1 a1 + f2 a2, f_k = r . c_k / det
    const double* r = pos + 3 * i;
    for (int k = 0; k < 3; ++k) fi[k] = (r[0] * cof[3 * k] + r[1] * cof[3 * k + 1] + r[2] * cof[3 * k + 2]) / det;
  }
  const double near2 = r_cut * r_cut * (1.0 + 1e-9);
  int count = 0;
  int bad = mine && !(isfinite(fi[0]) && isfinite(fi[1]) && isfinite(fi[2]));   // (an atom alone in its structure has no pair to show it)
  for (int c2 = st.ch.chunks_begin(s); c2 < st.ch.chunks_end(s); ++c2) {   // the structure's tiles, ascending
    const int64_t j0 = st.ch.row(c2, 0);
    const int nj = (int)(end - j0 < kChunkRows ? end - j0 : kChunkRows);
    __syncthreads();   // (the tile before has been read)
    if (t < nj) {
      const double* r = pos + 3 * (j0 + t);
      for (int k = 0; k < 3; ++k) fj[k][t] = (r[0] * cof[3 * k] + r[1] * cof[3 * k + 1] + r[2] * cof[3 * k + 2]) / det;
    }
    __syncthreads();
    if (!mine) continue;
    for (int j = 0; j < nj; j += kPairBatch) {   // every LDS address is the same for the whole wave
      // kPairBatch pairs at a time without a branch between them (one wave per SIMD: nothing else hides the latency of a pair's
      // chain), then one test whether any of them needs a closer look; past the tile's end the last row stands in and is not looked at
      double x[kPairBatch], y[kPairBatch], z[kPairBatch], r2[kPairBatch];
      bool look = false;
#pragma unroll
      for (int b = 0; b < kPairBatch; ++b) {
        const int row = j + b < nj ? j + b : nj - 1;
        double d[3];
        for (int k = 0; k < 3; ++k) {
          d[k] = fj[k][row] - fi[k];
          d[k] -= rint(d[k]);   // the minimum image of every pair closer than half the smallest perpendicular width
        }
        x[b] = d[0] * l[0] + d[1] * l[3] + d[2] * l[6];
        y[b] = d[0] * l[1] + d[1] * l[4] + d[2] * l[7];
        z[b] = d[0] * l[2] + d[1] * l[5] + d[2] * l[8];
        r2[b] = x[b] * x[b] + y[b] * y[b] + z[b] * z[b];
        look = look || !(r2[b] >= near2 && r2[b] < INFINITY);   // (a NaN fails the comparisons)
      }
      if (!look) continue;
#pragma unroll
      for (int b = 0; b < kPairBatch; ++b) {
        if (j + b >= nj) break;
        // the square root (a long dependent chain) only for the few pairs that may be in range: r^2 a hair beyond r_cut^2 still
        // includes every r < r_cut, and r itself decides
        if (r2[b] < near2 && r2[b] > 0.0) {
          const double r = sqrt(r2[b]);
          if (r < r_cut) {
            if (count < kMaxNb) {
              st.nb_index[(size_t)count * N + i] = (int32_t)(j0 - begin) + j + b;
              double* u = st.nb_unit + (size_t)(3 * count) * N + i;
              u[0] = x[b] / r;
              u[N] = y[b] / r;
              u[2 * N] = z[b] / r;
            }
            ++count;
          }
        } else if (!(r2[b] > 0.0 && r2[b] < INFINITY) && j0 + j + b != i) {   // (the atom itself is at r = 0)
          bad = 1;
        }
      }
    }
  }
  if (mine) st.nb_count[i] = count;
  const int over = __syncthreads_or(mine && count > kMaxNb), nonfinite = __syncthreads_or(bad);
  if (t == 0) st.chunk_flags[c] = flags | (over ? M3G_LO_NEIGHBORS : 0) | (nonfinite ? M3G_LO_NONFINITE : 0);
}

// the list of atom i: its stored length
__device__ inline int stored(const LoView& st, int64_t i) {
  const int n = st.nb_count[i];
  return n < 0 ? 0 : n < kMaxNb ? n : kMaxNb;   // (a count is never negative; the clamp keeps every list index inside the list)
}

template <int L>
__device__ inline void qlm_of_degree(const LoView& st, int64_t i, int slot, bool is_solid_degree) {
  double re[L + 1], im[L + 1];
#pragma unroll
  for (int m = 0; m <= L; ++m) re[m] = im[m] = 0.0;
  const int n = stored(st, i);
  const int64_t N = st.N;
  const double* nrm = st.norm + L * kOrders;
  for (int k = 0; k < n; ++k) {   // list order: ascending j
    const double* u = st.nb_unit + (size_t)(3 * k) * N + i;
    add_ylm<L>(u[0], u[N], u[2 * N], nrm, re, im);
  }
  if (n > 0) {
    const double count = (double)n;
#pragma unroll
    for (int m = 0; m <= L; ++m) {
      re[m] /= count;
      im[m] /= count;
    }
  }
  double* out = st.qlm + ((size_t)i * st.D + slot) * kQlm;
#pragma unroll
  for (int m = 0; m < kOrders; ++m) {
    out[2 * m] = m <= L ? re[m < L ? m : L] : 0.0;
    out[2 * m + 1] = m <= L ? im[m < L ? m : L] : 0.0;
  }
  st.ql[(size_t)i * st.D + slot] = invariant<L>(re, im, kFourPi / (double)(2 * L + 1));
  if (is_solid_degree) st.norm_solid[i] = invariant<L>(re, im, 1.0);
}

// one case per degree: the register arrays of a degree are static
#define M3G_LO_FOR_DEGREE(l, CALL)                                                                                            \
  switch (l) {                                                                                                                \
    case 1: CALL(1); break; case 2: CALL(2); break; case 3: CALL(3); break; case 4: CALL(4); break;                           \
    case 5: CALL(5); break; case 6: CALL(6); break; case 7: CALL(7); break; case 8: CALL(8); break;                           \
    case 9: CALL(9); break; case 10: CALL(10); break; case 11: CALL(11); break; case 12: CALL(12); break;                     \
    default: break;                                                                                                           \
  }

__global__ void __launch_bounds__(kChunkRows) k_lo_qlm(LoView st, LoDegrees deg) {
  const int c = blockIdx.x, t = threadIdx.x;
  if (c >= st.ch.n_chunks()) return;
  const int64_t i = st.ch.row(c, t);
  if (!st.ch.holds(st.ch.structure(c), i)) return;
  for (int slot = 0; slot < st.D; ++slot) {
#define M3G_LO_QLM(L) qlm_of_degree<L>(st, i, slot, slot == deg.solid_slot)
    M3G_LO_FOR_DEGREE(deg.l[slot], M3G_LO_QLM)
#undef M3G_LO_QLM
  }
}

// qbar_l of atom i for the degree in `slot`; with `bonds` the connected bonds of i as well (the degree is solid_degree)
template <int L>
__device__ inline int average_of_degree(const LoView& st, int64_t i, int64_t begin, int slot, bool bonds, double threshold) {
  double re[L + 1], im[L + 1], mine_re[L + 1], mine_im[L + 1];
  const double* own = st.qlm + ((size_t)i * st.D + slot) * kQlm;
#pragma unroll
  for (int m = 0; m <= L; ++m) {
    re[m] = mine_re[m] = own[2 * m];
    im[m] = mine_im[m] = own[2 * m + 1];
  }
  const int n = stored(st, i);
  const int64_t N = st.N;
  const double norm_i = bonds ? st.norm_solid[i] : 0.0;
  int connected = 0;
  for (int k = 0; k < n; ++k) {   // list order: ascending j
    const int64_t j = begin + st.nb_index[(size_t)k * N + i];
    const double* other = st.qlm + ((size_t)j * st.D + slot) * kQlm;
    double dot = 0.0;
#pragma unroll
    for (int m = L; m >= 0; --m) {
      const double a = other[2 * m], b = other[2 * m + 1];
      re[m] += a;
      im[m] += b;
      const double term = mine_re[m] * a + mine_im[m] * b;   // Re q_Lm(i) q_Lm*(j); the term of -m is the same
      dot += m > 0 ? 2.0 * term : term;
    }
    if (bonds) {
      const double norm_j = st.norm_solid[j];
      if (norm_i > 0.0 && norm_j > 0.0 && dot / (norm_i * norm_j) > threshold) ++connected;
    }
  }
  const double count = (double)(n + 1);
#pragma unroll
  for (int m = 0; m <= L; ++m) {
    re[m] /= count;
    im[m] /= count;
  }
  st.qbar[(size_t)i * st.D + slot] = invariant<L>(re, im, kFourPi / (double)(2 * L + 1));
  return connected;
}

__global__ void __launch_bounds__(kChunkRows) k_lo_average(LoView st, LoDegrees deg) {
  const int c = blockIdx.x, t = threadIdx.x;
  if (c >= st.ch.n_chunks()) return;
  const int s = st.ch.structure(c);
  const int64_t i = st.ch.row(c, t), begin = st.ch.offsets[s];
  if (!st.ch.holds(s, i)) return;
  int connected = 0;
  for (int slot = 0; slot < st.D; ++slot) {
    const bool bonds = slot == deg.solid_slot;
    int found = 0;
#define M3G_LO_AVERAGE(L) found = average_of_degree<L>(st, i, begin, slot, bonds, deg.threshold)
    M3G_LO_FOR_DEGREE(deg.l[slot], M3G_LO_AVERAGE)
#undef M3G_LO_AVERAGE
    if (bonds) connected = found;
  }
  const int solid = connected >= deg.solid_bonds ? 1 : 0;
  st.n_conn[i] = connected;
  st.solid[i] = solid;
  st.label[0][i] = solid ? (int32_t)(i - begin) : -1;
  st.cluster_size[i] = 0;
}

__global__ void __launch_bounds__(kClusterThreads) k_lo_cluster(LoView st) {
  __shared__ int counts_sh[3];   // n_solid, n_clusters, largest_cluster
  const int64_t s = blockIdx.x;
  const int t = threadIdx.x;
  const int64_t begin = st.ch.offsets[s], N = st.N;
  const int n = (int)(st.ch.offsets[s + 1] - begin);   // (a structure's rows fit int32_t: the init call checked)
  if (t < 3) counts_sh[t] = 0;
  int from = 0;
  for (int sweep = 0; sweep <= n; ++sweep) {   // at most n + 1 sweeps, whatever the lists hold
    const int32_t* in = st.label[from];
    int32_t* out = st.label[1 - from];
    int changed = 0;
    for (int a = t; a < n; a += kClusterThreads) {
      const int64_t i = begin + a;
      int32_t best = in[i];
      if (st.solid[i]) {
        const int len = stored(st, i);
        for (int k = 0; k < len; ++k) {
          const int b = st.nb_index[(size_t)k * N + i];
          if (b < 0 || b >= n || !st.solid[begin + b]) continue;   // (an index is always inside the structure; the test keeps it so)
          const int32_t other = in[begin + b];
          best = other < best ? other : best;
        }
        // one pointer jump: a label is the index of an atom of the same cluster, whose own label is no larger and belongs to the
        // cluster too -- the fixed point is the same (every atom at the smallest index), reached in fewer sweeps
        if (best >= 0 && best < n) {
          const int32_t above = in[begin + best];
          best = above >= 0 && above < best ? above : best;
        }
        changed |= best != in[i];
      }
      out[i] = best;
    }
    from = 1 - from;
    if (!__syncthreads_or(changed)) break;   // (the barrier also orders this sweep's stores before the next sweep's loads)
  }
  const int32_t* fin = st.label[from];
  for (int a = t; a < n; a += kClusterThreads) {
    const int32_t lab = fin[begin + a];
    st.label_out[begin + a] = lab;
    if (lab >= 0 && lab < n) {
      atomicAdd(&st.cluster_size[begin + lab], 1);
      atomicAdd(&counts_sh[0], 1);
      if (lab == a) atomicAdd(&counts_sh[1], 1);
    }
  }
  __syncthreads();   // every count of this structure's clusters is in (the counts belong to this workgroup alone)
  for (int a = t; a < n; a += kClusterThreads) {
    const int size = __hip_atomic_load(&st.cluster_size[begin + a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (size > 0) atomicMax(&counts_sh[2], size);
  }
  __syncthreads();
  if (t < 3) st.cluster_counts[3 * s + t] = counts_sh[t];
}

// the flags this sample raised in structure s: every chunk's word, by every thread alike
__device__ inline int sample_flags(const LoView& st, int s) {
  int flags = 0;
  for (int c = st.ch.chunks_begin(s); c < st.ch.chunks_end(s); ++c) flags |= st.chunk_flags[c];
  return flags;
}

__device__ inline int bin_of(double q, int B) {   // B bins on [0, 1], the last one closed
  int bin = (int)(q * (double)B);
  return bin < 0 ? 0 : bin < B ? bin : B - 1;
}

__global__ void __launch_bounds__(kChunkRows) k_lo_accumulate(LoView st, LoDegrees deg) {
  __shared__ double sh[kMoments][kChunkRows];
  __shared__ unsigned long long nb_sh;
  const int c = blockIdx.x, t = threadIdx.x;
  if (c >= st.ch.n_chunks()) return;
  const int s = st.ch.structure(c);
  if (sample_flags(st, s)) return;   // (the whole workgroup alike)
  const int M = st.M, D = st.D, B = st.B;
  const int64_t i = st.ch.row(c, t);
  const bool mine = st.ch.holds(s, i);
  int sp = -1, nb = 0;
  if (t == 0) nb_sh = 0ull;
  __syncthreads();
  if (mine) {
    sp = st.species[i];
    nb = stored(st, i);   // (no flag: the count is at most 32)
    atomicAdd(&st.hist_nb[((size_t)s * M + sp) * kNbBins + nb], 1ull);
    atomicAdd(&nb_sh, (unsigned long long)nb);
    for (int d = 0; d < D; ++d) {
      const size_t row = (((size_t)s * M + sp) * D + d) * B;
      atomicAdd(&st.hist_q[row + bin_of(st.ql[(size_t)i * D + d], B)], 1ull);
      atomicAdd(&st.hist_qbar[row + bin_of(st.qbar[(size_t)i * D + d], B)], 1ull);
    }
  }
  double* partial = st.partial + (size_t)c * st.partial_stride();
  for (int a = 0; a < M; ++a)
    for (int d = 0; d < D; ++d) {
      const double q = sp == a ? st.ql[(size_t)i * D + d] : 0.0, qb = sp == a ? st.qbar[(size_t)i * D + d] : 0.0;
      const double val[kMoments] = {q, q * q, qb, qb * qb};
      chunk_tree_reduce<kMoments>(sh, val, t);
      if (t < kMoments) partial[(a * D + d) * kMoments + t] = sh[t][0];
      __syncthreads();
    }
  for (int d = 0; d < D; ++d)   // sum_i N_b(i) q_lm(i), four columns (two orders) at a time
    for (int m = 0; m < kOrders + 1; m += 2) {
      double val[kMoments] = {0.0, 0.0, 0.0, 0.0};
      if (mine)
        for (int k = 0; k < kMoments; ++k)
          if (2 * m + k < kQlm) val[k] = (double)nb * st.qlm[((size_t)i * D + d) * kQlm + 2 * m + k];
      chunk_tree_reduce<kMoments>(sh, val, t);
      if (t < kMoments && 2 * m + t < kQlm) partial[M * D * kMoments + d * kQlm + 2 * m + t] = sh[t][0];
      __syncthreads();
    }
  if (t == 0) st.partial_nb[c] = nb_sh;
}

__global__ void __launch_bounds__(kChunkRows) k_lo_series(LoView st, LoDegrees deg) {
  const int64_t s = (int64_t)blockIdx.x * kChunkRows + threadIdx.x;
  if (s == 0) st.ctr[kDone] = st.ctr[kBegun];
  if (s >= st.ch.S) return;
  const int flags = sample_flags(st, (int)s);
  if (flags) {
    st.flags[s] |= flags;
    st.n_skipped[s] += 1;
    return;
  }
  const int M = st.M, D = st.D, stride = st.partial_stride();
  const int first = st.ch.chunks_begin(s), last = st.ch.chunks_end(s);
  const int64_t slot = st.n_samples[s];
  const bool keep = slot < st.K;
  const double atoms = (double)(st.ch.offsets[s + 1] - st.ch.offsets[s]);
  unsigned long long bonds = 0ull;
  for (int c = first; c < last; ++c) bonds += st.partial_nb[c];
  double* order = st.series_order + ((size_t)s * st.K + (keep ? slot : 0)) * 2 * D;
  for (int d = 0; d < D; ++d) {
    double qbar_all = 0.0;   // over the species in species order
    for (int a = 0; a < M; ++a)
      for (int k = 0; k < kMoments; ++k) {
        double sum = 0.0;
        for (int c = first; c < last; ++c) sum += st.partial[(size_t)c * stride + (a * D + d) * kMoments + k];   // chunk order
        st.moments[(((size_t)s * M + a) * D + d) * kMoments + k] += sum;
        if (k == 2) qbar_all += sum;
      }
    const int l = deg.l[d];
    double power = 0.0;   // |Q_l0|^2 + 2 sum_{m>0} |Q_lm|^2, times bonds^2
    for (int m = l; m >= 0; --m) {
      double re = 0.0, im = 0.0;
      for (int c = first; c < last; ++c) {
        const double* p = st.partial + (size_t)c * stride + M * D * kMoments + d * kQlm + 2 * m;
        re += p[0];
        im += p[1];
      }
      const double term = re * re + im * im;
      power += m > 0 ? 2.0 * term : term;
    }
    if (keep) {
      order[d] = bonds ? sqrt(kFourPi / (double)(2 * l + 1) * power) / (double)bonds : 0.0;
      order[D + d] = qbar_all / atoms;
    }
  }
  if (keep)
    for (int k = 0; k < 3; ++k) st.series_counts[((size_t)s * st.K + slot) * 3 + k] = st.cluster_counts[3 * s + k];
  st.n_samples[s] = slot + 1;
}

// nullptr when the sizes (and, where given, the parameters) are valid, else what is wrong with them
const char* lo_error(const m3g_lo_sizes* z, const m3g_lo_params* p, bool with_params) {
  if (!z || (with_params && !p)) return "null sizes or parameters";
  if (!batch32_sizes_ok(z->n_atoms, z->n_structs)) return "bad sizes";
  if (z->max_species < 1 || z->max_species > kMaxSpecies) return "max_species must be 1 .. 4";
  if (z->n_degrees < 1 || z->n_degrees > kMaxDegrees) return "n_degrees must be 1 .. 3";
  if (z->hist_bins < 1 || z->hist_bins > kMaxBins) return "hist_bins must be 1 .. 1024";
  if (z->series_cap < 1 || z->series_cap > kMaxSeries) return "series_cap must be 1 .. 65536";
  if (!with_params) return nullptr;
  bool found = false;
  for (int d = 0; d < z->n_degrees; ++d) {
    if (p->degrees[d] < 1 || p->degrees[d] > kMaxDegree) return "every degree must be 1 .. 12";
    for (int e = 0; e < d; ++e)
      if (p->degrees[e] == p->degrees[d]) return "the degrees must be distinct";
    found = found || p->degrees[d] == p->solid_degree;
  }
  if (!found) return "solid_degree must be one of the degrees";
  if (p->solid_bonds < 1 || p->solid_bonds > kMaxNb) return "solid_bonds must be 1 .. 32";
  if (!(p->solid_threshold >= -1.0 && p->solid_threshold <= 1.0)) return "solid_threshold must be -1 .. 1";
  return nullptr;
}

LoDegrees degrees_of(const m3g_lo_sizes& z, const m3g_lo_params& p) {
  LoDegrees deg{{0, 0, 0}, 0, p.solid_bonds, p.solid_threshold};
  for (int d = 0; d < z.n_degrees; ++d) {
    deg.l[d] = p.degrees[d];
    if (p.degrees[d] == p.solid_degree) deg.solid_slot = d;
  }
  return deg;
}
}  // namespace
}  // namespace m3g

using namespace m3g;

extern "C" int m3g_lo_state_bytes(const m3g_lo_sizes* sizes, size_t* bytes) {
  if (const char* why = lo_error(sizes, nullptr, false)) { set_error("m3g_lo_state_bytes: %s", why); return M3G_ERR_VALUE; }
  if (!bytes) { set_error("m3g_lo_state_bytes: null argument"); return M3G_ERR_VALUE; }
  *bytes = lo_view(*sizes, nullptr).bytes;
  return M3G_OK;
}

extern "C" int m3g_lo_init(const m3g_lo_sizes* sizes, const m3g_lo_params* params, const int64_t* host_offsets, const int32_t* host_species,
                           const double* host_r_cut, void* state, size_t state_bytes, void* stream_) {
  if (const char* why = lo_error(sizes, params, true)) { set_error("m3g_lo_init: %s", why); return M3G_ERR_VALUE; }
  if (!host_offsets || !host_species || !host_r_cut || !state) { set_error("m3g_lo_init: null argument"); return M3G_ERR_VALUE; }
  const int64_t N = sizes->n_atoms, S = sizes->n_structs;
  if (!offsets_ok("m3g_lo_init", host_offsets, N, S)) return M3G_ERR_VALUE;
  for (int64_t s = 0; s < S; ++s) {
    if (!structure_fits_int32("m3g_lo_init", host_offsets, s)) return M3G_ERR_VALUE;
    if (!finite_positive(host_r_cut[s])) { set_error("m3g_lo_init: r_cut of structure %lld is not finite and > 0", (long long)s); return M3G_ERR_VALUE; }
  }
  for (int64_t i = 0; i < N; ++i)
    if (host_species[i] < 0 || host_species[i] >= sizes->max_species) {
      set_error("m3g_lo_init: species index of atom %lld is outside 0 .. max_species - 1", (long long)i);
      return M3G_ERR_VALUE;
    }
  const auto [st, total] = lo_view(*sizes, state);
  if (!state_fits("m3g_lo_init", state_bytes, total, true)) return M3G_ERR_SIZE;
  std::vector<double> norm(kOrders * kOrders, 0.0);   // sqrt((2l+1)/(4 pi) (l-m)!/(l+m)!)
  for (int l = 0; l <= kMaxDegree; ++l)
    for (int m = 0; m <= l; ++m) {
      long double ratio = 1.0L;   // (l-m)!/(l+m)!
      for (int k = l - m + 1; k <= l + m; ++k) ratio /= (long double)k;
      norm[l * kOrders + m] = (double)sqrtl((long double)(2 * l + 1) / (4.0L * 3.14159265358979323846264338327950288L) * ratio);
    }
  const ChunkTable table(host_offsets, S);
  hipStream_t s = (hipStream_t)stream_;
  if (int rc = table.upload(st.ch, host_offsets, s)) return rc;
  M3G_HIP_CHECK(hipMemcpyAsync((void*)st.species, host_species, 4 * N, hipMemcpyHostToDevice, s));
  M3G_HIP_CHECK(hipMemcpyAsync((void*)st.r_cut, host_r_cut, 8 * S, hipMemcpyHostToDevice, s));
  M3G_HIP_CHECK(hipMemcpyAsync((void*)st.norm, norm.data(), 8 * norm.size(), hipMemcpyHostToDevice, s));
  M3G_HIP_CHECK(hipMemsetAsync(st.ctr, 0, (size_t)((const char*)st.chunk_flags - (const char*)st.ctr), s));
  M3G_HIP_CHECK(hipStreamSynchronize(s));   // (the host tables above go out of scope)
  return M3G_OK;
}

extern "C" int m3g_lo_sample(const m3g_lo_sizes* sizes, const m3g_lo_params* params, void* state, size_t state_bytes, const double* pos,
                             const double* lattice, void* stream_) {
  if (const char* why = lo_error(sizes, params, true)) { set_error("m3g_lo_sample: %s", why); return M3G_ERR_VALUE; }
  if (!state || !pos || !lattice) { set_error("m3g_lo_sample: null argument"); return M3G_ERR_VALUE; }
  const auto [st, total] = lo_view(*sizes, state);
  if (!state_fits("m3g_lo_sample", state_bytes, total)) return M3G_ERR_SIZE;
  const int64_t N = sizes->n_atoms, S = sizes->n_structs;
  hipStream_t s = (hipStream_t)stream_;
  const dim3 chunks((unsigned)chunk_bound(N, S)), rows(kChunkRows);   // workgroups beyond the table's chunk count return at once
  const LoDegrees deg = degrees_of(*sizes, *params);
  const auto sv = st;   // (a structured binding cannot be captured)
  hipLaunchKernelGGL(k_lo_neighbours, chunks, rows, 0, s, sv, pos, lattice);
  hipLaunchKernelGGL(k_lo_qlm, chunks, rows, 0, s, sv, deg);
  hipLaunchKernelGGL(k_lo_average, chunks, rows, 0, s, sv, deg);
  hipLaunchKernelGGL(k_lo_cluster, dim3((unsigned)S), dim3(kClusterThreads), 0, s, sv);
  hipLaunchKernelGGL(k_lo_accumulate, chunks, rows, 0, s, sv, deg);
  hipLaunchKernelGGL(k_lo_series, grid_for(S, kChunkRows), rows, 0, s, sv, deg);
  M3G_RETURN_LAUNCH_STATUS();
}

extern "C" int m3g_lo_read(const m3g_lo_sizes* sizes, const void* state, size_t state_bytes, uint64_t* host_hist_q, uint64_t* host_hist_qbar,
                           uint64_t* host_hist_nb, double* host_moments, int64_t* host_series_counts, double* host_series_order,
                           int64_t* host_n_samples, int64_t* host_n_skipped, int32_t* host_flags, void* stream_) {
  if (const char* why = lo_error(sizes, nullptr, false)) { set_error("m3g_lo_read: %s", why); return M3G_ERR_VALUE; }
  if (!state) { set_error("m3g_lo_read: null argument"); return M3G_ERR_VALUE; }
  const auto [st, total] = lo_view(*sizes, (void*)state);
  if (!state_fits("m3g_lo_read", state_bytes, total)) return M3G_ERR_SIZE;
  const size_t S = sizes->n_structs, M = sizes->max_species, D = sizes->n_degrees, B = sizes->hist_bins, K = sizes->series_cap;
  return read_all((hipStream_t)stream_,
                  {rb((unsigned long long*)host_hist_q, (const unsigned long long*)st.hist_q, S * M * D * B),
                   rb((unsigned long long*)host_hist_qbar, (const unsigned long long*)st.hist_qbar, S * M * D * B),
                   rb((unsigned long long*)host_hist_nb, (const unsigned long long*)st.hist_nb, S * M * kNbBins),
                   rb(host_moments, (const double*)st.moments, S * M * D * kMoments),
                   rb(host_series_counts, (const int64_t*)st.series_counts, S * K * 3),
                   rb(host_series_order, (const double*)st.series_order, S * K * 2 * D),
                   rb(host_n_samples, (const int64_t*)st.n_samples, S), rb(host_n_skipped, (const int64_t*)st.n_skipped, S),
                   rb(host_flags, (const int32_t*)st.flags, S)});
}

extern "C" int m3g_lo_frame(const m3g_lo_sizes* sizes, const void* state, size_t state_bytes, double* host_qlm, double* host_ql,
                            double* host_qbar, int32_t* host_n_neighbors, int32_t* host_n_conn, int32_t* host_solid, int32_t* host_label,
                            void* stream_) {
  if (const char* why = lo_error(sizes, nullptr, false)) { set_error("m3g_lo_frame: %s", why); return M3G_ERR_VALUE; }
  if (!state) { set_error("m3g_lo_frame: null argument"); return M3G_ERR_VALUE; }
  const auto [st, total] = lo_view(*sizes, (void*)state);
  if (!state_fits("m3g_lo_frame", state_bytes, total)) return M3G_ERR_SIZE;
  const size_t N = sizes->n_atoms, D = sizes->n_degrees;
  hipStream_t s = (hipStream_t)stream_;
  int64_t ctr[kCounters];
  M3G_HIP_CHECK(hipMemcpyAsync(ctr, st.ctr, sizeof(ctr), hipMemcpyDeviceToHost, s));
  M3G_HIP_CHECK(hipStreamSynchronize(s));
  if (ctr[kDone] < 1) { set_error("m3g_lo_frame: no sample has been taken"); return M3G_ERR_VALUE; }
  return read_all(s, {rb(host_qlm, (const double*)st.qlm, N * D * kQlm), rb(host_ql, (const double*)st.ql, N * D),
                      rb(host_qbar, (const double*)st.qbar, N * D), rb(host_n_neighbors, (const int32_t*)st.nb_count, N),
                      rb(host_n_conn, (const int32_t*)st.n_conn, N), rb(host_solid, (const int32_t*)st.solid, N),
                      rb(host_label, (const int32_t*)st.label_out, N)});
}
