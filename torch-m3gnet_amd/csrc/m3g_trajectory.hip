// Trajectory observables of a batch, accumulated on the device while it is integrated (or fed any frames): the radial distribution
// function as integer pair counts per species pair, and the mean-square displacement / velocity autocorrelation per species over a
// ring of the last n_lags sampled frames.  One m3g_traj_sample is, over the chunk table of m3g_chunks.h:
//   k_traj_rdf       (rdf_bins > 0) one workgroup per pair of 256-atom tiles (I <= J) of ONE structure, from a table built by the init
//                    call: thread t keeps atom t of tile I in registers, tile J (fractional coordinates, species) is staged in LDS;
//                    minimum image by rounding the fractional difference in fp64; integer counts, privatised in LDS where they fit,
//                    flushed with 64-bit integer atomics (order-free: bitwise reproducible).  The first pair of a structure adds the
//                    cell volume and checks r_max against half the smallest perpendicular width of the CURRENT cell;
//   k_traj_com       (n_lags > 0, remove_com) one workgroup per chunk: partial sums of m, m r, m v in a fixed tree order;
//   k_traj_store     one workgroup per chunk: the full-step velocity v + kick kappa F / m, minus the structure's centre of mass (the
//                    chunk partials in chunk order), into the ring slot of this sample;
//   k_traj_partials  grid (chunk, block of kLagBlock lags): per stored lag and species the sums of |r_now - r_old|^2 and v_now . v_old
//                    over the chunk's rows in the fixed tree order -- a streaming read of the ring, three 16-byte loads per atom and lag;
//   k_traj_finalize  one thread per (structure, lag, species): the chunk partials in chunk order into msd / vacf, lag_count += 1.
// No float atomics: every number depends on the structure's own rows only, so it is bitwise the same alone or in any batch.  The
// ring position lives in the state buffer (two counters: every kernel reads one and at most one thread writes the other, so no
// launch reads a word that the same launch writes), hence no allocation, copy or wait in m3g_traj_sample: capture-safe.
#include <cmath>

#include "m3g_chunks.h"
#include "m3g_internal.h"
#include "m3g_sampled_row.h"

namespace m3g {
namespace {
constexpr int kTile = kChunkRows;              // atoms per RDF tile == threads per workgroup
constexpr int kLagBlock = 8;                   // lags per workgroup of k_traj_partials (2 kLagBlock columns of 256 doubles in LDS: 32 KB)
constexpr int kMaxSpecies = 8, kMaxBins = 4096, kMaxLags = 4096;
constexpr size_t kHistLds = 48 * 1024;         // the histogram of one structure is privatised in LDS up to this size
enum { kDone = 0, kBegun = 1, kPairs = 2, kCounters = 4 };   // int64 words: frames stored, frames begun, tile pairs in the table

struct TilePair {
  int64_t i0, j0;     // first atoms of tiles I <= J
  int32_t s, first;   // their structure; 1 on the structure's first pair (it does the per-structure work)
};

__host__ __device__ inline int species_pairs(int m) { return m * (m + 1) / 2; }

// tile pairs of a batch, at most (from N and S alone): sum T_s (T_s + 1) / 2 over T_s >= 1 tiles with sum T_s <= chunk_bound is
// largest when one structure holds every spare tile
inline int64_t pair_bound(int64_t N, int64_t S) {
  const int64_t t = chunk_bound(N, S) - S + 1;
  return t * (t + 1) / 2 + (S - 1);
}

struct TrajView {
  int64_t N;
  int32_t M, B, G;
  ChunkView ch;
  const int32_t *species, *nspec;
  const double* mass;
  const TilePair* pairs;
  int64_t* ctr;
  int32_t* flags;
  int64_t* n_samples;
  double* volume;
  unsigned long long* hist;
  double *msd, *vacf;
  int64_t* lag_count;
  double *com, *partial;
  double2* ring;   // [G][3][N]: (x, y), (z, vx), (vy, vz) of atom i at [slot][0..2][i]
};
Carved<TrajView> traj_view(const m3g_traj_sizes& z, void* state) {
  const int64_t N = z.n_atoms, S = z.n_structs, M = z.max_species, B = z.rdf_bins, G = z.n_lags, C = chunk_bound(N, S);
  Carve c{state};
  TrajView st{N, z.max_species, z.rdf_bins, z.n_lags};
  st.ch = chunk_view(N, S, c);
  st.species = c.take<int32_t>(N);
  st.nspec = c.take<int32_t>(S);
  st.mass = c.take<double>(N);
  st.pairs = c.take<TilePair>(B ? pair_bound(N, S) : 0);
  st.ctr = c.take<int64_t>(kCounters);   // the accumulators from here up to `com` are cleared by the init call
  st.flags = c.take<int32_t>(S);
  st.n_samples = c.take<int64_t>(S);
  st.volume = c.take<double>(S);
  st.hist = c.take<unsigned long long>(S * species_pairs((int)M) * B);
  st.msd = c.take<double>(S * M * G);
  st.vacf = c.take<double>(S * M * G);
  st.lag_count = c.take<int64_t>(S * G);
  st.com = c.take<double>(G ? kComPart * C : 0);
  st.partial = c.take<double>(2 * M * G * C);
  st.ring = c.take<double2>(3 * G * N);
  return {st, c.off};
}

template <bool kLds>
__global__ void __launch_bounds__(kTile) k_traj_rdf(TrajView st, double r_max, const double* __restrict__ pos,
                                                   const double* __restrict__ lattice) {
  extern __shared__ unsigned int hist_sh[];   // [P][B] counts of this workgroup (kLds)
  __shared__ double fj[3][kTile];
  __shared__ int32_t sj[kTile];
  const int t = threadIdx.x;
  if ((int64_t)blockIdx.x >= st.ctr[kPairs]) return;
  const TilePair tp = st.pairs[blockIdx.x];
  const int s = tp.s, B = st.B, cells = species_pairs(st.M) * B;
  const int64_t end = st.ch.offsets[s + 1];
  const int ni = (int)(end - tp.i0 < kTile ? end - tp.i0 : kTile), nj = (int)(end - tp.j0 < kTile ? end - tp.j0 : kTile);
  double l[9], c[9];   // rows of l: the lattice vectors a0 a1 a2; rows of c: a1 x a2, a2 x a0, a0 x a1
  for (int k = 0; k < 9; ++k) l[k] = lattice[9 * s + k];
  for (int k = 0; k < 3; ++k) {
    const double* u = l + 3 * ((k + 1) % 3);
    const double* v = l + 3 * ((k + 2) % 3);
    c[3 * k] = u[1] * v[2] - u[2] * v[1];
    c[3 * k + 1] = u[2] * v[0] - u[0] * v[2];
    c[3 * k + 2] = u[0] * v[1] - u[1] * v[0];
  }
  const double det = l[0] * c[0] + l[1] * c[1] + l[2] * c[2];
  if (kLds)
    for (int k = t; k < cells; k += kTile) hist_sh[k] = 0u;
  double fi[3] = {0.0, 0.0, 0.0};
  int si = 0;
  if (t < ni) {   // fractional coordinates: r = f0 a0 + f1 a1 + f2 a2, f_k = r . c_k / det
    const double* r = pos + 3 * (tp.i0 + t);
    for (int k = 0; k < 3; ++k) fi[k] = (r[0] * c[3 * k] + r[1] * c[3 * k + 1] + r[2] * c[3 * k + 2]) / det;
    si = st.species[tp.i0 + t];
  }
  if (t < nj) {
    const double* r = pos + 3 * (tp.j0 + t);
    for (int k = 0; k < 3; ++k) fj[k][t] = (r[0] * c[3 * k] + r[1] * c[3 * k + 1] + r[2] * c[3 * k + 2]) / det;
    sj[t] = st.species[tp.j0 + t];
  }
  __syncthreads();
  if (t < ni) {
    unsigned long long* hist = st.hist + (size_t)s * cells;
    for (int j = (tp.i0 == tp.j0) ? t + 1 : 0; j < nj; ++j) {   // the diagonal tile counts i < j only
      double d[3];
      for (int k = 0; k < 3; ++k) {
        d[k] = fj[k][j] - fi[k];
        d[k] -= rint(d[k]);   // the minimum image of every pair closer than half the smallest perpendicular width
      }
      const double x = d[0] * l[0] + d[1] * l[3] + d[2] * l[6], y = d[0] * l[1] + d[1] * l[4] + d[2] * l[7],
                   z = d[0] * l[2] + d[1] * l[5] + d[2] * l[8];
      const double r = sqrt(x * x + y * y + z * z);
      if (r < r_max) {   // a NaN fails this: a non-finite distance is counted nowhere and never indexes the histogram
        int bin = (int)(r * (double)B / r_max);
        bin = bin < B ? bin : B - 1;   // (r just under r_max can round up to B)
        const int a = si < sj[j] ? si : sj[j], b = si < sj[j] ? sj[j] : si;
        const int cell = (a * st.M - a * (a - 1) / 2 + (b - a)) * B + bin;   // row-major upper triangle
        if (kLds)
          atomicAdd(&hist_sh[cell], 1u);
        else
          atomicAdd(&hist[cell], 1ull);
      }
    }
  }
  if (kLds) {
    __syncthreads();
    unsigned long long* hist = st.hist + (size_t)s * cells;
    for (int k = t; k < cells; k += kTile)
      if (hist_sh[k]) atomicAdd(&hist[k], (unsigned long long)hist_sh[k]);
  }
  if (tp.first && t == 0) {
    double widest = 0.0;   // max |a_j x a_k|
    for (int k = 0; k < 3; ++k) widest = fmax(widest, sqrt(c[3 * k] * c[3 * k] + c[3 * k + 1] * c[3 * k + 1] + c[3 * k + 2] * c[3 * k + 2]));
    st.volume[s] += fabs(det);
    st.n_samples[s] += 1;
    // (1 + 1e-12: the rounding of the width itself, so r_max = a / 2 of a cubic cell passes; a NaN cell sets the flag too)
    if (!(r_max <= 0.5 * (fabs(det) / widest) * (1.0 + 1e-12))) st.flags[s] |= M3G_TRAJ_RDF_RANGE;
  }
}

// (sampled_row and the body of k_traj_com: m3g_sampled_row.h, shared with m3g_scattering.hip)
__global__ void __launch_bounds__(kChunkRows) k_traj_com(TrajView st, const double* __restrict__ pos, const double* __restrict__ vel,
                                                          const float* __restrict__ forces, double kick) {
  com_chunk_partials(st.ch, st.mass, st.com, pos, vel, forces, kick);
}

__global__ void __launch_bounds__(kChunkRows) k_traj_store(TrajView st, int32_t remove_com, const double* __restrict__ pos,
                                                            const double* __restrict__ vel, const float* __restrict__ forces, double kick) {
  const int c = blockIdx.x, t = threadIdx.x;
  if (c >= st.ch.n_chunks()) return;
  const int s = st.ch.structure(c);
  const int64_t done = st.ctr[kDone];
  if (c == 0 && t == 0) st.ctr[kBegun] = done + 1;
  double acc[kComPart];
  if (remove_com) wave_chunk_sum<kComPart>(st.ch, s, st.com, t % kWave, acc);   // (whole waves: every lane ends with the same bits)
  const int64_t i = st.ch.row(c, t);
  if (!st.ch.holds(s, i)) return;
  double r[3], v[3];
  sampled_row(st.mass, i, pos, vel, forces, kick, r, v);
  if (remove_com)
    for (int k = 0; k < 3; ++k) {
      r[k] -= acc[1 + k] / acc[0];
      v[k] -= acc[4 + k] / acc[0];
    }
  double2* slot = st.ring + (size_t)(done % st.G) * 3 * st.N;
  slot[i] = make_double2(r[0], r[1]);
  slot[st.N + i] = make_double2(r[2], v[0]);
  slot[2 * st.N + i] = make_double2(v[1], v[2]);
}

__global__ void __launch_bounds__(kChunkRows) k_traj_partials(TrajView st) {
  __shared__ double sh[2 * kLagBlock][kChunkRows];
  const int c = blockIdx.x, t = threadIdx.x;
  if (c >= st.ch.n_chunks()) return;
  const int64_t done = st.ctr[kDone];
  const int G = st.G, top = (int)(done < G - 1 ? done : G - 1);   // the longest stored lag
  const int lag0 = blockIdx.y * kLagBlock;
  if (lag0 > top) return;
  const int s = st.ch.structure(c), now = (int)(done % G);
  const int64_t i = st.ch.row(c, t), N = st.N;
  const bool mine = st.ch.holds(s, i);
  double dr2[kLagBlock], vv[kLagBlock];
  for (int k = 0; k < kLagBlock; ++k) dr2[k] = vv[k] = 0.0;
  int sp = -1;
  if (mine) {
    sp = st.species[i];
    const double2* cur = st.ring + (size_t)now * 3 * N;
    const double2 a0 = cur[i], a1 = cur[N + i], a2 = cur[2 * N + i];
#pragma unroll
    for (int k = 0; k < kLagBlock; ++k) {
      if (lag0 + k <= top) {
        const double2* old = st.ring + (size_t)((now - lag0 - k + G) % G) * 3 * N;
        const double2 b0 = old[i], b1 = old[N + i], b2 = old[2 * N + i];
        const double dx = a0.x - b0.x, dy = a0.y - b0.y, dz = a1.x - b1.x;
        dr2[k] = dx * dx + dy * dy + dz * dz;
        vv[k] = a1.y * b1.y + a2.x * b2.x + a2.y * b2.y;
      }
    }
  }
  const int ns = st.nspec[s];
  for (int a = 0; a < ns; ++a) {
    double val[2 * kLagBlock];
#pragma unroll
    for (int k = 0; k < kLagBlock; ++k) {
      val[2 * k] = sp == a ? dr2[k] : 0.0;
      val[2 * k + 1] = sp == a ? vv[k] : 0.0;
    }
    chunk_tree_reduce<2 * kLagBlock>(sh, val, t);
    if (t < 2 * kLagBlock && lag0 + t / 2 <= top) st.partial[(((size_t)c * G + lag0 + t / 2) * st.M + a) * 2 + t % 2] = sh[t][0];
    __syncthreads();   // (sh is written again by the next species)
  }
}

__global__ void __launch_bounds__(kChunkRows) k_traj_finalize(TrajView st, int32_t count_samples) {
  const int64_t idx = (int64_t)blockIdx.x * kChunkRows + threadIdx.x;
  const int64_t begun = st.ctr[kBegun];
  if (idx == 0) st.ctr[kDone] = begun;
  const int G = st.G, M = st.M;
  if (idx >= st.ch.S * G * M) return;
  const int a = (int)(idx % M), lag = (int)(idx / M % G);
  const int64_t s = idx / M / G;
  if (count_samples && a == 0 && lag == 0) st.n_samples[s] += 1;
  if (lag >= begun || a >= st.nspec[s]) return;   // begun <= G: lags 0 .. begun - 1 are stored; beyond: all G
  double m = 0.0, v = 0.0;
  for (int c = st.ch.chunks_begin(s); c < st.ch.chunks_end(s); ++c) {   // chunk order
    const double* p = st.partial + (((size_t)c * G + lag) * M + a) * 2;
    m += p[0];
    v += p[1];
  }
  st.msd[(s * M + a) * G + lag] += m;
  st.vacf[(s * M + a) * G + lag] += v;
  if (a == 0) st.lag_count[s * G + lag] += 1;
}

// nullptr when sizes and parameters are valid, else what is wrong with them
const char* traj_error(const m3g_traj_sizes* z, const m3g_traj_params* p) {
  if (!z || !p) return "null sizes or parameters";
  if (!batch_sizes_ok(z->n_atoms, z->n_structs)) return "bad sizes";
  if (z->max_species < 1 || z->max_species > kMaxSpecies) return "max_species must be 1 .. 8";
  if (z->rdf_bins < 0 || z->rdf_bins > kMaxBins) return "rdf_bins must be 0 .. 4096";
  if (z->n_lags < 0 || z->n_lags > kMaxLags) return "n_lags must be 0 .. 4096";
  if (z->rdf_bins == 0 && z->n_lags == 0) return "rdf_bins and n_lags are both 0: nothing to accumulate";
  if (z->rdf_bins > 0 && pair_bound(z->n_atoms, z->n_structs) > INT32_MAX) return "too many tile pairs for one launch";
  if (z->rdf_bins > 0 && !finite_positive(p->r_max)) return "r_max must be finite and > 0";
  if (p->remove_com != 0 && p->remove_com != 1) return "remove_com must be 0 or 1";
  return nullptr;
}
const m3g_traj_params kNoRdf = {1.0, 0};   // stands in where a call needs the sizes checked only
}  // namespace
}  // namespace m3g

using namespace m3g;

extern "C" int m3g_traj_state_bytes(const m3g_traj_sizes* sizes, size_t* bytes) {
  const m3g_traj_params* any = &kNoRdf;
  if (const char* why = traj_error(sizes, any)) { set_error("m3g_traj_state_bytes: %s", why); return M3G_ERR_VALUE; }
  if (!bytes) { set_error("m3g_traj_state_bytes: null argument"); return M3G_ERR_VALUE; }
  *bytes = traj_view(*sizes, nullptr).bytes;
  return M3G_OK;
}

extern "C" int m3g_traj_init(const m3g_traj_sizes* sizes, const m3g_traj_params* params, const int64_t* host_offsets, const int32_t* host_species,
                             const double* host_masses, void* state, size_t state_bytes, void* stream_) {
  if (const char* why = traj_error(sizes, params)) { set_error("m3g_traj_init: %s", why); return M3G_ERR_VALUE; }
  if (!host_offsets || !host_species || !host_masses || !state) { set_error("m3g_traj_init: null argument"); return M3G_ERR_VALUE; }
  const int64_t N = sizes->n_atoms, S = sizes->n_structs;
  if (!offsets_ok("m3g_traj_init", host_offsets, N, S)) return M3G_ERR_VALUE;
  std::vector<int32_t> nspec(S, 0);
  for (int64_t s = 0; s < S; ++s)
    for (int64_t i = host_offsets[s]; i < host_offsets[s + 1]; ++i) {
      if (host_species[i] < 0 || host_species[i] >= sizes->max_species) {
        set_error("m3g_traj_init: species index of atom %lld is outside 0 .. max_species - 1", (long long)i);
        return M3G_ERR_VALUE;
      }
      if (!mass_ok("m3g_traj_init", host_masses, i)) return M3G_ERR_VALUE;
      if (host_species[i] >= nspec[s]) nspec[s] = host_species[i] + 1;
    }
  const auto [st, total] = traj_view(*sizes, state);
  if (!state_fits("m3g_traj_init", state_bytes, total, true)) return M3G_ERR_SIZE;
  std::vector<TilePair> pairs;
  if (sizes->rdf_bins > 0)
    for (int64_t s = 0; s < S; ++s)
      for (int64_t i0 = host_offsets[s]; i0 < host_offsets[s + 1]; i0 += kTile)
        for (int64_t j0 = i0; j0 < host_offsets[s + 1]; j0 += kTile)
          pairs.push_back(TilePair{i0, j0, (int32_t)s, i0 == host_offsets[s] && j0 == i0 ? 1 : 0});
  const int64_t ctr[kCounters] = {0, 0, (int64_t)pairs.size(), 0};
  const ChunkTable table(host_offsets, S);
  hipStream_t s = (hipStream_t)stream_;
  if (int rc = table.upload(st.ch, host_offsets, s)) return rc;
  M3G_HIP_CHECK(hipMemcpyAsync((void*)st.species, host_species, 4 * N, hipMemcpyHostToDevice, s));
  M3G_HIP_CHECK(hipMemcpyAsync((void*)st.nspec, nspec.data(), 4 * S, hipMemcpyHostToDevice, s));
  M3G_HIP_CHECK(hipMemcpyAsync((void*)st.mass, host_masses, 8 * N, hipMemcpyHostToDevice, s));
  if (!pairs.empty()) M3G_HIP_CHECK(hipMemcpyAsync((void*)st.pairs, pairs.data(), sizeof(TilePair) * pairs.size(), hipMemcpyHostToDevice, s));
  M3G_HIP_CHECK(hipMemsetAsync(st.ctr, 0, (size_t)((const char*)st.com - (const char*)st.ctr), s));
  M3G_HIP_CHECK(hipMemcpyAsync(st.ctr, ctr, sizeof(ctr), hipMemcpyHostToDevice, s));
  M3G_HIP_CHECK(hipStreamSynchronize(s));   // (the host tables above go out of scope)
  return M3G_OK;
}

extern "C" int m3g_traj_sample(const m3g_traj_sizes* sizes, const m3g_traj_params* params, void* state, size_t state_bytes, const double* pos,
                               const double* lattice, const double* vel, const float* forces, double kick, void* stream_) {
  if (const char* why = traj_error(sizes, params)) { set_error("m3g_traj_sample: %s", why); return M3G_ERR_VALUE; }
  const bool rdf = sizes->rdf_bins > 0, lags = sizes->n_lags > 0;
  if (!state || !pos || (rdf && !lattice) || (lags && !vel)) { set_error("m3g_traj_sample: null argument"); return M3G_ERR_VALUE; }
  if (forces && !std::isfinite(kick)) { set_error("m3g_traj_sample: kick must be finite"); return M3G_ERR_VALUE; }
  const auto [st, total] = traj_view(*sizes, state);
  if (!state_fits("m3g_traj_sample", state_bytes, total)) return M3G_ERR_SIZE;
  const int64_t N = sizes->n_atoms, S = sizes->n_structs;
  hipStream_t s = (hipStream_t)stream_;
  if (rdf) {   // workgroups beyond the table's pair count return at once
    const dim3 grid((unsigned)pair_bound(N, S));
    const size_t lds = sizeof(unsigned int) * species_pairs(sizes->max_species) * sizes->rdf_bins;
    if (lds <= kHistLds)
      hipLaunchKernelGGL(k_traj_rdf<true>, grid, dim3(kTile), lds, s, st, params->r_max, pos, lattice);
    else
      hipLaunchKernelGGL(k_traj_rdf<false>, grid, dim3(kTile), 0, s, st, params->r_max, pos, lattice);
  }
  if (lags) {
    const dim3 grid((unsigned)chunk_bound(N, S));   // workgroups beyond the table's chunk count return at once
    if (params->remove_com) hipLaunchKernelGGL(k_traj_com, grid, dim3(kChunkRows), 0, s, st, pos, vel, forces, kick);
    hipLaunchKernelGGL(k_traj_store, grid, dim3(kChunkRows), 0, s, st, params->remove_com, pos, vel, forces, kick);
    hipLaunchKernelGGL(k_traj_partials, dim3(grid.x, (unsigned)((sizes->n_lags + kLagBlock - 1) / kLagBlock)), dim3(kChunkRows), 0, s, st);
    hipLaunchKernelGGL(k_traj_finalize, grid_for(S * sizes->n_lags * sizes->max_species, kChunkRows), dim3(kChunkRows), 0, s, st,
                       rdf ? 0 : 1);
  }
  M3G_RETURN_LAUNCH_STATUS();
}

extern "C" int m3g_traj_read(const m3g_traj_sizes* sizes, const void* state, size_t state_bytes, uint64_t* host_hist, double* host_msd,
                             double* host_vacf, int64_t* host_lag_count, int64_t* host_n_samples, double* host_volume_sum, int32_t* host_flags,
                             void* stream_) {
  if (const char* why = traj_error(sizes, &kNoRdf)) { set_error("m3g_traj_read: %s", why); return M3G_ERR_VALUE; }
  if (!state) { set_error("m3g_traj_read: null argument"); return M3G_ERR_VALUE; }
  const auto [st, total] = traj_view(*sizes, (void*)state);
  if (!state_fits("m3g_traj_read", state_bytes, total)) return M3G_ERR_SIZE;
  const size_t S = sizes->n_structs, M = sizes->max_species, B = sizes->rdf_bins, G = sizes->n_lags;
  return read_all((hipStream_t)stream_,
                  {rb((unsigned long long*)host_hist, st.hist, S * species_pairs((int)M) * B), rb(host_msd, st.msd, S * M * G),
                   rb(host_vacf, st.vacf, S * M * G), rb(host_lag_count, st.lag_count, S * G), rb(host_n_samples, st.n_samples, S),
                   rb(host_volume_sum, st.volume, S), rb(host_flags, st.flags, S)});
}

extern "C" int m3g_traj_frame(const m3g_traj_sizes* sizes, const void* state, size_t state_bytes, int32_t lag, double* host_pos, double* host_vel,
                              void* stream_) {
  if (const char* why = traj_error(sizes, &kNoRdf)) { set_error("m3g_traj_frame: %s", why); return M3G_ERR_VALUE; }
  if (!state || !host_pos || !host_vel || sizes->n_lags == 0) { set_error("m3g_traj_frame: null argument or no ring (n_lags == 0)"); return M3G_ERR_VALUE; }
  const auto [st, total] = traj_view(*sizes, (void*)state);
  if (!state_fits("m3g_traj_frame", state_bytes, total)) return M3G_ERR_SIZE;
  const int64_t N = sizes->n_atoms, G = sizes->n_lags;
  hipStream_t s = (hipStream_t)stream_;
  int64_t ctr[kCounters];
  M3G_HIP_CHECK(hipMemcpyAsync(ctr, st.ctr, sizeof(ctr), hipMemcpyDeviceToHost, s));
  M3G_HIP_CHECK(hipStreamSynchronize(s));
  if (lag < 0 || lag >= G || lag >= ctr[kDone]) { set_error("m3g_traj_frame: no frame %d samples back", (int)lag); return M3G_ERR_VALUE; }
  std::vector<double2> slot(3 * N);
  M3G_HIP_CHECK(hipMemcpyAsync(slot.data(), st.ring + 3 * N * ((ctr[kDone] - 1 - lag) % G), 48 * N, hipMemcpyDeviceToHost, s));
  M3G_HIP_CHECK(hipStreamSynchronize(s));
  for (int64_t i = 0; i < N; ++i) {
    host_pos[3 * i] = slot[i].x; host_pos[3 * i + 1] = slot[i].y; host_pos[3 * i + 2] = slot[N + i].x;
    host_vel[3 * i] = slot[N + i].y; host_vel[3 * i + 1] = slot[2 * N + i].x; host_vel[3 * i + 2] = slot[2 * N + i].y;
  }
  return M3G_OK;
}
