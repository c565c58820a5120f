// Scattering observables of a batch, accumulated on the device while it is integrated (or fed any frames): per structure and q-vector
// the species-resolved density rho_a(q) = sum_j exp(-i q . r_j) and current j_a(q) = sum_j v_j exp(-i q . r_j), and over a ring of the
// last n_lags samples the sums behind F(q,t), C_L(q,t) and C_T(q,t) per species pair (conventions: include/m3gnet_hip.h).  Unlike
// m3g_nma.hip, whose phases are tabulated once from equilibrium sites, the phases here come from the current positions: N Q complex
// exponentials per sample.  One m3g_sq_sample is, over the chunk table of m3g_chunks.h:
//   k_sq_com        (remove_com) one workgroup per chunk: partial sums of m, m r, m v in a fixed tree order (the body of k_traj_com);
//   k_sq_density    grid (chunk, tile of kQTile q-vectors): the chunk's <= 256 rows are staged in LDS as REDUCED fractional
//                   coordinates f - rint(f), completed velocities (centre of mass removed) and species; lane l of each of the four
//                   waves owns q-vector l of the tile, and wave w walks rows 64 w .. 64 w + 63 in row order -- every LDS read is one
//                   address for the whole wave, a broadcast -- reducing h . f again before sincospi, with rho and j per species
//                   in registers (8 M doubles); the four segments are added in segment order through LDS: one partial per
//                   (chunk, q, species);
//   k_sq_store      one thread per (q, species): the chunk partials in chunk order, projected on qhat of the CURRENT cell, into the ring
//                   slot of this sample; one thread per structure judges the cell, sets the flags and counts the sample;
//   k_sq_correlate  grid (q, block of kLagBlock lags): the current slot's entries of q against the slot `lag` samples back; one thread
//                   owns the accumulator elements (q, every pair, lag).  Workgroups past the last q advance lag_count, one thread per
//                   (structure, lag).
// No float atomics: every number depends on the structure's own rows only, so it is bitwise the same alone or in any batch.  The
// ring position lives in the state buffer (the two counters of m3g_trajectory.hip: every kernel reads one and at most one thread
// writes the other), hence no allocation, copy or wait in m3g_sq_sample: capture-safe.
#include <cmath>
#include <type_traits>

#include "m3g_chunks.h"
#include "m3g_internal.h"
#include "m3g_sampled_row.h"

namespace m3g {
namespace {
constexpr int kQTile = 64;        // q-vectors per workgroup of k_sq_density: one per lane of a wave
// its waves: each walks a quarter of the chunk's rows (one wave alone is bound by the latency of 256 sincospi calls one after the
// other: profiles/scattering.txt)
constexpr int kSegments = 4, kSegRows = kChunkRows / kSegments;
static_assert(kQTile == kWave && kQTile * kSegments == kChunkRows, "k_sq_density: one row per thread when staging, one q per lane");
constexpr int kLagBlock = 64;     // lags per workgroup of k_sq_correlate == its threads
constexpr int kEntry = 10;        // ring entry per (q, species): rho (re, im), j_L (re, im), j_T [3] (re, im)
constexpr int kPartial = 8;       // chunk partial per (q, species): rho (re, im), j [3] (re, im)
constexpr int kMaxSpecies = M3G_SQ_MAX_SPECIES, kMaxLags = M3G_SQ_MAX_LAGS, kMaxQ = M3G_SQ_MAX_Q, kMaxIndex = M3G_SQ_MAX_INDEX;
constexpr double kMinDet = 1e-12;   // a cell below it is singular to lattice_ok (m3g_chunks.h) as well
enum { kDone = 0, kBegun = 1, kCounters = 4 };   // int64 words: samples stored, samples begun

__host__ __device__ inline int species_pairs(int m) { return m * (m + 1) / 2; }
inline int64_t q_cap(int64_t n_q) { return n_q < kMaxQ ? n_q : kMaxQ; }   // q-vectors of one structure, at most

struct SqView {
  int64_t N, Q, cap;   // atoms, q-vectors in all, the q stride of `partial`
  int32_t M, G;
  ChunkView ch;
  const int32_t *species, *nspec;
  const double* mass;
  const int64_t* q_offsets;   // [S+1]
  const int32_t* hkl;         // [Q][3]
  const int32_t* q_struct;    // [Q]
  int64_t* ctr;
  int32_t* flags;
  int64_t* n_samples;
  int64_t* lag_count;         // [S][G]
  double *f, *cl, *ct;        // [Q][P][G]
  int32_t* slot_ok;           // [S][G]: the cell of the sample in that ring slot was invertible
  double *com, *partial;      // [C][kComPart]; [C][cap][M][kPartial]
  double* ring;               // [G][Q][M][kEntry]
};
Carved<SqView> sq_view(const m3g_sq_sizes& z, void* state) {
  const int64_t N = z.n_atoms, S = z.n_structs, Q = z.n_q, M = z.max_species, G = z.n_lags, C = chunk_bound(N, S);
  const int64_t P = species_pairs((int)M);
  Carve c{state};
  SqView st{N, Q, q_cap(Q), z.max_species, z.n_lags};
  st.ch = chunk_view(N, S, c);
  st.species = c.take<int32_t>(N);
  st.nspec = c.take<int32_t>(S);
  st.mass = c.take<double>(N);
  st.q_offsets = c.take<int64_t>(S + 1);
  st.hkl = c.take<int32_t>(3 * Q);
  st.q_struct = c.take<int32_t>(Q);
  st.ctr = c.take<int64_t>(kCounters);   // the accumulators from here up to `slot_ok` are cleared by the init call
  st.flags = c.take<int32_t>(S);
  st.n_samples = c.take<int64_t>(S);
  st.lag_count = c.take<int64_t>(S * G);
  st.f = c.take<double>(Q * P * G);
  st.cl = c.take<double>(Q * P * G);
  st.ct = c.take<double>(Q * P * G);
  st.slot_ok = c.take<int32_t>(S * G);
  st.com = c.take<double>(kComPart * C);
  st.partial = c.take<double>(C * st.cap * M * kPartial);
  st.ring = c.take<double>(G * Q * M * kEntry);
  return {st, c.off};
}

// rows of c: a1 x a2, a2 x a0, a0 x a1 of the cell l (rows = lattice vectors); returns det = a0 . (a1 x a2)
__device__ inline double cofactors(const double* __restrict__ lattice, double (&c)[9]) {
  double l[9];
  for (int k = 0; k < 9; ++k) l[k] = lattice[k];
  for (int k = 0; k < 3; ++k) {
    const double* u = l + 3 * ((k + 1) % 3);
    const double* v = l + 3 * ((k + 2) % 3);
    c[3 * k] = u[1] * v[2] - u[2] * v[1];
    c[3 * k + 1] = u[2] * v[0] - u[0] * v[2];
    c[3 * k + 2] = u[0] * v[1] - u[1] * v[0];
  }
  return l[0] * c[0] + l[1] * c[1] + l[2] * c[2];
}

__global__ void __launch_bounds__(kChunkRows) k_sq_com(SqView st, const double* __restrict__ pos, const double* __restrict__ vel,
                                                        const float* __restrict__ forces, double kick) {
  com_chunk_partials(st.ch, st.mass, st.com, pos, vel, forces, kick);
}

template <int M>
__global__ void __launch_bounds__(kChunkRows) k_sq_density(SqView st, int32_t remove_com, const double* __restrict__ pos,
                                                            const double* __restrict__ lattice, const double* __restrict__ vel,
                                                            const float* __restrict__ forces, double kick) {
  __shared__ double row_sh[6][kChunkRows];   // reduced fractional coordinates [3], velocity [3]
  __shared__ int32_t species_sh[kChunkRows];
  __shared__ double part_sh[M * kPartial][kQTile];   // the sums of one later segment on their way to the first
  const int c = blockIdx.x, t = threadIdx.x;
  if (c >= st.ch.n_chunks()) return;
  const int s = st.ch.structure(c);
  const int64_t q_lo = st.q_offsets[s];
  const int n_q = (int)(st.q_offsets[s + 1] - q_lo), q0 = blockIdx.y * kQTile;
  if (q0 >= n_q) return;
  double cof[9];
  const double det = cofactors(lattice + 9 * s, cof);
  {
    double acc[kComPart];
    if (remove_com) wave_chunk_sum<kComPart>(st.ch, s, st.com, t % kWave, acc);   // (whole waves: every lane ends with the same bits)
    const int64_t i = st.ch.row(c, t);
    int sp = -1;   // (a part-filled chunk: rows beyond the structure belong to no species)
    if (st.ch.holds(s, i)) {
      double r[3], v[3];
      sampled_row(st.mass, i, pos, vel, forces, kick, r, v);
      if (remove_com)
        for (int k = 0; k < 3; ++k) {
          r[k] -= acc[1 + k] / acc[0];
          v[k] -= acc[4 + k] / acc[0];
        }
      for (int k = 0; k < 3; ++k) {   // r = f0 a0 + f1 a1 + f2 a2, f_k = r . c_k / det; only f modulo 1 enters a phase
        const double f = (r[0] * cof[3 * k] + r[1] * cof[3 * k + 1] + r[2] * cof[3 * k + 2]) / det;
        row_sh[k][t] = f - rint(f);
        row_sh[3 + k][t] = v[k];
      }
      sp = st.species[i];
    }
    species_sh[t] = sp;
  }
  __syncthreads();
  const int seg = t / kQTile, ql = t % kQTile;   // wave `seg` walks rows seg kSegRows .. of the chunk for the tile's q-vectors
  const bool mine = q0 + ql < n_q;
  const int32_t* h = st.hkl + 3 * (q_lo + (mine ? q0 + ql : 0));
  const double h0 = (double)h[0], h1 = (double)h[1], h2 = (double)h[2];
  double sum[M][kPartial];
  for (int a = 0; a < M; ++a)
    for (int k = 0; k < kPartial; ++k) sum[a][k] = 0.0;
  const int64_t end = st.ch.offsets[s + 1] - st.ch.row(c, 0);
  const int rows = (int)(end < kChunkRows ? end : kChunkRows);
  const int last = rows < (seg + 1) * kSegRows ? rows : (seg + 1) * kSegRows;
  for (int j = seg * kSegRows; j < last; ++j) {   // row order; every LDS address is the same for the whole wave
    double p = h0 * row_sh[0][j] + h1 * row_sh[1][j] + h2 * row_sh[2][j];   // |p| <= 1.5 kMaxIndex
    p -= rint(p);
    double sn, cs;
    sincospi(2.0 * p, &sn, &cs);   // exp(-i 2 pi p) = cs - i sn, the argument in [-1, 1]
    const double vx = row_sh[3][j], vy = row_sh[4][j], vz = row_sh[5][j];
    const int sp = species_sh[j];
#pragma unroll
    for (int a = 0; a < M; ++a)
      if (sp == a) {   // (uniform over the wave)
        sum[a][0] += cs;
        sum[a][1] -= sn;
        sum[a][2] += vx * cs;
        sum[a][3] -= vx * sn;
        sum[a][4] += vy * cs;
        sum[a][5] -= vy * sn;
        sum[a][6] += vz * cs;
        sum[a][7] -= vz * sn;
      }
  }
  for (int other = 1; other < kSegments; ++other) {   // ((segment 0 + 1) + 2) + 3: a fixed order
    if (seg == other) {
#pragma unroll
      for (int a = 0; a < M; ++a)
        for (int k = 0; k < kPartial; ++k) part_sh[a * kPartial + k][ql] = sum[a][k];
    }
    __syncthreads();
    if (seg == 0) {
#pragma unroll
      for (int a = 0; a < M; ++a)
        for (int k = 0; k < kPartial; ++k) sum[a][k] += part_sh[a * kPartial + k][ql];
    }
    __syncthreads();
  }
  if (seg != 0 || !mine) return;
  double* out = st.partial + (((size_t)c * st.cap + q0 + ql) * M) * kPartial;
#pragma unroll
  for (int a = 0; a < M; ++a)
    for (int k = 0; k < kPartial; ++k) out[a * kPartial + k] = sum[a][k];
}

__global__ void __launch_bounds__(kChunkRows) k_sq_store(SqView st, const double* __restrict__ lattice) {
  const int64_t idx = (int64_t)blockIdx.x * kChunkRows + threadIdx.x;
  const int64_t done = st.ctr[kDone];
  if (idx == 0) st.ctr[kBegun] = done + 1;
  const int M = st.M, G = st.G, slot = (int)(done % G);
  if (idx < st.ch.S) {   // the structure's part: is the cell of this sample invertible?
    double cof[9];
    const double det = cofactors(lattice + 9 * idx, cof);
    const bool ok = isfinite(det) && fabs(det) >= kMinDet;
    st.slot_ok[idx * G + slot] = ok ? 1 : 0;
    if (ok) st.n_samples[idx] += 1;
    else st.flags[idx] |= M3G_SQ_CELL;
  }
  if (idx >= st.Q * M) return;
  const int a = (int)(idx % M);
  const int64_t q = idx / M;
  const int s = st.q_struct[q];
  const int64_t ql = q - st.q_offsets[s];
  double sum[kPartial] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int c = st.ch.chunks_begin(s); c < st.ch.chunks_end(s); ++c) {   // chunk order
    const double* p = st.partial + (((size_t)c * st.cap + ql) * M + a) * kPartial;
    for (int k = 0; k < kPartial; ++k) sum[k] += p[k];
  }
  double cof[9];
  const double det = cofactors(lattice + 9 * s, cof);
  const int32_t* h = st.hkl + 3 * q;
  double u[3];   // q / 2 pi = (h0 c0 + h1 c1 + h2 c2) / det
  for (int k = 0; k < 3; ++k) u[k] = ((double)h[0] * cof[k] + (double)h[1] * cof[3 + k] + (double)h[2] * cof[6 + k]) / det;
  const double norm = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
  for (int k = 0; k < 3; ++k) u[k] /= norm;
  double* e = st.ring + (((size_t)slot * st.Q + q) * M + a) * kEntry;
  e[0] = sum[0];
  e[1] = sum[1];
  for (int part = 0; part < 2; ++part) {   // real and imaginary parts: qhat is real
    const double jx = sum[2 + part], jy = sum[4 + part], jz = sum[6 + part];
    const double jl = u[0] * jx + u[1] * jy + u[2] * jz;
    e[2 + part] = jl;
    e[4 + part] = jx - u[0] * jl;
    e[6 + part] = jy - u[1] * jl;
    e[8 + part] = jz - u[2] * jl;
  }
}

template <int M>
__global__ void __launch_bounds__(kLagBlock) k_sq_correlate(SqView st) {
  constexpr int P = M * (M + 1) / 2;
  const int64_t begun = st.ctr[kBegun], done = begun - 1;
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) st.ctr[kDone] = begun;
  const int G = st.G, lag = blockIdx.y * kLagBlock + threadIdx.x;
  const int top = (int)(done < G - 1 ? done : G - 1);   // the longest stored lag
  if (lag > top) return;
  const int now = (int)(done % G), then = (now - lag + G) % G;
  if ((int64_t)blockIdx.x >= st.Q) {   // the workgroups past the last q: lag_count, one thread per (structure, lag)
    const int64_t s = (int64_t)blockIdx.x - st.Q;
    if (st.slot_ok[s * G + now] && st.slot_ok[s * G + then]) st.lag_count[s * G + lag] += 1;
    return;
  }
  const int64_t q = blockIdx.x;
  const int64_t s = st.q_struct[q];
  if (!st.slot_ok[s * G + now] || !st.slot_ok[s * G + then]) return;
  const double* cur = st.ring + ((size_t)now * st.Q + q) * M * kEntry;    // (one address for the whole workgroup)
  const double* old = st.ring + ((size_t)then * st.Q + q) * M * kEntry;
  double x[M][kEntry], y[M][kEntry];
#pragma unroll
  for (int a = 0; a < M; ++a)
    for (int k = 0; k < kEntry; ++k) {
      x[a][k] = cur[a * kEntry + k];
      y[a][k] = old[a * kEntry + k];
    }
  int pair = 0;
#pragma unroll
  for (int a = 0; a < M; ++a)
#pragma unroll
    for (int b = a; b < M; ++b, ++pair) {   // row-major upper triangle
      // Re[x_a y_b* + x_b y_a*] / 2 of every component
      double term[kEntry / 2];
      for (int k = 0; k < kEntry / 2; ++k)
        term[k] = 0.5 * ((x[a][2 * k] * y[b][2 * k] + x[a][2 * k + 1] * y[b][2 * k + 1]) +
                         (x[b][2 * k] * y[a][2 * k] + x[b][2 * k + 1] * y[a][2 * k + 1]));
      const size_t at = ((size_t)q * P + pair) * G + lag;
      st.f[at] += term[0];
      st.cl[at] += term[1];
      st.ct[at] += 0.5 * (term[2] + term[3] + term[4]);
    }
}

// nullptr when sizes and parameters are valid, else what is wrong with them
const char* sq_error(const m3g_sq_sizes* z, const m3g_sq_params* p) {
  if (!z || !p) return "null sizes or parameters";
  if (!batch32_sizes_ok(z->n_atoms, z->n_structs)) return "bad sizes";
  if (z->n_q < 1 || z->n_q > z->n_structs * (int64_t)kMaxQ || z->n_q > INT32_MAX / kChunkRows) return "n_q must be 1 .. 4096 n_structs";
  if (z->max_species < 1 || z->max_species > kMaxSpecies) return "max_species must be 1 .. 4";
  if (z->n_lags < 1 || z->n_lags > kMaxLags) return "n_lags must be 1 .. 4096";
  if (p->remove_com != 0 && p->remove_com != 1) return "remove_com must be 0 or 1";
  return nullptr;
}
const m3g_sq_params kAnyParams = {0, 0};   // stands in where a call needs the sizes checked only

template <class F>
void dispatch_species(int m, F&& f) {   // compile-time species count of the register arrays
  switch (m) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    default: f(std::integral_constant<int, 4>{}); break;
  }
}
}  // namespace
}  // namespace m3g

using namespace m3g;

extern "C" int m3g_sq_state_bytes(const m3g_sq_sizes* sizes, size_t* bytes) {
  if (const char* why = sq_error(sizes, &kAnyParams)) { set_error("m3g_sq_state_bytes: %s", why); return M3G_ERR_VALUE; }
  if (!bytes) { set_error("m3g_sq_state_bytes: null argument"); return M3G_ERR_VALUE; }
  *bytes = sq_view(*sizes, nullptr).bytes;
  return M3G_OK;
}

extern "C" int m3g_sq_init(const m3g_sq_sizes* sizes, const m3g_sq_params* params, const int64_t* host_offsets, const int32_t* host_species,
                           const double* host_masses, const int64_t* host_q_offsets, const int32_t* host_hkl, void* state, size_t state_bytes,
                           void* stream_) {
  if (const char* why = sq_error(sizes, params)) { set_error("m3g_sq_init: %s", why); return M3G_ERR_VALUE; }
  if (!host_offsets || !host_species || !host_masses || !host_q_offsets || !host_hkl || !state) {
    set_error("m3g_sq_init: null argument");
    return M3G_ERR_VALUE;
  }
  const int64_t N = sizes->n_atoms, S = sizes->n_structs, Q = sizes->n_q;
  if (!offsets_ok("m3g_sq_init", host_offsets, N, S)) return M3G_ERR_VALUE;
  std::vector<int32_t> nspec(S, 0), q_struct(Q);
  for (int64_t s = 0; s < S; ++s)
    for (int64_t i = host_offsets[s]; i < host_offsets[s + 1]; ++i) {
      if (host_species[i] < 0 || host_species[i] >= sizes->max_species) {
        set_error("m3g_sq_init: species index of atom %lld is outside 0 .. max_species - 1", (long long)i);
        return M3G_ERR_VALUE;
      }
      if (!mass_ok("m3g_sq_init", host_masses, i)) return M3G_ERR_VALUE;
      if (host_species[i] >= nspec[s]) nspec[s] = host_species[i] + 1;
    }
  if (host_q_offsets[0] != 0 || host_q_offsets[S] != Q) { set_error("m3g_sq_init: q offsets must run from 0 to n_q"); return M3G_ERR_VALUE; }
  for (int64_t s = 0; s < S; ++s) {
    const int64_t n = host_q_offsets[s + 1] - host_q_offsets[s];
    if (n < 0) { set_error("m3g_sq_init: q offsets must not decrease"); return M3G_ERR_VALUE; }
    if (n > kMaxQ) { set_error("m3g_sq_init: structure %lld has more than %d q-vectors", (long long)s, kMaxQ); return M3G_ERR_VALUE; }
  }
  for (int64_t s = 0; s < S; ++s)   // (the offsets are now known to stay inside [0, n_q])
    for (int64_t q = host_q_offsets[s]; q < host_q_offsets[s + 1]; ++q) {
      const int32_t* h = host_hkl + 3 * q;
      if (h[0] == 0 && h[1] == 0 && h[2] == 0) { set_error("m3g_sq_init: q-vector %lld is h = 0", (long long)q); return M3G_ERR_VALUE; }
      for (int k = 0; k < 3; ++k)
        if (h[k] > kMaxIndex || h[k] < -kMaxIndex) {
          set_error("m3g_sq_init: q-vector %lld has an index beyond +-%d", (long long)q, kMaxIndex);
          return M3G_ERR_VALUE;
        }
      q_struct[q] = (int32_t)s;
    }
  const auto [st, total] = sq_view(*sizes, state);
  if (!state_fits("m3g_sq_init", state_bytes, total, true)) return M3G_ERR_SIZE;
  const ChunkTable table(host_offsets, S);
  hipStream_t s = (hipStream_t)stream_;
  if (int rc = table.upload(st.ch, host_offsets, s)) return rc;
  M3G_HIP_CHECK(hipMemcpyAsync((void*)st.species, host_species, 4 * N, hipMemcpyHostToDevice, s));
  M3G_HIP_CHECK(hipMemcpyAsync((void*)st.nspec, nspec.data(), 4 * S, hipMemcpyHostToDevice, s));
  M3G_HIP_CHECK(hipMemcpyAsync((void*)st.mass, host_masses, 8 * N, hipMemcpyHostToDevice, s));
  M3G_HIP_CHECK(hipMemcpyAsync((void*)st.q_offsets, host_q_offsets, 8 * (S + 1), hipMemcpyHostToDevice, s));
  M3G_HIP_CHECK(hipMemcpyAsync((void*)st.hkl, host_hkl, 12 * Q, hipMemcpyHostToDevice, s));
  M3G_HIP_CHECK(hipMemcpyAsync((void*)st.q_struct, q_struct.data(), 4 * Q, hipMemcpyHostToDevice, s));
  M3G_HIP_CHECK(hipMemsetAsync(st.ctr, 0, (size_t)((const char*)st.slot_ok - (const char*)st.ctr), s));
  M3G_HIP_CHECK(hipStreamSynchronize(s));   // (the host tables above go out of scope)
  return M3G_OK;
}

extern "C" int m3g_sq_sample(const m3g_sq_sizes* sizes, const m3g_sq_params* params, void* state, size_t state_bytes, const double* pos,
                             const double* lattice, const double* vel, const float* forces, double kick, void* stream_) {
  if (const char* why = sq_error(sizes, params)) { set_error("m3g_sq_sample: %s", why); return M3G_ERR_VALUE; }
  if (!state || !pos || !lattice || !vel) { set_error("m3g_sq_sample: null argument"); return M3G_ERR_VALUE; }
  if (forces && !std::isfinite(kick)) { set_error("m3g_sq_sample: kick must be finite"); return M3G_ERR_VALUE; }
  const auto [st, total] = sq_view(*sizes, state);
  if (!state_fits("m3g_sq_sample", state_bytes, total)) return M3G_ERR_SIZE;
  const int64_t N = sizes->n_atoms, S = sizes->n_structs, Q = sizes->n_q;
  const int32_t M = sizes->max_species, G = sizes->n_lags, remove_com = params->remove_com;
  hipStream_t s = (hipStream_t)stream_;
  const unsigned chunks = (unsigned)chunk_bound(N, S);   // workgroups beyond the table's chunk count return at once
  if (remove_com) hipLaunchKernelGGL(k_sq_com, dim3(chunks), dim3(kChunkRows), 0, s, st, pos, vel, forces, kick);
  const dim3 tiles(chunks, (unsigned)((st.cap + kQTile - 1) / kQTile));   // tiles beyond the structure's own vectors return at once
  const auto sv = st;   // (a structured binding cannot be captured)
  dispatch_species(M, [&](auto m) {
    hipLaunchKernelGGL(k_sq_density<decltype(m)::value>, tiles, dim3(kChunkRows), 0, s, sv, remove_com, pos, lattice, vel, forces, kick);
  });
  const int64_t store = Q * M > S ? Q * M : S;
  hipLaunchKernelGGL(k_sq_store, grid_for(store, kChunkRows), dim3(kChunkRows), 0, s, sv, lattice);
  const dim3 corr((unsigned)(Q + S), (unsigned)((G + kLagBlock - 1) / kLagBlock));
  dispatch_species(M, [&](auto m) { hipLaunchKernelGGL(k_sq_correlate<decltype(m)::value>, corr, dim3(kLagBlock), 0, s, sv); });
  M3G_RETURN_LAUNCH_STATUS();
}

extern "C" int m3g_sq_read(const m3g_sq_sizes* sizes, const void* state, size_t state_bytes, double* host_f, double* host_cl, double* host_ct,
                           int64_t* host_lag_count, int64_t* host_n_samples, int32_t* host_flags, void* stream_) {
  if (const char* why = sq_error(sizes, &kAnyParams)) { set_error("m3g_sq_read: %s", why); return M3G_ERR_VALUE; }
  if (!state) { set_error("m3g_sq_read: null argument"); return M3G_ERR_VALUE; }
  const auto [st, total] = sq_view(*sizes, (void*)state);
  if (!state_fits("m3g_sq_read", state_bytes, total)) return M3G_ERR_SIZE;
  const size_t S = sizes->n_structs, G = sizes->n_lags, cells = (size_t)sizes->n_q * species_pairs(sizes->max_species) * G;
  return read_all((hipStream_t)stream_,
                  {rb(host_f, (const double*)st.f, cells), rb(host_cl, (const double*)st.cl, cells), rb(host_ct, (const double*)st.ct, cells),
                   rb(host_lag_count, (const int64_t*)st.lag_count, S * G), rb(host_n_samples, (const int64_t*)st.n_samples, S),
                   rb(host_flags, (const int32_t*)st.flags, S)});
}

extern "C" int m3g_sq_frame(const m3g_sq_sizes* sizes, const void* state, size_t state_bytes, int32_t lag, double* host_rho, double* host_jl,
                            double* host_jt, void* stream_) {
  if (const char* why = sq_error(sizes, &kAnyParams)) { set_error("m3g_sq_frame: %s", why); return M3G_ERR_VALUE; }
  if (!state) { set_error("m3g_sq_frame: null argument"); return M3G_ERR_VALUE; }
  const auto [st, total] = sq_view(*sizes, (void*)state);
  if (!state_fits("m3g_sq_frame", state_bytes, total)) return M3G_ERR_SIZE;
  const int64_t G = sizes->n_lags, rows = sizes->n_q * sizes->max_species;
  hipStream_t s = (hipStream_t)stream_;
  int64_t ctr[kCounters];
  M3G_HIP_CHECK(hipMemcpyAsync(ctr, st.ctr, sizeof(ctr), hipMemcpyDeviceToHost, s));
  M3G_HIP_CHECK(hipStreamSynchronize(s));
  if (lag < 0 || lag >= G || lag >= ctr[kDone]) { set_error("m3g_sq_frame: no frame %d samples back", (int)lag); return M3G_ERR_VALUE; }
  std::vector<double> slot(rows * kEntry);
  M3G_HIP_CHECK(hipMemcpyAsync(slot.data(), st.ring + rows * kEntry * ((ctr[kDone] - 1 - lag) % G), 8 * rows * kEntry, hipMemcpyDeviceToHost, s));
  M3G_HIP_CHECK(hipStreamSynchronize(s));
  for (int64_t i = 0; i < rows; ++i) {
    const double* e = slot.data() + kEntry * i;
    if (host_rho) { host_rho[2 * i] = e[0]; host_rho[2 * i + 1] = e[1]; }
    if (host_jl) { host_jl[2 * i] = e[2]; host_jl[2 * i + 1] = e[3]; }
    if (host_jt)
      for (int k = 0; k < 6; ++k) host_jt[6 * i + k] = e[4 + k];
  }
  return M3G_OK;
}
