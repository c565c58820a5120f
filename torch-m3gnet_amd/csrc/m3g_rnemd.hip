// Batched reverse non-equilibrium MD (Mueller-Plathe 1997 for heat, 1999 for momentum; the unequal-mass exchange of Nieto-Draghi and
// Avalos 2003; LAMMPS' fix thermal/conductivity and fix viscosity) over the state of m3g_dyn_* (m3g_dyn_state.h), the sibling of
// m3g_remd.hip and m3g_mc.hip.  Every structure is cut into n_slabs slabs along one lattice direction.  An exchange takes the
// hottest (fastest along flow_axis) atoms of slab 0 and the coldest (slowest) of slab n_slabs / 2 and exchanges their velocities, which
// conserves the energy and the momentum of the structure: the flux is imposed, the profile over the slabs is the response.  Positions
// never move, so every neighbour list stays valid.  One m3g_rnemd_exchange, at a synchronous point of the integrator (after a
// finish_only m3g_dyn_step), is two launches:
//   k_rnemd_chunks    one workgroup per chunk of the chunk table (m3g_chunks.h), thread t on row t: slab, selection key and the five
//                     sampled terms of every row go to LDS; lane b < n_slabs of wave w walks the rows 64 w .. 64 w + 63 in row order for
//                     the partials of slab b, and the four are added in row order; wave 0 (wave 1) picks the chunk's first n_swaps
//                     candidates of slab 0 (the middle slab), pick after pick by a butterfly under the total order (key, row);
//   k_rnemd_finalize  one wave per structure: pair p = the p-th candidate of either list over the structure's chunks (lane-strided
//                     over the chunks' candidates, a butterfly under the total order (key, row)), the exchange of the <= 8 pairs by
//                     lane 0 in the order p = 0, 1, ..., then lane b < n_slabs adds the chunk partials of slab b in chunk order.
// No atomics: a chunk never straddles a structure and the orders above are fixed, so every result of a structure depends on its own
// rows only -- bitwise the same alone or in any batch.  No allocation, copy or wait in m3g_rnemd_exchange (capture-safe: the
// counters live on the device).
#include <cmath>
#include <cstring>

#include "m3g_dyn_state.h"

namespace m3g {
namespace {
constexpr int kTerms = 5;                          // sum m, sum m vx, sum m vy, sum m vz, sum m |v|^2
constexpr int kMaxSwaps = M3G_RNEMD_MAX_SWAPS;
constexpr int kMaxSlabs = M3G_RNEMD_MAX_SLABS;
static_assert(kMaxSlabs <= kWave && 2 * kMaxSwaps <= kChunkRows, "one lane per slab, one thread per candidate slot");

struct RnemdView {
  int64_t S;
  int32_t n_slabs;
  ChunkView ch;
  const uint8_t* active;
  const double* g;                 // [S,3]: column `axis` of the inverse lattice
  int64_t* part_count;             // per chunk and slab
  double* part_sums;               // per chunk and slab: kTerms
  double* cand_key;                // per chunk and list (0: slab 0, 1: slab n_slabs / 2): kMaxSwaps, best first
  int32_t* cand_row;               // rows relative to the structure, -1 = none
  int64_t *n_calls, *n_exchanged, *n_samples;
  double* transferred;
  int32_t* last_pairs;             // [S, n_swaps, 2] at the front of a region of S * kMaxSwaps * 2
  int64_t* count;                  // [S, n_slabs]
  double* sums;                    // [S, n_slabs, kTerms]
};
Carved<RnemdView> rnemd_view(int64_t N, int64_t S, int32_t n_slabs, void* state) {
  Carve c{state};
  const int64_t C = chunk_bound(N, S);
  RnemdView st{S, n_slabs};
  st.ch = chunk_view(N, S, c);
  st.active = c.take<uint8_t>(N);
  st.g = c.take<double>(3 * S);
  st.part_count = c.take<int64_t>(C * n_slabs);
  st.part_sums = c.take<double>(C * n_slabs * kTerms);
  st.cand_key = c.take<double>(C * 2 * kMaxSwaps);
  st.cand_row = c.take<int32_t>(C * 2 * kMaxSwaps);
  st.n_calls = c.take<int64_t>(S);
  st.n_exchanged = c.take<int64_t>(S);
  st.n_samples = c.take<int64_t>(S);
  st.transferred = c.take<double>(S);
  st.last_pairs = c.take<int32_t>(S * kMaxSwaps * 2);
  st.count = c.take<int64_t>(S * n_slabs);
  st.sums = c.take<double>(S * n_slabs * kTerms);
  return {st, c.off};
}

// the total order of a candidate list: slab 0 takes the largest key first, the middle slab the smallest; ties go to the lower row
__device__ inline bool rnemd_before(int list, double ka, int32_t ra, double kb, int32_t rb) {
  return (list == 0 ? ka > kb : ka < kb) || (ka == kb && ra < rb);
}

// One workgroup per chunk, thread t on row t of the chunk.
__global__ void __launch_bounds__(kChunkRows) k_rnemd_chunks(RnemdView st, m3g_rnemd_params p, const int32_t* __restrict__ flags,
                                                             const double* __restrict__ mass, const double* __restrict__ v,
                                                             const double* __restrict__ pos, int do_sample) {
#pragma clang fp contract(off)   // (the slab of a row and every sampled term round as they are written)
  __shared__ double sh_term[kTerms][kChunkRows];
  __shared__ double sh_key[kChunkRows];
  __shared__ int32_t sh_slab[kChunkRows];      // -1: no row here
  __shared__ int32_t sh_list[kChunkRows];      // 0 / 1: candidate of that list, -1: of neither
  __shared__ double sh_cand_key[2 * kMaxSwaps];
  __shared__ int32_t sh_cand_row[2 * kMaxSwaps];
  __shared__ double sh_part[kChunkRows / kWave][kTerms][kWave];   // per wave and slab
  __shared__ int32_t sh_part_n[kChunkRows / kWave][kWave];
  const int c = blockIdx.x;
  if (c >= st.ch.n_chunks()) return;
  const int s = st.ch.structure(c);
  if (flags[s] & (M3G_DYN_ERROR | M3G_DYN_STARTED)) return;   // k_rnemd_finalize skips the structure too: nothing of it is read
  const int t = threadIdx.x;
  const int n_slabs = st.n_slabs;
  const int64_t i = st.ch.row(c, t);
  const bool here = st.ch.holds(s, i);
  int32_t slab = -1, list = -1;
  double key = 0.0;
  double term[kTerms] = {0.0, 0.0, 0.0, 0.0, 0.0};
  if (here) {
    const double* g = st.g + 3 * (int64_t)s;
    double f = (pos[3 * i] * g[0] + pos[3 * i + 1] * g[1]) + pos[3 * i + 2] * g[2];
    f -= floor(f);
    const double scaled = f * (double)n_slabs;
    slab = scaled >= 0.0 ? (int32_t)scaled : 0;   // (a non-finite position: slab 0, as any definite answer would do)
    if (slab > n_slabs - 1) slab = n_slabs - 1;   // a wrapped f of exactly 1.0
    const double m = mass[i], vx = v[3 * i], vy = v[3 * i + 1], vz = v[3 * i + 2];
    term[0] = m;
    term[1] = m * vx;
    term[2] = m * vy;
    term[3] = m * vz;
    term[4] = m * ((vx * vx + vy * vy) + vz * vz);
    key = p.kind == M3G_RNEMD_HEAT ? term[4] : v[3 * i + p.flow_axis];
    if (st.active[i] && std::isfinite(key)) list = slab == 0 ? 0 : (slab == n_slabs / 2 ? 1 : -1);
  }
  for (int j = 0; j < kTerms; ++j) sh_term[j][t] = term[j];
  sh_key[t] = key;
  sh_slab[t] = slab;
  sh_list[t] = list;
  if (t < 2 * kMaxSwaps) { sh_cand_key[t] = 0.0; sh_cand_row[t] = -1; }
  __syncthreads();
  const int rows = (int)min((int64_t)kChunkRows, st.ch.offsets[s + 1] - st.ch.row(c, 0));   // the chunk's rows (its last one may be part-filled)
  const int w = t / kWave, lane = t % kWave;
  if (do_sample && lane < n_slabs) {   // wave w: the partials of slab `lane` over the rows 64 w .. 64 w + 63, in row order
    int32_t n = 0;
    double acc[kTerms] = {0.0, 0.0, 0.0, 0.0, 0.0};
    // without a branch, so that the LDS reads of several rows are in flight together: a row of another slab adds +0.0, which changes
    // no bit (a sum that starts at +0.0 is never -0.0 in round-to-nearest)
    const int u_end = min(kWave * (w + 1), rows);
#pragma unroll 8
    for (int u = kWave * w; u < u_end; ++u) {
      const bool in = sh_slab[u] == lane;
      n += in ? 1 : 0;
      for (int j = 0; j < kTerms; ++j) acc[j] += in ? sh_term[j][u] : 0.0;
    }
    sh_part_n[w][lane] = n;
    for (int j = 0; j < kTerms; ++j) sh_part[w][j][lane] = acc[j];
  }
  if (w < 2) {   // wave 0: the candidates of slab 0, wave 1: those of the middle slab -- pick after pick, each the best that comes after the last
    double key_prev = 0.0;
    int row_prev = -1;
    for (int q = 0; q < p.n_swaps; ++q) {
      double k_best = 0.0;
      int r_best = -1;
      for (int u = lane; u < rows; u += kWave) {
        if (sh_list[u] != w) continue;
        const double k = sh_key[u];
        if (row_prev >= 0 && !rnemd_before(w, key_prev, row_prev, k, u)) continue;
        if (r_best < 0 || rnemd_before(w, k, u, k_best, r_best)) { k_best = k; r_best = u; }
      }
#pragma unroll
      for (int x = kWave / 2; x > 0; x >>= 1) {
        const double k = __shfl_xor(k_best, x, kWave);
        const int r = __shfl_xor(r_best, x, kWave);
        if (r >= 0 && (r_best < 0 || rnemd_before(w, k, r, k_best, r_best))) { k_best = k; r_best = r; }
      }
      if (r_best < 0) break;   // (the same in every lane)
      if (lane == 0) {
        sh_cand_key[w * kMaxSwaps + q] = k_best;
        sh_cand_row[w * kMaxSwaps + q] = (int32_t)(st.ch.row(c, r_best) - st.ch.offsets[s]);
      }
      key_prev = k_best;
      row_prev = r_best;
    }
  }
  __syncthreads();
  if (do_sample && t < n_slabs) {   // the four partials of slab t in row order, from zero
    int64_t n = 0;
    double acc[kTerms] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int x = 0; x < kChunkRows / kWave; ++x) {
      n += sh_part_n[x][t];
      for (int j = 0; j < kTerms; ++j) acc[j] += sh_part[x][j][t];
    }
    const int64_t at = (int64_t)c * n_slabs + t;
    st.part_count[at] = n;
    for (int j = 0; j < kTerms; ++j) st.part_sums[kTerms * at + j] = acc[j];
  }
  if (t < 2 * kMaxSwaps) {
    st.cand_key[(int64_t)c * 2 * kMaxSwaps + t] = sh_cand_key[t];
    st.cand_row[(int64_t)c * 2 * kMaxSwaps + t] = sh_cand_row[t];
  }
}

// the best candidate of `list` over the chunks c0 .. c1 that comes strictly after (key_prev, row_prev) (row_prev < 0: the first);
// the same (key, row) in every lane, row -1 when there is none
__device__ inline void rnemd_next(const RnemdView& st, int list, int c0, int c1, int n_swaps, int lane, double key_prev, int32_t row_prev,
                                  double& key_out, int32_t& row_out) {
  double key = 0.0;
  int32_t row = -1;
  const int slots = (c1 - c0) * n_swaps;
  for (int q = lane; q < slots; q += kWave) {
    const int64_t at = ((int64_t)(c0 + q / n_swaps) * 2 + list) * kMaxSwaps + q % n_swaps;
    const int32_t r = st.cand_row[at];
    if (r < 0) continue;
    const double k = st.cand_key[at];
    if (row_prev >= 0 && !rnemd_before(list, key_prev, row_prev, k, r)) continue;
    if (row < 0 || rnemd_before(list, k, r, key, row)) { key = k; row = r; }
  }
#pragma unroll
  for (int w = kWave / 2; w > 0; w >>= 1) {
    const double k = __shfl_xor(key, w, kWave);
    const int32_t r = __shfl_xor(row, w, kWave);
    if (r >= 0 && (row < 0 || rnemd_before(list, k, r, key, row))) { key = k; row = r; }
  }
  key_out = key;
  row_out = row;
}

// One wave per structure, kFinalizeWaves structures per workgroup (no barrier: the waves share nothing).
__global__ void __launch_bounds__(kFinalizeWaves * kWave) k_rnemd_finalize(RnemdView st, m3g_rnemd_params p, const int32_t* __restrict__ flags,
                                                                           const double* __restrict__ mass, double* __restrict__ v,
                                                                           int do_swap, int do_sample) {
#pragma clang fp contract(off)   // (the exchange and the transferred quantity round as they are written)
  const int64_t s = (int64_t)blockIdx.x * kFinalizeWaves + threadIdx.x / kWave;
  const int lane = threadIdx.x % kWave;
  if (s >= st.S) return;
  if (flags[s] & (M3G_DYN_ERROR | M3G_DYN_STARTED)) return;   // bitwise untouched, not sampled, not counted
  const int c0 = st.ch.chunks_begin(s), c1 = st.ch.chunks_end(s);
  const int64_t lo = st.ch.offsets[s];
  const int n_slabs = st.n_slabs, n_swaps = p.n_swaps;
  if (do_swap) {
    double k0 = 0.0, k1 = 0.0, moved = st.transferred[s];
    int32_t r0 = -1, r1 = -1;
    int64_t n_done = 0;
    bool more = true;   // both lists still held a candidate at the pair before
    for (int q = 0; q < n_swaps; ++q) {
      if (more) {
        rnemd_next(st, 0, c0, c1, n_swaps, lane, k0, r0, k0, r0);
        rnemd_next(st, 1, c0, c1, n_swaps, lane, k1, r1, k1, r1);
        more = r0 >= 0 && r1 >= 0;
      }
      const bool swap = more && k0 > k1;
      more = swap;   // slab 0 only gets colder (slower) down its list and the middle slab hotter: no later pair can be ahead
      if (lane == 0) {
        st.last_pairs[(s * n_swaps + q) * 2] = swap ? r0 : -1;
        st.last_pairs[(s * n_swaps + q) * 2 + 1] = swap ? r1 : -1;
      }
      if (!swap || lane != 0) continue;
      const int64_t i = lo + r0, j = lo + r1;
      const double mi = mass[i], mj = mass[j];
      const int k_lo = p.kind == M3G_RNEMD_HEAT ? 0 : p.flow_axis, k_hi = p.kind == M3G_RNEMD_HEAT ? 3 : p.flow_axis + 1;
      double vi[3], wi[3];   // the slab-0 row before and after
      for (int k = 0; k < 3; ++k) vi[k] = wi[k] = v[3 * i + k];
      for (int k = k_lo; k < k_hi; ++k) {
        const double a = v[3 * i + k], b = v[3 * j + k];
        if (mi == mj) {
          v[3 * i + k] = b;
          v[3 * j + k] = a;
          wi[k] = b;
        } else {
          const double vcm = (mi * a + mj * b) / (mi + mj);
          wi[k] = 2.0 * vcm - a;
          v[3 * i + k] = wi[k];
          v[3 * j + k] = 2.0 * vcm - b;
        }
      }
      if (p.kind == M3G_RNEMD_HEAT) {
        const double before = (vi[0] * vi[0] + vi[1] * vi[1]) + vi[2] * vi[2], after = (wi[0] * wi[0] + wi[1] * wi[1]) + wi[2] * wi[2];
        moved += 0.5 * mi * (before - after) / kKappa;
      } else {
        moved += mi * (vi[p.flow_axis] - wi[p.flow_axis]);
      }
      n_done += 1;
    }
    if (lane == 0) {
      st.transferred[s] = moved;
      st.n_exchanged[s] += n_done;
    }
  }
  if (do_sample && lane < n_slabs) {   // slab `lane`: the chunk partials in chunk order, then one addition to the accumulator
    int64_t n = 0;
    double acc[kTerms] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
    for (int c = c0; c < c1; ++c) {
      const int64_t at = (int64_t)c * n_slabs + lane;
      n += st.part_count[at];
      for (int j = 0; j < kTerms; ++j) acc[j] += st.part_sums[kTerms * at + j];
    }
    const int64_t at = s * n_slabs + lane;
    st.count[at] += n;
    for (int j = 0; j < kTerms; ++j) st.sums[kTerms * at + j] += acc[j];
  }
  if (lane == 0) {
    st.n_calls[s] += 1;
    if (do_sample) st.n_samples[s] += 1;
  }
}

bool rnemd_slabs_ok(int32_t n_slabs) { return n_slabs >= 2 && n_slabs <= kMaxSlabs && n_slabs % 2 == 0; }

bool rnemd_params_ok(const char* fn, const m3g_rnemd_params* p) {
  if (p->kind != M3G_RNEMD_HEAT && p->kind != M3G_RNEMD_MOMENTUM) { set_error("%s: unknown kind %d", fn, p->kind); return false; }
  if (p->axis < 0 || p->axis > 2 || p->flow_axis < 0 || p->flow_axis > 2) { set_error("%s: axis and flow_axis must be 0, 1 or 2", fn); return false; }
  if (p->kind == M3G_RNEMD_MOMENTUM && p->flow_axis == p->axis) {
    set_error("%s: the momentum exchanged must be perpendicular to the slab normal (flow_axis != axis)", fn);
    return false;
  }
  if (!rnemd_slabs_ok(p->n_slabs)) { set_error("%s: n_slabs must be even, >= 2 and <= %d", fn, kMaxSlabs); return false; }
  if (p->n_swaps < 1 || p->n_swaps > kMaxSwaps) { set_error("%s: n_swaps must be 1 .. %d", fn, kMaxSwaps); return false; }
  return true;
}
}  // namespace
}  // namespace m3g

using namespace m3g;

extern "C" int m3g_rnemd_state_bytes(int64_t n_atoms, int64_t n_structs, int32_t n_slabs, size_t* bytes) {
  if (!bytes || !batch32_sizes_ok(n_atoms, n_structs) || !rnemd_slabs_ok(n_slabs)) {
    set_error("m3g_rnemd_state_bytes: null argument or bad sizes");
    return M3G_ERR_VALUE;
  }
  *bytes = rnemd_view(n_atoms, n_structs, n_slabs, nullptr).bytes;
  return M3G_OK;
}

extern "C" int m3g_rnemd_init(const m3g_rnemd_params* params, int64_t n_atoms, int64_t n_structs, const int64_t* host_offsets,
                              const double* host_lattices, const uint8_t* host_active, void* state, size_t state_bytes, void* stream_) {
  const int64_t N = n_atoms, S = n_structs;
  if (!params || !batch32_sizes_ok(N, S) || !host_offsets || !host_lattices || !state) {
    set_error("m3g_rnemd_init: null argument or bad sizes");
    return M3G_ERR_VALUE;
  }
  if (!rnemd_params_ok("m3g_rnemd_init", params)) return M3G_ERR_VALUE;
  if (!offsets_ok("m3g_rnemd_init", host_offsets, N, S)) return M3G_ERR_VALUE;
  for (int64_t s = 0; s < S; ++s) {
    if (!lattice_ok("m3g_rnemd_init", host_lattices + 9 * s, s)) return M3G_ERR_VALUE;
    if (!structure_fits_int32("m3g_rnemd_init", host_offsets, s)) return M3G_ERR_VALUE;
  }
  const auto [st, total] = rnemd_view(N, S, params->n_slabs, state);
  if (!state_fits("m3g_rnemd_init", state_bytes, total, true)) return M3G_ERR_SIZE;
  std::vector<char> image(total, 0);   // counters and accumulators start at zero (the chunk table's part is not sent: upload_image)
  const RnemdView im = rnemd_view(N, S, params->n_slabs, image.data()).view;
  for (int64_t i = 0; i < N; ++i) ((uint8_t*)im.active)[i] = (!host_active || host_active[i]) ? 1 : 0;
  for (int64_t s = 0; s < S; ++s) {
    double inv[9];
    inv3(host_lattices + 9 * s, inv);   // rows = lattice vectors: fractional = cartesian . inverse
    for (int k = 0; k < 3; ++k) ((double*)im.g)[3 * s + k] = inv[3 * k + params->axis];
  }
  for (int64_t q = 0; q < S * kMaxSwaps * 2; ++q) im.last_pairs[q] = -1;
  return upload_image(image, state, st.active, (const char*)state + total, st.ch, host_offsets, (hipStream_t)stream_);   // all after the table
}

extern "C" int m3g_rnemd_exchange(const m3g_rnemd_params* params, int64_t n_atoms, int64_t n_structs, void* state, size_t state_bytes,
                                  void* dyn_state, size_t dyn_bytes, const double* pos, int32_t do_swap, int32_t do_sample, void* stream_) {
  const int64_t N = n_atoms, S = n_structs;
  if (!params || !batch32_sizes_ok(N, S) || !state || !dyn_state || !pos) {
    set_error("m3g_rnemd_exchange: null argument or bad sizes");
    return M3G_ERR_VALUE;
  }
  if (!rnemd_params_ok("m3g_rnemd_exchange", params)) return M3G_ERR_VALUE;
  const auto [st, total] = rnemd_view(N, S, params->n_slabs, state);
  const auto [dyn, dyn_total] = dyn_view(N, S, dyn_state);
  if (!state_fits("m3g_rnemd_exchange", state_bytes, total, false, "rNEMD")) return M3G_ERR_SIZE;
  if (!state_fits("m3g_rnemd_exchange", dyn_bytes, dyn_total, false, "dynamics")) return M3G_ERR_SIZE;
  if (!do_swap && !do_sample) return M3G_OK;   // nothing asked for
  hipStream_t s = (hipStream_t)stream_;
  hipLaunchKernelGGL(k_rnemd_chunks, dim3((unsigned)chunk_bound(N, S)), dim3(kChunkRows), 0, s, st, *params, dyn.flags, dyn.mass, dyn.v, pos,
                     do_sample ? 1 : 0);
  hipLaunchKernelGGL(k_rnemd_finalize, dim3((unsigned)((S + kFinalizeWaves - 1) / kFinalizeWaves)), dim3(kFinalizeWaves * kWave), 0, s, st,
                     *params, dyn.flags, dyn.mass, dyn.v, do_swap ? 1 : 0, do_sample ? 1 : 0);
  M3G_RETURN_LAUNCH_STATUS();
}

extern "C" int m3g_rnemd_read(const m3g_rnemd_params* params, int64_t n_atoms, int64_t n_structs, const void* state, size_t state_bytes,
                              int64_t* host_n_calls, int64_t* host_n_exchanged, double* host_transferred, int64_t* host_n_samples,
                              int32_t* host_last_pairs, int64_t* host_count, double* host_sums, void* stream_) {
  const int64_t N = n_atoms, S = n_structs;
  if (!params || !batch32_sizes_ok(N, S) || !state) { set_error("m3g_rnemd_read: null argument or bad sizes"); return M3G_ERR_VALUE; }
  if (!rnemd_params_ok("m3g_rnemd_read", params)) return M3G_ERR_VALUE;
  const auto [st, total] = rnemd_view(N, S, params->n_slabs, (void*)state);
  if (!state_fits("m3g_rnemd_read", state_bytes, total)) return M3G_ERR_SIZE;
  return read_all((hipStream_t)stream_,
                  {rb(host_n_calls, st.n_calls, S), rb(host_n_exchanged, st.n_exchanged, S), rb(host_transferred, st.transferred, S),
                   rb(host_n_samples, st.n_samples, S), rb(host_last_pairs, st.last_pairs, S * params->n_swaps * 2),
                   rb(host_count, st.count, S * params->n_slabs), rb(host_sums, st.sums, S * params->n_slabs * kTerms)});
}
