// Batched canonical atom-swap Monte Carlo (alone on a fixed lattice, or interleaved with the MD of m3g_dyn_*: the scheme of LAMMPS'
// fix atom/swap), the sibling of m3g_remd.hip.  A trial exchanges the OCCUPANTS of two rows of one structure: two entries of
// atom_types (and, with a dynamics state, their masses and velocities -- the atoms trade places and keep their own velocity).
// Positions never move, so every neighbour list stays valid, and the multiset of species is preserved, so the engine's range check
// stays true.  One trial of every structure of the batch is
//   m3g_mc_propose  k_mc_propose   one wave per structure: the two rank selections (ballot / popcount prefix ranks over the rows, 64 at a
//                                  time, the running rank in a scalar), the exchange, the pair, the verdict's uniform, PENDING;
//   (the caller's engine evaluation at the swapped species)
//   m3g_mc_decide   k_mc_verdict   one wave per structure: Metropolis on lane 0, the revert of a rejected pair by the lanes, the
//                                  statistics, the history row, the `accepted` word;
//                   k_mc_commit    one workgroup per chunk of the chunk table (m3g_chunks.h): the trial forces / stresses of accepted
//                                  structures become the current ones (not launched when the caller tracks energies only).
// No atomics: the order inside a structure is the lanes of its wave and a fixed strided loop over its rows, so a structure's results
// are bitwise the same alone or in any batch.  No allocation, copy or wait in either call (capture-safe: the counters live on the
// device).
#include <cmath>
#include <cstring>

#include "m3g_dyn_state.h"

namespace m3g {
namespace {
struct McView {
  int64_t S;
  ChunkView ch;
  const uint8_t* active;
  const double* temps;
  const uint64_t* seed;
  int32_t *flags, *pair, *accepted;
  int64_t *counter, *decided, *attempts, *accepts, *nonfinite, *count;
  double *u2, *mean, *m2;
};
Carved<McView> mc_view(int64_t N, int64_t S, void* state) {
  Carve c{state};
  McView st{S};
  st.ch = chunk_view(N, S, c);
  st.active = c.take<uint8_t>(N);        // per row
  st.temps = c.take<double>(S);
  st.seed = c.take<uint64_t>(S);
  st.flags = c.take<int32_t>(S);         // M3G_MC_*
  st.counter = c.take<int64_t>(S);       // proposals drawn = m3g_mc_propose calls
  st.decided = c.take<int64_t>(S);       // calls whose history row has been written
  st.pair = c.take<int32_t>(2 * S);      // rows (i, j) of the last attempted trial, relative to the structure
  st.u2 = c.take<double>(S);             // the verdict's uniform of the pending trial
  st.accepted = c.take<int32_t>(S);      // verdict of the last m3g_mc_decide (k_mc_commit reads it)
  st.attempts = c.take<int64_t>(S);
  st.accepts = c.take<int64_t>(S);
  st.nonfinite = c.take<int64_t>(S);
  st.count = c.take<int64_t>(S);
  st.mean = c.take<double>(S);
  st.m2 = c.take<double>(S);
  return {st, c.off};
}

// the rows lo .. hi of one structure, 64 at a time by one wave: row `row` takes part when it is active and (with `other` >= 0) holds
// another species than `other`
__device__ inline bool mc_takes_part(const uint8_t* active, const int64_t* types, int64_t row, int64_t hi, int64_t other) {
  return row < hi && active[row] != 0 && (other < 0 || types[row] != other);
}
__device__ inline int64_t mc_count(const uint8_t* active, const int64_t* types, int64_t lo, int64_t hi, int64_t other, int lane) {
  int64_t n = 0;
  for (int64_t base = lo; base < hi; base += kWave) n += __popcll(__ballot(mc_takes_part(active, types, base + lane, hi, other)));
  return n;
}
// the participating row of rank `rank` in row order (-1: there are not that many)
__device__ inline int64_t mc_select(const uint8_t* active, const int64_t* types, int64_t lo, int64_t hi, int64_t other, int64_t rank, int lane) {
  int64_t before = 0;   // participating rows below `base`: the same in every lane
  for (int64_t base = lo; base < hi; base += kWave) {
    const bool in = mc_takes_part(active, types, base + lane, hi, other);
    const unsigned long long mask = __ballot(in);
    const int64_t here = __popcll(mask);
    if (rank < before + here) {
      const int64_t prefix = __popcll(mask & ((1ull << lane) - 1ull));
      const unsigned long long hit = __ballot(in && before + prefix == rank);
      return base + (__ffsll((long long)hit) - 1);
    }
    before += here;
  }
  return -1;
}

__device__ inline void mc_swap_rows(int lane, int64_t i, int64_t j, int64_t* types, double* mass, double* v) {
  if (lane == 0) { const int64_t t = types[i]; types[i] = types[j]; types[j] = t; }
  if (mass && lane == 1) { const double m = mass[i]; mass[i] = mass[j]; mass[j] = m; }
  if (v && lane >= 2 && lane < 5) { const int k = lane - 2; const double x = v[3 * i + k]; v[3 * i + k] = v[3 * j + k]; v[3 * j + k] = x; }
}

// One wave (= one workgroup) per structure.  dyn_flags / mass / v are null without a dynamics state.
__global__ void __launch_bounds__(kWave) k_mc_propose(McView st, int64_t* __restrict__ types, const int32_t* __restrict__ dyn_flags,
                                                       double* __restrict__ mass, double* __restrict__ v, const float* __restrict__ energies) {
  const int64_t s = blockIdx.x;
  const int lane = threadIdx.x;
  if (s >= st.S) return;
  const int64_t lo = st.ch.offsets[s], hi = st.ch.offsets[s + 1];
  const int64_t a = st.counter[s];
  const int32_t flags = st.flags[s];
  int32_t set = 0;
  int64_t i = -1, j = -1;
  uint64_t c[4] = {(uint64_t)a, 0, 0, 0};
  if (flags & M3G_MC_PENDING) {
    set = M3G_MC_ERR_ORDER;   // sticky; the pending trial stays as it is
  } else if (!(dyn_flags && (dyn_flags[s] & (M3G_DYN_ERROR | M3G_DYN_STARTED))) && std::isfinite(energies[s])) {
    philox4x64_10(c, st.seed[s], 2);   // key word 2: disjoint from the Langevin draws (seed, 0) and replica exchange (seed, 1)
    const int64_t n_p = mc_count(st.active, types, lo, hi, -1, lane);
    if (n_p >= 2) {
      const int64_t ri = (int64_t)(uniform53(c[0]) * (double)n_p);
      i = mc_select(st.active, types, lo, hi, -1, ri < n_p - 1 ? ri : n_p - 1, lane);
    }
    if (i >= 0) {
      const int64_t si = types[i];
      const int64_t m = mc_count(st.active, types, lo, hi, si, lane);
      if (m >= 1) {
        const int64_t rj = (int64_t)(uniform53(c[1]) * (double)m);
        j = mc_select(st.active, types, lo, hi, si, rj < m - 1 ? rj : m - 1, lane);
      }
    }
    if (j < 0) set = M3G_MC_NO_PAIR;   // fewer than two species on the active rows
  }
  if (j >= 0) {
    __syncthreads();   // (every lane has read the species it compares before two of them move)
    mc_swap_rows(lane, i, j, types, mass, v);
    set = M3G_MC_PENDING;
    if (lane == 0) {
      st.pair[2 * s] = (int32_t)(i - lo);
      st.pair[2 * s + 1] = (int32_t)(j - lo);
      st.u2[s] = uniform53(c[2]);
    }
  }
  if (lane == 0) {
    if (set) st.flags[s] = flags | set;
    st.counter[s] = a + 1;
  }
}

__global__ void __launch_bounds__(kWave) k_mc_verdict(McView st, int64_t* __restrict__ types, double* __restrict__ mass, double* __restrict__ v,
                                                       const float* __restrict__ trial, float* __restrict__ energies, int32_t* __restrict__ history,
                                                       int64_t history_rows) {
#pragma clang fp contract(off)   // (the Welford update rounds as it is written)
  const int64_t s = blockIdx.x;
  const int lane = threadIdx.x;
  if (s >= st.S) return;
  const int64_t lo = st.ch.offsets[s];
  const int32_t flags = st.flags[s];
  const bool pending = (flags & M3G_MC_PENDING) != 0;
  const int64_t a = st.counter[s] - 1;   // the call this verdict belongs to
  const bool row_due = st.decided[s] != a + 1;
  const int32_t pi = st.pair[2 * s], pj = st.pair[2 * s + 1];
  int accept = 0;
  if (pending && lane == 0) {
    const double e_new = (double)trial[s], e_old = (double)energies[s];
    bool bad = false;
    if (!std::isfinite(e_new)) {
      bad = true;   // rejected explicitly: -inf would pass dE <= 0
    } else {
      const double dE = e_new - e_old;
      accept = (dE <= 0.0 || st.u2[s] < exp(-dE / (kBoltzmann * st.temps[s]))) ? 1 : 0;
    }
    if (accept) energies[s] = trial[s];
    const double e = accept ? e_new : e_old;   // the current energy after the verdict
    st.attempts[s] += 1;
    st.accepts[s] += accept;
    if (bad) st.nonfinite[s] += 1;
    const int64_t n = st.count[s] + 1;
    const double d = e - st.mean[s];
    const double mean = st.mean[s] + d / (double)n;
    st.count[s] = n;
    st.mean[s] = mean;
    st.m2[s] += d * (e - mean);
    st.flags[s] = flags & ~M3G_MC_PENDING;
  }
  accept = __shfl(accept, 0, kWave);
  if (pending && !accept) mc_swap_rows(lane, lo + pi, lo + pj, types, mass, v);   // the same two rows back: bitwise what they were
  if (lane == 0) {
    st.accepted[s] = accept;
    if (row_due && a >= 0) {
      if (history && a < history_rows) {
        int32_t* h = history + 3 * (a * st.S + s);
        h[0] = pending ? pi : -1;
        h[1] = pending ? pj : -1;
        h[2] = pending ? accept : -1;
      }
      st.decided[s] = a + 1;
    }
  }
}

// One workgroup per chunk, thread t on row t of the chunk.  forces / stresses pairs may be null.
__global__ void __launch_bounds__(kChunkRows) k_mc_commit(McView st, const float* __restrict__ trial_forces, float* __restrict__ forces,
                                                           const float* __restrict__ trial_stresses, float* __restrict__ stresses) {
  const int c = blockIdx.x;
  if (c >= st.ch.n_chunks()) return;
  const int s = st.ch.structure(c);
  if (!st.accepted[s]) return;   // bitwise untouched
  const int t = threadIdx.x;
  const int64_t i = st.ch.row(c, t);
  if (forces && st.ch.holds(s, i))
    for (int k = 0; k < 3; ++k) forces[3 * i + k] = trial_forces[3 * i + k];
  if (stresses && c == st.ch.chunks_begin(s) && t < 6) stresses[6 * (int64_t)s + t] = trial_stresses[6 * (int64_t)s + t];
}

}  // namespace
}  // namespace m3g

using namespace m3g;

extern "C" int m3g_mc_state_bytes(int64_t n_atoms, int64_t n_structs, size_t* bytes) {
  if (!bytes || !batch32_sizes_ok(n_atoms, n_structs)) { set_error("m3g_mc_state_bytes: null argument or bad sizes"); return M3G_ERR_VALUE; }
  *bytes = mc_view(n_atoms, n_structs, nullptr).bytes;
  return M3G_OK;
}

extern "C" int m3g_mc_init(int64_t n_atoms, int64_t n_structs, const int64_t* host_offsets, const double* host_temperatures,
                           const uint64_t* host_seeds, const uint8_t* host_active, void* state, size_t state_bytes, void* stream_) {
  const int64_t N = n_atoms, S = n_structs;
  if (!batch32_sizes_ok(N, S) || !host_offsets || !host_temperatures || !host_seeds || !host_active || !state) {
    set_error("m3g_mc_init: null argument or bad sizes");
    return M3G_ERR_VALUE;
  }
  if (!offsets_ok("m3g_mc_init", host_offsets, N, S)) return M3G_ERR_VALUE;
  for (int64_t s = 0; s < S; ++s) {
    if (!temperature_ok("m3g_mc_init", host_temperatures, s)) return M3G_ERR_VALUE;
    if (!structure_fits_int32("m3g_mc_init", host_offsets, s)) return M3G_ERR_VALUE;
  }
  const auto [st, total] = mc_view(N, S, state);
  if (!state_fits("m3g_mc_init", state_bytes, total, true)) return M3G_ERR_SIZE;
  std::vector<char> image(total, 0);   // counters, statistics and flags start at zero (the chunk table's part is not sent: upload_image)
  const McView im = mc_view(N, S, image.data()).view;
  for (int64_t i = 0; i < N; ++i) ((uint8_t*)im.active)[i] = host_active[i] ? 1 : 0;
  std::memcpy((void*)im.temps, host_temperatures, 8 * S);
  std::memcpy((void*)im.seed, host_seeds, 8 * S);
  for (int64_t s = 0; s < S; ++s) {
    int64_t n_p = 0;
    for (int64_t i = host_offsets[s]; i < host_offsets[s + 1]; ++i) n_p += host_active[i] ? 1 : 0;
    if (n_p < 2) im.flags[s] = M3G_MC_NO_PAIR;   // (the species are the device's to look at: k_mc_propose)
  }
  return upload_image(image, state, st.active, (const char*)state + total, st.ch, host_offsets, (hipStream_t)stream_);   // all after the table
}

extern "C" int m3g_mc_propose(int64_t n_atoms, int64_t n_structs, void* state, size_t state_bytes, int64_t* atom_types, void* dyn_state,
                              size_t dyn_bytes, const float* energies, void* stream_) {
  const int64_t N = n_atoms, S = n_structs;
  if (!batch32_sizes_ok(N, S) || !state || !atom_types || !energies) { set_error("m3g_mc_propose: null argument or bad sizes"); return M3G_ERR_VALUE; }
  const auto [st, total] = mc_view(N, S, state);
  const auto [dyn, dyn_total] = dyn_state ? dyn_view(N, S, dyn_state) : Carved<DynView>{};
  if (!state_fits("m3g_mc_propose", state_bytes, total, false, "Monte Carlo")) return M3G_ERR_SIZE;
  if (!state_fits("m3g_mc_propose", dyn_bytes, dyn_total, false, "dynamics")) return M3G_ERR_SIZE;
  hipLaunchKernelGGL(k_mc_propose, dim3((unsigned)S), dim3(kWave), 0, (hipStream_t)stream_, st, atom_types, dyn.flags, dyn.mass,
                     dyn.v, energies);
  M3G_RETURN_LAUNCH_STATUS();
}

extern "C" int m3g_mc_decide(int64_t n_atoms, int64_t n_structs, void* state, size_t state_bytes, int64_t* atom_types, void* dyn_state,
                             size_t dyn_bytes, const float* trial_energies, const float* trial_forces, const float* trial_stresses,
                             float* energies, float* forces, float* stresses, int32_t* history, int64_t history_rows, void* stream_) {
  const int64_t N = n_atoms, S = n_structs;
  if (!batch32_sizes_ok(N, S) || !state || !atom_types || !trial_energies || !energies || history_rows < 0) {
    set_error("m3g_mc_decide: null argument or bad sizes");
    return M3G_ERR_VALUE;
  }
  if (!trial_forces != !forces || !trial_stresses != !stresses) {
    set_error("m3g_mc_decide: trial and current forces (stresses) must be given together");
    return M3G_ERR_VALUE;
  }
  const auto [st, total] = mc_view(N, S, state);
  const auto [dyn, dyn_total] = dyn_state ? dyn_view(N, S, dyn_state) : Carved<DynView>{};
  if (!state_fits("m3g_mc_decide", state_bytes, total, false, "Monte Carlo")) return M3G_ERR_SIZE;
  if (!state_fits("m3g_mc_decide", dyn_bytes, dyn_total, false, "dynamics")) return M3G_ERR_SIZE;
  hipStream_t s = (hipStream_t)stream_;
  hipLaunchKernelGGL(k_mc_verdict, dim3((unsigned)S), dim3(kWave), 0, s, st, atom_types, dyn.mass, dyn.v, trial_energies, energies, history,
                     history_rows);
  if (forces || stresses)
    hipLaunchKernelGGL(k_mc_commit, dim3((unsigned)chunk_bound(N, S)), dim3(kChunkRows), 0, s, st, trial_forces, forces, trial_stresses, stresses);
  M3G_RETURN_LAUNCH_STATUS();
}

extern "C" int m3g_mc_read(int64_t n_atoms, int64_t n_structs, const void* state, size_t state_bytes, int32_t* host_flags, int64_t* host_counters,
                           int64_t* host_attempts, int64_t* host_accepts, int64_t* host_nonfinite, int64_t* host_count, double* host_mean,
                           double* host_m2, int32_t* host_pairs, void* stream_) {
  const int64_t N = n_atoms, S = n_structs;
  if (!batch32_sizes_ok(N, S) || !state) { set_error("m3g_mc_read: null argument or bad sizes"); return M3G_ERR_VALUE; }
  const auto [st, total] = mc_view(N, S, (void*)state);
  if (!state_fits("m3g_mc_read", state_bytes, total)) return M3G_ERR_SIZE;
  return read_all((hipStream_t)stream_,
                  {rb(host_flags, st.flags, S), rb(host_counters, st.counter, S), rb(host_attempts, st.attempts, S), rb(host_accepts, st.accepts, S),
                   rb(host_nonfinite, st.nonfinite, S), rb(host_count, st.count, S), rb(host_mean, st.mean, S), rb(host_m2, st.m2, S),
                   rb(host_pairs, st.pair, 2 * S)});
}
