// Batched replica-exchange MD (parallel tempering, Sugita and Okamoto 1999) over the state of m3g_dyn_* (m3g_dyn_state.h).  The S
// structures of an MD batch are cut into G ladders, contiguous runs of R_g >= 2 replicas of one system; ladder g has R_g ascending
// temperatures and replica lo_g + k starts holding temperature index k.  An exchange swaps TEMPERATURES, never configurations: the
// positions stay in their rows, so every neighbour list stays valid.  One m3g_remd_exchange, at a synchronous point of the integrator
// (after a finish_only m3g_dyn_step), is two launches:
//   k_remd_decide    one wave per ladder: the energy statistics of every temperature index, the Metropolis verdicts of the pairs
//                    (k, k+1) with k % 2 == attempt % 2 (lane-strided; the pairs of one parity share no replica), the swapped target
//                    temperatures written into the dyn state, the velocity scale of every replica, the round-trip labels, one row
//                    of the history and the attempt counter;
//   k_remd_rescale   one workgroup per chunk of the dyn state's chunk table: v *= scale; a chunk whose scale is exactly 1 returns at
//                    once.
// No atomics: the order inside a ladder is the lanes of its wave and a fixed strided loop, so a ladder's results depend on its own
// replicas only -- bitwise the same alone or beside any other ladders.  No allocation, copy or wait in m3g_remd_exchange
// (capture-safe: the attempt counter lives on the device).
#include <cmath>
#include <cstring>

#include "m3g_dyn_state.h"

namespace m3g {
namespace {
constexpr int kUp = 1, kDown = 2;   // round-trip labels: last end of the ladder touched was index 0 / index R-1 (after index 0)

struct RemdView {
  int64_t S, G;
  const int64_t* offsets;
  int32_t *held, *label, *holder;
  double *scale, *mean, *m2;
  int64_t *trips, *count, *attempts, *accepts, *counter;
  const double* temps;
  const uint64_t* seed;
};
Carved<RemdView> remd_view(int64_t S, int64_t G, void* state) {
  Carve c{state};
  RemdView st{S, G};
  st.offsets = c.take<int64_t>(G + 1);
  st.held = c.take<int32_t>(S);       // per replica
  st.scale = c.take<double>(S);
  st.label = c.take<int32_t>(S);
  st.trips = c.take<int64_t>(S);
  st.holder = c.take<int32_t>(S);     // per (ladder, temperature index): row lo_g + k
  st.count = c.take<int64_t>(S);
  st.mean = c.take<double>(S);
  st.m2 = c.take<double>(S);
  st.attempts = c.take<int64_t>(S);   // per pair (k, k+1): row lo_g + k (row lo_g + R_g - 1 stays 0)
  st.accepts = c.take<int64_t>(S);
  st.counter = c.take<int64_t>(G);    // per ladder
  st.temps = c.take<double>(S);
  st.seed = c.take<uint64_t>(G);
  return {st, c.off};
}

// One wave (= one workgroup, so __syncthreads is the wave's barrier and makes its writes visible to its other lanes) per ladder.
__global__ void __launch_bounds__(kWave) k_remd_decide(RemdView st, double* __restrict__ t0, const int32_t* __restrict__ flags,
                                                        const float* __restrict__ energies, int32_t* __restrict__ history,
                                                        int64_t history_rows) {
#pragma clang fp contract(off)   // (the Welford update rounds as it is written)
  const int64_t g = blockIdx.x;
  const int lane = threadIdx.x;
  if (g >= st.G) return;
  const int64_t lo = st.offsets[g], R = st.offsets[g + 1] - lo;
  const int64_t a = st.counter[g];
  const double* T = st.temps + lo;
  // the energy of every replica that has not failed joins the statistics of the temperature it holds NOW
  for (int64_t k = lane; k < R; k += kWave) {
    const int32_t r = st.holder[lo + k];
    st.scale[r] = 1.0;
    const double e = (double)energies[r];
    if ((flags[r] & M3G_DYN_ERROR) || !std::isfinite(e)) continue;
    const int64_t n = st.count[lo + k] + 1;
    const double d = e - st.mean[lo + k];
    const double mean = st.mean[lo + k] + d / (double)n;
    st.count[lo + k] = n;
    st.mean[lo + k] = mean;
    st.m2[lo + k] += d * (e - mean);
  }
  __syncthreads();
  for (int64_t k = (a & 1) + 2 * (int64_t)lane; k + 1 < R; k += 2 * kWave) {
    const int32_t i = st.holder[lo + k], j = st.holder[lo + k + 1];
    const double ei = (double)energies[i], ej = (double)energies[j];
    if (((flags[i] | flags[j]) & (M3G_DYN_ERROR | M3G_DYN_STARTED)) || !std::isfinite(ei) || !std::isfinite(ej)) continue;   // not attempted
    const double delta = (1.0 / (kBoltzmann * T[k]) - 1.0 / (kBoltzmann * T[k + 1])) * (ei - ej);
    bool accept = delta >= 0.0;
    if (!accept) {
      uint64_t c[4] = {(uint64_t)a, (uint64_t)k, 0, 0};
      philox4x64_10(c, st.seed[g], 1);   // key word 1: disjoint from the Langevin draws (seed, 0)
      accept = uniform53(c[0]) < exp(delta);
    }
    st.attempts[lo + k] += 1;
    if (!accept) continue;
    st.accepts[lo + k] += 1;
    st.held[i] = (int32_t)(k + 1);
    st.held[j] = (int32_t)k;
    st.holder[lo + k] = j;
    st.holder[lo + k + 1] = i;
    t0[i] = T[k + 1];
    t0[j] = T[k];
    st.scale[i] = sqrt(T[k + 1] / T[k]);
    st.scale[j] = sqrt(T[k] / T[k + 1]);
  }
  __syncthreads();
  for (int64_t r = lo + lane; r < lo + R; r += kWave) {
    const int32_t h = st.held[r];
    if (h == 0) {
      if (st.label[r] == kDown) st.trips[r] += 1;
      st.label[r] = kUp;
    } else if (h == R - 1 && st.label[r] == kUp) {
      st.label[r] = kDown;
    }
    if (history && a < history_rows) history[a * st.S + r] = h;
  }
  if (lane == 0) st.counter[g] = a + 1;
}

__global__ void __launch_bounds__(kChunkRows) k_remd_rescale(DynView dyn, const double* __restrict__ scale) {
  const int c = blockIdx.x;
  if (c >= dyn.ch.n_chunks()) return;
  const int s = dyn.ch.structure(c);
  const double sc = scale[s];
  if (sc == 1.0) return;   // bitwise untouched
  const int64_t i = dyn.ch.row(c, threadIdx.x);
  if (!dyn.ch.holds(s, i)) return;
  for (int k = 0; k < 3; ++k) dyn.v[3 * i + k] *= sc;
}

bool remd_sizes_ok(int64_t S, int64_t G) { return G >= 1 && S >= 2 && 2 * G <= S && S <= INT32_MAX; }   // every ladder holds two replicas
}  // namespace
}  // namespace m3g

using namespace m3g;

extern "C" int m3g_remd_state_bytes(int64_t n_structs, int64_t n_ladders, size_t* bytes) {
  if (!bytes || !remd_sizes_ok(n_structs, n_ladders)) { set_error("m3g_remd_state_bytes: null argument or bad sizes"); return M3G_ERR_VALUE; }
  *bytes = remd_view(n_structs, n_ladders, nullptr).bytes;
  return M3G_OK;
}

extern "C" int m3g_remd_target_view(int64_t n_atoms, int64_t n_structs, size_t* temperature_offset) {
  if (!temperature_offset || !batch_sizes_ok(n_atoms, n_structs)) { set_error("m3g_remd_target_view: null argument or bad sizes"); return M3G_ERR_VALUE; }
  *temperature_offset = carve_offset(dyn_view(n_atoms, n_structs, nullptr).view.t0);   // (over a null state: the offset)
  return M3G_OK;
}

extern "C" int m3g_remd_init(int64_t n_structs, int64_t n_ladders, const int64_t* host_ladder_offsets, const double* host_temperatures,
                             const uint64_t* host_seeds, void* state, size_t state_bytes, void* stream_) {
  const int64_t S = n_structs, G = n_ladders;
  if (!remd_sizes_ok(S, G) || !host_ladder_offsets || !host_temperatures || !host_seeds || !state) {
    set_error("m3g_remd_init: null argument or bad sizes");
    return M3G_ERR_VALUE;
  }
  if (!offsets_ok("m3g_remd_init", host_ladder_offsets, S, G, "ladder_offsets", "n_structs")) return M3G_ERR_VALUE;
  for (int64_t g = 0; g < G; ++g) {
    const int64_t lo = host_ladder_offsets[g], hi = host_ladder_offsets[g + 1];
    if (hi - lo < 2) { set_error("m3g_remd_init: ladder %lld holds fewer than 2 replicas", (long long)g); return M3G_ERR_VALUE; }
    for (int64_t r = lo; r < hi; ++r)
      if (!finite_positive(host_temperatures[r]) || (r > lo && host_temperatures[r] <= host_temperatures[r - 1])) {
        set_error("m3g_remd_init: the temperatures of ladder %lld must be finite, > 0 and strictly ascending", (long long)g);
        return M3G_ERR_VALUE;
      }
  }
  const size_t total = remd_view(S, G, nullptr).bytes;
  if (!state_fits("m3g_remd_init", state_bytes, total, true)) return M3G_ERR_SIZE;
  std::vector<char> image(total, 0);   // counts, means, accepts and the attempt counters start at zero
  const RemdView im = remd_view(S, G, image.data()).view;
  std::memcpy((void*)im.offsets, host_ladder_offsets, 8 * (G + 1));
  std::memcpy((void*)im.temps, host_temperatures, 8 * S);
  std::memcpy((void*)im.seed, host_seeds, 8 * G);
  for (int64_t g = 0; g < G; ++g)
    for (int64_t lo = host_ladder_offsets[g], r = lo; r < host_ladder_offsets[g + 1]; ++r) {
      im.held[r] = (int32_t)(r - lo);
      im.holder[r] = (int32_t)r;
      im.label[r] = r == lo ? kUp : 0;
      im.scale[r] = 1.0;
    }
  hipStream_t s = (hipStream_t)stream_;
  M3G_HIP_CHECK(hipMemcpyAsync(state, image.data(), total, hipMemcpyHostToDevice, s));
  M3G_HIP_CHECK(hipStreamSynchronize(s));   // (the host image above goes out of scope)
  return M3G_OK;
}

extern "C" int m3g_remd_exchange(int64_t n_atoms, int64_t n_structs, int64_t n_ladders, void* remd_state, size_t remd_bytes, void* dyn_state,
                                 size_t dyn_bytes, const float* energies, int32_t* history, int64_t history_rows, void* stream_) {
  const int64_t N = n_atoms, S = n_structs, G = n_ladders;
  if (!batch_sizes_ok(N, S) || !remd_sizes_ok(S, G) || !remd_state || !dyn_state || !energies || history_rows < 0) {
    set_error("m3g_remd_exchange: null argument or bad sizes");
    return M3G_ERR_VALUE;
  }
  const auto [st, remd_total] = remd_view(S, G, remd_state);
  const auto [dyn, dyn_total] = dyn_view(N, S, dyn_state);
  if (!state_fits("m3g_remd_exchange", remd_bytes, remd_total, false, "replica-exchange")) return M3G_ERR_SIZE;
  if (!state_fits("m3g_remd_exchange", dyn_bytes, dyn_total, false, "dynamics")) return M3G_ERR_SIZE;
  hipStream_t s = (hipStream_t)stream_;
  hipLaunchKernelGGL(k_remd_decide, dim3((unsigned)G), dim3(kWave), 0, s, st, dyn.t0, dyn.flags, energies, history, history_rows);
  hipLaunchKernelGGL(k_remd_rescale, dim3((unsigned)chunk_bound(N, S)), dim3(kChunkRows), 0, s, dyn, st.scale);
  M3G_RETURN_LAUNCH_STATUS();
}

extern "C" int m3g_remd_read(int64_t n_structs, int64_t n_ladders, const void* state, size_t state_bytes, int32_t* host_held,
                             int32_t* host_holder, int64_t* host_attempts, int64_t* host_accepts, int64_t* host_count, double* host_mean,
                             double* host_m2, int64_t* host_round_trips, int64_t* host_counters, void* stream_) {
  const int64_t S = n_structs, G = n_ladders;
  if (!remd_sizes_ok(S, G) || !state) { set_error("m3g_remd_read: null argument or bad sizes"); return M3G_ERR_VALUE; }
  const auto [st, total] = remd_view(S, G, (void*)state);
  if (!state_fits("m3g_remd_read", state_bytes, total)) return M3G_ERR_SIZE;
  return read_all((hipStream_t)stream_,
                  {rb(host_held, st.held, S), rb(host_holder, st.holder, S), rb(host_attempts, st.attempts, S), rb(host_accepts, st.accepts, S),
                   rb(host_count, st.count, S), rb(host_mean, st.mean, S), rb(host_m2, st.m2, S), rb(host_round_trips, st.trips, S),
                   rb(host_counters, st.counter, G)});
}
