// Thermodynamic fluctuation observables of a batch, accumulated on the device while it is integrated (or fed any samples): per
// structure the running mean and the Welford co-moments of the row x = (e_pot, ke, V, h, p, Green-Lagrange strain [6]) and, over a ring
// of the last n_lags pressure tensors, the lag sums behind the Green-Kubo viscosities.  Definitions: include/m3gnet_hip.h.  One
// m3g_thermo_sample is, over the chunk table of m3g_chunks.h:
//   k_thermo_partials  (mode (a): velocities given) one workgroup per chunk: every row's mass, velocity and force read once (44 B per
//                      atom: memory-bound), the full-step velocity v + kick kappa F / m, and the chunk's sums of m v_a v_b [6], m,
//                      m v [3] and the count of non-finite rows in the fixed tree order;
//   k_thermo_finalize  one wave per structure, kFinalizeWaves to a workgroup: the chunk partials in chunk order (wave_chunk_sum, every
//                      lane ends with the same bits), the row and the tensor -- formed by every lane alike from the same numbers, so
//                      nothing has to be handed from lane 0 to the others --, then the lanes stride over the 66 co-moments and over
//                      the lags of the ring; lane 0 stores what is per structure.
// Mode (b) (kinetic energy and pressure tensor read from an integrator's obs row) is the second launch alone.  No float atomics:
// every number depends on the structure's own rows only, so it is bitwise the same alone or in any batch.  Ring position, ring
// fill and all counts live in the state buffer and each is read and written by its structure's wave only, hence no allocation, copy
// or wait in m3g_thermo_sample: capture-safe.
#include <cmath>

#include "m3g_chunks.h"
#include "m3g_internal.h"

namespace m3g {
namespace {
constexpr int kRow = M3G_THERMO_ROW, kCo = M3G_THERMO_COMOMENTS, kTen = M3G_THERMO_TENSOR;
constexpr int kMaxLags = M3G_THERMO_MAX_LAGS;
constexpr int kPart = 11;   // per chunk: sum m v_a v_b (xx, yy, zz, yz, zx, xy), sum m, sum m v [3], non-finite rows
enum { kDone = 0, kCounters = 2 };   // int64 words: samples taken (skipped ones included)
static_assert(kCo == kRow * (kRow + 1) / 2, "the upper triangle of the row");

struct ThermoView {
  int64_t N;
  int32_t G;
  ChunkView ch;
  const double *mass, *p_ext, *ref_inv;
  int64_t* ctr;
  int32_t* flags;
  int64_t *n_samples, *n_skipped;
  int32_t *ring_fill, *ring_pos;
  double *mean, *comoment, *last_row;
  double *lag_uu, *lag_now, *lag_old;
  int64_t* lag_count;
  double* ring;      // [S][G][kTen]
  double* partial;   // [chunk][kPart]
};
Carved<ThermoView> thermo_view(const m3g_thermo_sizes& z, void* state) {
  const int64_t N = z.n_atoms, S = z.n_structs, G = z.n_lags;
  Carve c{state};
  ThermoView st{N, z.n_lags};
  st.ch = chunk_view(N, S, c);
  st.mass = c.take<double>(N);
  st.p_ext = c.take<double>(S);
  st.ref_inv = c.take<double>(9 * S);
  st.ctr = c.take<int64_t>(kCounters);   // the accumulators from here up to `partial` are cleared by the init call
  st.flags = c.take<int32_t>(S);
  st.n_samples = c.take<int64_t>(S);
  st.n_skipped = c.take<int64_t>(S);
  st.ring_fill = c.take<int32_t>(S);
  st.ring_pos = c.take<int32_t>(S);
  st.mean = c.take<double>(kRow * S);
  st.comoment = c.take<double>(kCo * S);
  st.last_row = c.take<double>(kRow * S);
  st.lag_uu = c.take<double>(kTen * G * S);
  st.lag_now = c.take<double>(kTen * G * S);
  st.lag_old = c.take<double>(kTen * G * S);
  st.lag_count = c.take<int64_t>(G * S);
  st.ring = c.take<double>(kTen * G * S);
  st.partial = c.take<double>(kPart * chunk_bound(N, S));
  return {st, c.off};
}

__global__ void __launch_bounds__(kChunkRows) k_thermo_partials(ThermoView st, const double* __restrict__ vel, const float* __restrict__ forces,
                                                                 double kick) {
  __shared__ double sh[kPart][kChunkRows];
  const int c = blockIdx.x, t = threadIdx.x;
  if (c >= st.ch.n_chunks()) return;
  const int s = st.ch.structure(c);
  const int64_t i = st.ch.row(c, t);
  double val[kPart] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (st.ch.holds(s, i)) {
    const double m = st.mass[i];
    double v[3];
    for (int k = 0; k < 3; ++k) {
      v[k] = vel[3 * i + k];
      if (forces) v[k] += kick * (kKappa * (double)forces[3 * i + k] / m);   // the finish kick, as sampled_row spells it
    }
    const double mv[3] = {m * v[0], m * v[1], m * v[2]};
    val[0] = mv[0] * v[0];
    val[1] = mv[1] * v[1];
    val[2] = mv[2] * v[2];
    val[3] = mv[1] * v[2];
    val[4] = mv[2] * v[0];
    val[5] = mv[0] * v[1];
    val[6] = m;
    for (int k = 0; k < 3; ++k) val[7 + k] = mv[k];
    val[10] = (std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2])) ? 0.0 : 1.0;
  }
  chunk_tree_reduce<kPart>(sh, val, t);
  if (t < kPart) st.partial[kPart * c + t] = sh[t][0];
}

// The sums of one lag of one structure and the ring entry they pair the new tensor with, read (lag_load) and written back with the
// new tensor u in (lag_store).  Lag l > 0 never names the slot `pos` that the same launch writes: 0 < l < G.
struct Lag { double old[kTen], uu[kTen], now[kTen], od[kTen]; int64_t count; };
__device__ inline void lag_load(const ThermoView& st, int64_t s, int pos, int l, Lag& g) {
  const int G = st.G;
  const double* entry = st.ring + ((size_t)s * G + (size_t)((pos - l + G) % G)) * kTen;
  const size_t at = ((size_t)s * G + l) * kTen;
#pragma unroll
  for (int c = 0; c < kTen; ++c) {
    g.old[c] = l == 0 ? 0.0 : entry[c];
    g.uu[c] = st.lag_uu[at + c];
    g.now[c] = st.lag_now[at + c];
    g.od[c] = st.lag_old[at + c];
  }
  g.count = st.lag_count[(size_t)s * G + l];
}
__device__ inline void lag_store(const ThermoView& st, int64_t s, int l, const Lag& g, const double (&u)[kTen]) {
  const size_t at = ((size_t)s * st.G + l) * kTen;
#pragma unroll
  for (int c = 0; c < kTen; ++c) {
    const double o = l == 0 ? u[c] : g.old[c];
    st.lag_uu[at + c] = g.uu[c] + u[c] * o;
    st.lag_now[at + c] = g.now[c] + u[c];
    st.lag_old[at + c] = g.od[c] + o;
  }
  st.lag_count[(size_t)s * st.G + l] = g.count + 1;
}
// the row-major upper triangle of the row: where row i begins, and the row that holds entry `at`
__device__ inline int triangle_at(int i) { return i * kRow - i * (i - 1) / 2; }
__device__ inline int triangle_row(int at) {
  int i = 0;
#pragma unroll
  for (int k = 1; k < kRow; ++k) i += at >= triangle_at(k) ? 1 : 0;
  return i;
}
// a[k] without indexing registers by a variable (a sum of one entry and ten zeros: a chain of selects is turned back into an indexed
// load from scratch)
__device__ inline double pick(const double (&a)[kRow], int k) {
  double r = 0.0;
#pragma unroll
  for (int i = 0; i < kRow; ++i) r += k == i ? a[i] : 0.0;
  return r;
}

// kVel: mode (a), the kinetic tensor from the chunk partials; else mode (b), ke and (where given) the tensor from the caller's rows
template <bool kVel>
__global__ void __launch_bounds__(kWave* kFinalizeWaves) k_thermo_finalize(ThermoView st, int32_t remove_com, const float* __restrict__ energies,
                                                                            const float* __restrict__ stresses,
                                                                            const double* __restrict__ lattice,
                                                                            const double* __restrict__ kinetic, int64_t kinetic_stride,
                                                                            const double* __restrict__ tensor, int64_t tensor_stride) {
  const int lane = threadIdx.x % kWave;
  const int64_t s = (int64_t)blockIdx.x * kFinalizeWaves + threadIdx.x / kWave;
  if (s >= st.ch.S) return;   // (whole waves: s is uniform across a wave)
  const int G = st.G;
  const bool has_u = kVel || tensor != nullptr;

  // ---- what the wave will update, read first: no load below has to queue behind a store (a round trip each, one after the other) ----
  // lane k keeps co-moment k, lanes 0 and 1 also 64 and 65; (i, j) of a co-moment from its place in the row-major upper triangle
  static_assert(kCo > kWave && kCo <= 2 * kWave, "one or two co-moments per lane");
  double* C = st.comoment + kCo * s;
  const bool second = lane + kWave < kCo;
  const int i0 = triangle_row(lane), j0 = i0 + (lane - triangle_at(i0));
  const int i1 = triangle_row((lane + kWave) % kCo), j1 = i1 + ((lane + kWave) % kCo - triangle_at(i1));
  const double c0 = C[lane], c1 = second ? C[lane + kWave] : 0.0;
  const int64_t n_new = st.n_samples[s] + 1;
  double mean[kRow];
  for (int i = 0; i < kRow; ++i) mean[i] = st.mean[kRow * s + i];
  int fill = 0, pos = 0;
  if (G > 0) {
    fill = st.ring_fill[s];
    pos = st.ring_pos[s];
    fill = fill < G ? fill + 1 : G;   // entries once u is in
  }
  double* ring = st.ring + (size_t)s * G * kTen;
  // the sums of lag l = lane (the later ones, lane + 64, ...: one at a time below)
  Lag first;
  if (lane < fill) lag_load(st, s, pos, lane, first);

  // ---- the row and the tensor: every lane, the same bits ---------------------------------------------------------------------------
  double x[kRow], u[kTen] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  bool bad = false;
  const double* L = lattice + 9 * s;
  const float* sv = stresses + 6 * s;
  const double vol = fabs(L[0] * (L[4] * L[8] - L[5] * L[7]) - L[1] * (L[3] * L[8] - L[5] * L[6]) + L[2] * (L[3] * L[7] - L[4] * L[6]));
  double ke, p;
  if constexpr (kVel) {
    double acc[kPart];
    wave_chunk_sum<kPart>(st.ch, s, st.partial, lane, acc);
    bad = acc[10] != 0.0;
    double K[6];
    for (int c = 0; c < 6; ++c) K[c] = acc[c];
    if (remove_com) {
      const double q[3] = {acc[7], acc[8], acc[9]}, m = acc[6];
      K[0] -= q[0] * q[0] / m;
      K[1] -= q[1] * q[1] / m;
      K[2] -= q[2] * q[2] / m;
      K[3] -= q[1] * q[2] / m;
      K[4] -= q[2] * q[0] / m;
      K[5] -= q[0] * q[1] / m;
    }
    for (int c = 0; c < 6; ++c) K[c] = K[c] / kKappa;
    ke = ((K[0] + K[1]) + K[2]) / 2.0;
    for (int c = 0; c < 6; ++c) u[c] = (double)sv[c] + K[c] / vol;
    p = ((u[0] + u[1]) + u[2]) / 3.0;
  } else {
    ke = kinetic[s * kinetic_stride];
    if (tensor) {
      for (int c = 0; c < 6; ++c) u[c] = tensor[s * tensor_stride + c];
      p = ((u[0] + u[1]) + u[2]) / 3.0;
    } else {
      const double trw = vol * (((double)sv[0] + (double)sv[1]) + (double)sv[2]), k2 = 2.0 * ke;
      p = (trw + k2) / (3.0 * vol);   // the pressure of m3g_nhc_step, in its own words
    }
  }
  u[6] = p;
  x[0] = (double)energies[s];
  x[1] = ke;
  x[2] = vol;
  x[3] = (x[0] + ke) + st.p_ext[s] * vol;
  x[4] = p;
  {
    const double* R = st.ref_inv + 9 * s;
    double A[9];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) A[3 * i + j] = R[3 * i] * L[j] + R[3 * i + 1] * L[3 + j] + R[3 * i + 2] * L[6 + j];
    auto dot = [&](int i, int j) { return A[3 * i] * A[3 * j] + A[3 * i + 1] * A[3 * j + 1] + A[3 * i + 2] * A[3 * j + 2]; };
    x[5] = 0.5 * (dot(0, 0) - 1.0);
    x[6] = 0.5 * (dot(1, 1) - 1.0);
    x[7] = 0.5 * (dot(2, 2) - 1.0);
    x[8] = 0.5 * dot(1, 2);
    x[9] = 0.5 * dot(2, 0);
    x[10] = 0.5 * dot(0, 1);
  }
  for (int i = 0; i < kRow; ++i) bad = bad || !std::isfinite(x[i]);
  if (has_u)
    for (int c = 0; c < kTen; ++c) bad = bad || !std::isfinite(u[c]);

  // ---- from here on: stores ----------------------------------------------------------------------------------------------------------
  if (s == 0 && lane == 0) st.ctr[kDone] += 1;   // (read by the host only)
  if (lane == 0)
    for (int i = 0; i < kRow; ++i) st.last_row[kRow * s + i] = x[i];
  if (bad) {   // enters nothing; no lag may span the gap
    if (lane == 0) {
      st.flags[s] |= M3G_THERMO_NONFINITE;
      st.n_skipped[s] += 1;
      st.ring_fill[s] = 0;
    }
    return;
  }

  // Welford: d = x - mean; mean += d / n; C_ij += d_i (x_j - mean_j) with the new mean
  const double n = (double)n_new;
  double d[kRow], e[kRow], mean_new[kRow];
  for (int i = 0; i < kRow; ++i) {
    d[i] = x[i] - mean[i];
    mean_new[i] = mean[i] + d[i] / n;
    e[i] = x[i] - mean_new[i];
  }
  C[lane] = c0 + pick(d, i0) * pick(e, j0);
  if (second) C[lane + kWave] = c1 + pick(d, i1) * pick(e, j1);

  // the ring and the lag sums: lane l, l + 64, ... takes lag l
  if (lane < fill) lag_store(st, s, lane, first, u);
  for (int l = lane + kWave; l < fill; l += kWave) {
    Lag g;
    lag_load(st, s, pos, l, g);
    lag_store(st, s, l, g, u);
  }
  if (lane == 0) {
    for (int c = 0; c < kTen && G > 0; ++c) ring[(size_t)pos * kTen + c] = u[c];
    for (int i = 0; i < kRow; ++i) st.mean[kRow * s + i] = mean_new[i];
    st.n_samples[s] = n_new;
    if (G > 0) {
      st.ring_fill[s] = fill;
      st.ring_pos[s] = (pos + 1) % G;
    }
  }
}

// nullptr when the sizes (and, where given, the parameters) are valid, else what is wrong with them
const char* thermo_error(const m3g_thermo_sizes* z, const m3g_thermo_params* p, bool with_params) {
  if (!z || (with_params && !p)) return "null sizes or parameters";
  if (!batch32_sizes_ok(z->n_atoms, z->n_structs)) return "bad sizes";
  if (z->n_lags < 0 || z->n_lags > kMaxLags) return "n_lags must be 0 .. 4096";
  if (with_params && p->remove_com != 0 && p->remove_com != 1) return "remove_com must be 0 or 1";
  return nullptr;
}
}  // namespace
}  // namespace m3g

using namespace m3g;

extern "C" int m3g_thermo_state_bytes(const m3g_thermo_sizes* sizes, size_t* bytes) {
  if (const char* why = thermo_error(sizes, nullptr, false)) { set_error("m3g_thermo_state_bytes: %s", why); return M3G_ERR_VALUE; }
  if (!bytes) { set_error("m3g_thermo_state_bytes: null argument"); return M3G_ERR_VALUE; }
  *bytes = thermo_view(*sizes, nullptr).bytes;
  return M3G_OK;
}

extern "C" int m3g_thermo_init(const m3g_thermo_sizes* sizes, const m3g_thermo_params* params, const int64_t* host_offsets,
                               const double* host_masses, const double* host_p_ext, const double* host_reference_cells, void* state,
                               size_t state_bytes, void* stream_) {
  constexpr const char* fn = "m3g_thermo_init";
  if (const char* why = thermo_error(sizes, params, true)) { set_error("%s: %s", fn, why); return M3G_ERR_VALUE; }
  if (!host_offsets || !host_masses || !host_p_ext || !host_reference_cells || !state) { set_error("%s: null argument", fn); return M3G_ERR_VALUE; }
  const int64_t N = sizes->n_atoms, S = sizes->n_structs;
  if (!offsets_ok(fn, host_offsets, N, S)) return M3G_ERR_VALUE;
  for (int64_t i = 0; i < N; ++i)
    if (!mass_ok(fn, host_masses, i)) return M3G_ERR_VALUE;
  std::vector<double> ref_inv(9 * S);
  for (int64_t s = 0; s < S; ++s) {
    if (!std::isfinite(host_p_ext[s])) { set_error("%s: p_ext of structure %lld is not finite", fn, (long long)s); return M3G_ERR_VALUE; }
    if (!lattice_ok(fn, host_reference_cells + 9 * s, s)) return M3G_ERR_VALUE;
    inv3(host_reference_cells + 9 * s, ref_inv.data() + 9 * s);
  }
  const auto [st, total] = thermo_view(*sizes, state);
  if (!state_fits(fn, state_bytes, total, true)) return M3G_ERR_SIZE;
  const ChunkTable table(host_offsets, S);
  hipStream_t s = (hipStream_t)stream_;
  if (int rc = table.upload(st.ch, host_offsets, s)) return rc;
  M3G_HIP_CHECK(hipMemcpyAsync((void*)st.mass, host_masses, 8 * N, hipMemcpyHostToDevice, s));
  M3G_HIP_CHECK(hipMemcpyAsync((void*)st.p_ext, host_p_ext, 8 * S, hipMemcpyHostToDevice, s));
  M3G_HIP_CHECK(hipMemcpyAsync((void*)st.ref_inv, ref_inv.data(), 72 * S, hipMemcpyHostToDevice, s));
  M3G_HIP_CHECK(hipMemsetAsync(st.ctr, 0, (size_t)((const char*)st.partial - (const char*)st.ctr), s));
  M3G_HIP_CHECK(hipStreamSynchronize(s));   // (the host tables above go out of scope)
  return M3G_OK;
}

extern "C" int m3g_thermo_sample(const m3g_thermo_sizes* sizes, const m3g_thermo_params* params, void* state, size_t state_bytes,
                                 const float* energies, const float* stresses, const double* lattice, const double* vel, const float* forces,
                                 double kick, const double* kinetic, int64_t kinetic_stride, const double* pressure_tensor,
                                 int64_t tensor_stride, void* stream_) {
  constexpr const char* fn = "m3g_thermo_sample";
  if (const char* why = thermo_error(sizes, params, true)) { set_error("%s: %s", fn, why); return M3G_ERR_VALUE; }
  if (!state || !energies || !stresses || !lattice) { set_error("%s: null argument", fn); return M3G_ERR_VALUE; }
  if ((vel != nullptr) == (kinetic != nullptr)) { set_error("%s: exactly one of vel and kinetic must be given", fn); return M3G_ERR_VALUE; }
  if (vel) {
    if (pressure_tensor) { set_error("%s: pressure_tensor goes with kinetic, not with vel", fn); return M3G_ERR_VALUE; }
    if (forces && !std::isfinite(kick)) { set_error("%s: kick must be finite", fn); return M3G_ERR_VALUE; }
  } else {
    if (forces) { set_error("%s: forces go with vel, not with kinetic", fn); return M3G_ERR_VALUE; }
    if (kinetic_stride < 1) { set_error("%s: kinetic_stride must be >= 1", fn); return M3G_ERR_VALUE; }
    if (pressure_tensor && tensor_stride < 6) { set_error("%s: tensor_stride must be >= 6", fn); return M3G_ERR_VALUE; }
    if (!pressure_tensor && sizes->n_lags > 0) {
      set_error("%s: n_lags > 0 needs the pressure tensor (vel, or pressure_tensor beside kinetic)", fn);
      return M3G_ERR_VALUE;
    }
  }
  const auto [st, total] = thermo_view(*sizes, state);
  if (!state_fits(fn, state_bytes, total)) return M3G_ERR_SIZE;
  const int64_t N = sizes->n_atoms, S = sizes->n_structs;
  hipStream_t s = (hipStream_t)stream_;
  const auto sv = st;   // (a structured binding cannot be captured)
  const dim3 waves = grid_for(S, kFinalizeWaves), lanes(kWave * kFinalizeWaves);
  if (vel) {   // workgroups beyond the table's chunk count return at once
    hipLaunchKernelGGL(k_thermo_partials, dim3((unsigned)chunk_bound(N, S)), dim3(kChunkRows), 0, s, sv, vel, forces, kick);
    hipLaunchKernelGGL(k_thermo_finalize<true>, waves, lanes, 0, s, sv, params->remove_com, energies, stresses, lattice, nullptr, (int64_t)0,
                       nullptr, (int64_t)0);
  } else {
    hipLaunchKernelGGL(k_thermo_finalize<false>, waves, lanes, 0, s, sv, 0, energies, stresses, lattice, kinetic, kinetic_stride,
                       pressure_tensor, tensor_stride);
  }
  M3G_RETURN_LAUNCH_STATUS();
}

extern "C" int m3g_thermo_read(const m3g_thermo_sizes* sizes, const void* state, size_t state_bytes, double* host_mean, double* host_comoments,
                               double* host_lag_uu, double* host_lag_now, double* host_lag_old, int64_t* host_lag_count,
                               int64_t* host_n_samples, int64_t* host_n_skipped, int32_t* host_flags, void* stream_) {
  if (const char* why = thermo_error(sizes, nullptr, false)) { set_error("m3g_thermo_read: %s", why); return M3G_ERR_VALUE; }
  if (!state) { set_error("m3g_thermo_read: null argument"); return M3G_ERR_VALUE; }
  const auto [st, total] = thermo_view(*sizes, (void*)state);
  if (!state_fits("m3g_thermo_read", state_bytes, total)) return M3G_ERR_SIZE;
  const size_t S = sizes->n_structs, G = sizes->n_lags;
  return read_all((hipStream_t)stream_,
                  {rb(host_mean, (const double*)st.mean, S * kRow), rb(host_comoments, (const double*)st.comoment, S * kCo),
                   rb(host_lag_uu, (const double*)st.lag_uu, S * G * kTen), rb(host_lag_now, (const double*)st.lag_now, S * G * kTen),
                   rb(host_lag_old, (const double*)st.lag_old, S * G * kTen), rb(host_lag_count, (const int64_t*)st.lag_count, S * G),
                   rb(host_n_samples, (const int64_t*)st.n_samples, S), rb(host_n_skipped, (const int64_t*)st.n_skipped, S),
                   rb(host_flags, (const int32_t*)st.flags, S)});
}

extern "C" int m3g_thermo_frame(const m3g_thermo_sizes* sizes, const void* state, size_t state_bytes, int32_t lag, double* host_row,
                                double* host_tensor, void* stream_) {
  constexpr const char* fn = "m3g_thermo_frame";
  if (const char* why = thermo_error(sizes, nullptr, false)) { set_error("%s: %s", fn, why); return M3G_ERR_VALUE; }
  if (!state) { set_error("%s: null argument", fn); return M3G_ERR_VALUE; }
  const int64_t S = sizes->n_structs, G = sizes->n_lags;
  if (host_tensor && (lag < 0 || lag >= G)) { set_error("%s: no ring entry %d samples back (n_lags = %d)", fn, (int)lag, (int)G); return M3G_ERR_VALUE; }
  const auto [st, total] = thermo_view(*sizes, (void*)state);
  if (!state_fits(fn, state_bytes, total)) return M3G_ERR_SIZE;
  hipStream_t s = (hipStream_t)stream_;
  int64_t ctr[kCounters];
  M3G_HIP_CHECK(hipMemcpyAsync(ctr, st.ctr, sizeof(ctr), hipMemcpyDeviceToHost, s));
  M3G_HIP_CHECK(hipStreamSynchronize(s));
  if (ctr[kDone] < 1) { set_error("%s: no sample has been taken", fn); return M3G_ERR_VALUE; }
  if (!host_tensor) return read_all(s, {rb(host_row, (const double*)st.last_row, (size_t)S * kRow)});
  std::vector<double> ring((size_t)S * G * kTen);
  std::vector<int32_t> fill(S), pos(S);
  if (int rc = read_all(s, {rb(host_row, (const double*)st.last_row, (size_t)S * kRow), rb(ring.data(), (const double*)st.ring, ring.size()),
                            rb(fill.data(), (const int32_t*)st.ring_fill, (size_t)S), rb(pos.data(), (const int32_t*)st.ring_pos, (size_t)S)}))
    return rc;
  for (int64_t k = 0; k < S; ++k)
    for (int c = 0; c < kTen; ++c)   // (ring_pos is the slot the NEXT sample takes)
      host_tensor[kTen * k + c] = lag < fill[k] ? ring[((size_t)k * G + (size_t)((pos[k] - 1 - lag + 2 * G) % G)) * kTen + c] : NAN;
  return M3G_OK;
}
