// Batched thermodynamic integration to an Einstein crystal (Frenkel, Ladd, J. Chem. Phys. 81, 3188 (1984)), at fixed coupling or by
// non-equilibrium switching (Freitas, Asta, de Koning, Comput. Mater. Sci. 112, 333 (2016)).  A fifth MD family beside
// m3g_dynamics.hip, m3g_nhc.hip, m3g_mtk.hip and m3g_pimd.hip, on the same layers (the chunk table of m3g_chunks.h, the constants and
// the generator of m3g_dyn_state.h).  Every structure moves under H(lambda) = KE + lambda E_model(x) + (1 - lambda) U_s(x),
// U_s = 1/2 sum_i k_i |x_i - r0_i|^2, by BAOAB Langevin dynamics whose CENTRE OF MASS IS HELD: the force on atom i is
// G_i - (m_i / M) sum_j G_j with G_i = lambda F_i - (1 - lambda) k_i (x_i - r0_i), and the O step takes the momentum its noise would
// add, pbar = sum_j m_j sigma_j xi_j, out again: v_i <- c1 v_i + sigma_i xi_i - pbar / M.  lambda follows the structure's path
// (lambda_b, lambda_e, n_switch) by its step index c; the work W = int D dlambda, D = dH/dlambda = E - U_s, is summed by the
// trapezoid rule, D goes through Welford's accumulators and |x_i - r0_i|^2 into per-atom sums once c >= n_discard.
// One call -- finish step k, observables, start step k+1 -- is three launches for the whole batch, as m3g_dyn_step:
//   k_ti_partials  one workgroup per chunk: the finish kick by the UNCONSTRAINED force in registers, then the chunk sums of m |w|^2,
//                  m w, G, k |u|^2, the momentum m sigma xi of the COMING O step (Philox is counter-based: k_ti_apply draws the same
//                  numbers again) and the non-finite count, in a fixed tree order;
//   k_ti_finalize  one wave per structure: the chunk partials in chunk order, the error verdict, lambda, the kinetic energy in closed
//                  form sum m |w - d|^2 = sum m |w|^2 - 2 d . sum m w + M |d|^2 with d = h kappa sum G / M -- no second pass over
//                  the atoms --, the work, the accumulators, the observables and the coefficients of the apply;
//   k_ti_apply     one workgroup per chunk: the finish kick and B A O A of every atom by the constrained force.
// No atomics: every result depends on the structure's own rows only, so it is bitwise the same alone or in any batch.  No allocation,
// copy or wait in m3g_ti_step (capture-safe).  The Box-Muller draw and its key word, the epilogue of the partials and the checks and
// copies of the entry points are m3g_integrator.h.
#include <cmath>
#include <vector>

#include "m3g_integrator.h"

namespace m3g {
namespace {
constexpr int kTiPart = 12;   // per chunk: sum m |w|^2, sum m w [3], sum G [3], sum k |u|^2, sum m sigma xi [3], non-finite forces
constexpr int kTiCoef = 12;   // per structure: action, finish kick?, lambda, sum G / M [3], pbar / M [3], sample?, noise^2, unused
enum TiPath : int { kPathSwitch = 0, kPathDiscard = 1, kPathIndex = 2, kPathWords = 3 };   // per structure: n_switch, n_discard, c

struct TiView {
  int64_t N;
  ChunkView ch;
  double *partial, *mass, *v, *ref, *spring, *msd, *t0, *mtot, *lam_b, *lam_e, *work, *lam_prev, *d_prev, *mean, *m2, *coef;
  uint64_t* seed;
  int64_t *steps, *count, *path;
  int32_t *flags, *has_prev;
};
inline Carved<TiView> ti_view(int64_t N, int64_t S, void* state) {
  Carve c{state};
  TiView st{N};
  st.ch = chunk_view(N, S, c);
  st.partial = c.take<double>(kTiPart * chunk_bound(N, S));
  st.mass = c.take<double>(N);
  st.v = c.take<double>(3 * N);
  st.ref = c.take<double>(3 * N);
  st.spring = c.take<double>(N);
  st.msd = c.take<double>(N);
  st.t0 = c.take<double>(S);
  st.mtot = c.take<double>(S);
  st.lam_b = c.take<double>(S);
  st.lam_e = c.take<double>(S);
  st.work = c.take<double>(S);
  st.lam_prev = c.take<double>(S);
  st.d_prev = c.take<double>(S);
  st.mean = c.take<double>(S);
  st.m2 = c.take<double>(S);
  st.coef = c.take<double>(kTiCoef * S);
  st.seed = c.take<uint64_t>(S);
  st.steps = c.take<int64_t>(S);
  st.count = c.take<int64_t>(S);
  st.path = c.take<int64_t>(kPathWords * S);
  st.flags = c.take<int32_t>(S);
  st.has_prev = c.take<int32_t>(S);
  return {st, c.off};
}

// lambda of structure s at its step index: lambda_b + (lambda_e - lambda_b) g(min(c, n_switch) / n_switch)
__device__ inline double path_lambda(const TiView& st, int64_t s, int32_t schedule) {
  const int64_t n = st.path[kPathWords * s + kPathSwitch], c = st.path[kPathWords * s + kPathIndex];
  const double lb = st.lam_b[s];
  if (n == 0) return lb;
  if (c >= n) return st.lam_e[s];   // (the end of the path to the bit: lambda = 1 is the model alone)
  const double t = (double)c / (double)n;
  double g = t;
  if (schedule == M3G_TI_SMOOTH) {
    const double t2 = t * t;
    g = t2 * t2 * t * (70.0 * t2 * t2 - 315.0 * t2 * t + 540.0 * t2 - 420.0 * t + 126.0);
  }
  return lb + (st.lam_e[s] - lb) * g;
}

// a new path for every structure that has not failed (k_ti_init: for all, with lambda = 1 throughout)
__global__ void __launch_bounds__(kChunkRows) k_ti_path(TiView st, int64_t n_switch, int64_t n_discard, int32_t init) {
  const int c = blockIdx.x, t = threadIdx.x;
  if (c >= st.ch.n_chunks()) return;
  const int s = st.ch.structure(c);
  if (!init && (st.flags[s] & M3G_DYN_ERROR)) return;   // failed: bitwise untouched
  const int64_t i = st.ch.row(c, t);
  if (st.ch.holds(s, i)) st.msd[i] = 0.0;
  if (t != 0 || c != st.ch.chunks_begin(s)) return;
  st.path[kPathWords * s + kPathSwitch] = n_switch;
  st.path[kPathWords * s + kPathDiscard] = n_discard;
  st.path[kPathWords * s + kPathIndex] = 0;
  st.work[s] = 0.0;
  st.lam_prev[s] = 0.0;
  st.d_prev[s] = 0.0;
  st.has_prev[s] = 0;
  st.count[s] = 0;
  st.mean[s] = 0.0;
  st.m2[s] = 0.0;
}

__global__ void __launch_bounds__(kChunkRows) k_ti_init(TiView st, const double* __restrict__ vel, const double* __restrict__ reference) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < 3 * st.N) {
    st.v[i] = vel[i];
    st.ref[i] = reference[i];
  }
  if (i < st.ch.S) {
    st.flags[i] = 0;
    st.steps[i] = 0;
    st.lam_b[i] = 1.0;
    st.lam_e[i] = 1.0;
    st.coef[kTiCoef * i] = 0.0;
  }
}

__global__ void __launch_bounds__(kChunkRows) k_ti_partials(TiView st, int32_t schedule, double half_dt, double c1, const float* __restrict__ forces,
                                                            const double* __restrict__ pos) {
  const int c = blockIdx.x, t = threadIdx.x;
  if (c >= st.ch.n_chunks()) return;
  const int s = st.ch.structure(c);
  const int fl = st.flags[s];
  if (fl & M3G_DYN_ERROR) return;   // frozen: finalize reads nothing of it
  const int64_t i = st.ch.row(c, t);
  double val[kTiPart] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (st.ch.holds(s, i)) {
    const double lam = path_lambda(st, s, schedule);
    const double m = st.mass[i], k = st.spring[i];
    double f[3], g[3], w[3], u2 = 0.0;
    for (int a = 0; a < 3; ++a) {
      f[a] = forces[3 * i + a];
      const double u = pos[3 * i + a] - st.ref[3 * i + a];
      u2 += u * u;
      g[a] = lam * f[a] - (1.0 - lam) * (k * u);
      w[a] = st.v[3 * i + a];
      if (fl & M3G_DYN_STARTED) w[a] += half_dt * (kKappa * g[a] / m);   // the finish kick, before the constraint's share
    }
    val[0] = m * (w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    for (int a = 0; a < 3; ++a) {
      val[1 + a] = m * w[a];
      val[4 + a] = g[a];
    }
    val[7] = k * u2;
    if (c1 < 1.0) {   // the momentum the noise of the coming O step carries (steps: the number of that start)
      double xi[3];
      gaussian3(st.seed[s], kTiKey, (uint64_t)st.steps[s], (uint64_t)(i - st.ch.offsets[s]), 0, xi);   // (start, atom of its structure)
      const double sigma = sqrt((1.0 - c1 * c1) * kBoltzmann * st.t0[s] * kKappa / m);
      for (int a = 0; a < 3; ++a) val[8 + a] = m * (sigma * xi[a]);
    }
    val[11] = (std::isfinite(f[0]) && std::isfinite(f[1]) && std::isfinite(f[2])) ? 0.0 : 1.0;
  }
  reduce_store<kTiPart>(val, c, t, st.partial);
}

__global__ void __launch_bounds__(kWave * kFinalizeWaves) k_ti_finalize(TiView st, int32_t schedule, int32_t finish_only, double half_dt,
                                                                        double c1, const float* __restrict__ energies,
                                                                        double* __restrict__ obs) {
  const int lane = threadIdx.x % kWave;
  const int64_t s = (int64_t)blockIdx.x * kFinalizeWaves + threadIdx.x / kWave;
  if (s >= st.ch.S) return;   // (whole waves: s is uniform across a wave)
  const int fl = st.flags[s];
  double* coef = st.coef + kTiCoef * s;
  if (fl & M3G_DYN_ERROR) {
    if (lane == 0) coef[0] = 0.0;
    return;
  }
  double acc[kTiPart];
  wave_chunk_sum<kTiPart>(st.ch, s, st.partial, lane, acc);
  if (lane != 0) return;
  const double e = (double)energies[s];
  if (acc[11] != 0.0 || !std::isfinite(e)) {   // never move a structure with a non-finite force or energy
    st.flags[s] = fl | M3G_DYN_ERROR;
    coef[0] = 0.0;
    return;
  }
  const double lam = path_lambda(st, s, schedule);
  const double n = (double)(st.ch.offsets[s + 1] - st.ch.offsets[s]), mt = st.mtot[s];
  const bool started = fl & M3G_DYN_STARTED;
  double gbar[3], two_kappa_ke = acc[0];
  for (int a = 0; a < 3; ++a) gbar[a] = acc[4 + a] / mt;
  if (started) {
    double d[3];
    for (int a = 0; a < 3; ++a) d[a] = half_dt * (kKappa * gbar[a]);
    two_kappa_ke = acc[0] - 2.0 * (d[0] * acc[1] + d[1] * acc[2] + d[2] * acc[3]) + mt * (d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  }
  const double ke = two_kappa_ke / (2.0 * kKappa);
  const double us = 0.5 * acc[7], dh = e - us;
  double work = st.work[s];
  if (st.has_prev[s]) work += (lam - st.lam_prev[s]) * (0.5 * (dh + st.d_prev[s]));
  st.work[s] = work;
  st.lam_prev[s] = lam;
  st.d_prev[s] = dh;
  st.has_prev[s] = 1;
  int64_t* path = st.path + kPathWords * s;
  const bool sample = path[kPathIndex] >= path[kPathDiscard];
  if (sample) {
    const int64_t cnt = st.count[s] + 1;
    const double mean = st.mean[s], delta = dh - mean, mean1 = mean + delta / (double)cnt;
    st.count[s] = cnt;
    st.mean[s] = mean1;
    st.m2[s] += delta * (dh - mean1);
  }
  if (obs) {
    double* o = obs + M3G_TI_OBS * s;
    o[0] = ke;
    o[1] = 2.0 * ke / ((3.0 * n - 3.0) * kBoltzmann);
    o[2] = us;
    o[3] = dh;
    o[4] = lam;
    o[5] = work;
    o[6] = 0.0;
    o[7] = 0.0;
  }
  coef[1] = started ? 1.0 : 0.0;
  coef[2] = lam;
  for (int a = 0; a < 3; ++a) {
    coef[3 + a] = gbar[a];
    coef[6 + a] = acc[8 + a] / mt;
  }
  coef[9] = sample ? 1.0 : 0.0;
  coef[10] = (1.0 - c1 * c1) * kBoltzmann * st.t0[s] * kKappa;
  coef[11] = 0.0;
  if (finish_only) {
    st.flags[s] = fl & ~M3G_DYN_STARTED;
    coef[0] = 1.0;
    return;
  }
  coef[0] = 2.0;
  st.flags[s] = fl | M3G_DYN_STARTED;
  st.steps[s] += 1;
  path[kPathIndex] += 1;
}

__global__ void __launch_bounds__(kChunkRows) k_ti_apply(TiView st, double h, double c1, const float* __restrict__ forces, double* __restrict__ pos) {
  const int c = blockIdx.x;
  if (c >= st.ch.n_chunks()) return;
  const int s = st.ch.structure(c);
  const double* coef = st.coef + kTiCoef * s;
  const double act = coef[0];
  if (act == 0.0) return;   // failed: bitwise untouched
  const int64_t i = st.ch.row(c, threadIdx.x);
  if (!st.ch.holds(s, i)) return;
  const double m = st.mass[i], k = st.spring[i], lam = coef[2];
  double a[3], v[3], x[3], u2 = 0.0;
  for (int j = 0; j < 3; ++j) {
    x[j] = pos[3 * i + j];
    const double u = x[j] - st.ref[3 * i + j];
    u2 += u * u;
    const double g = lam * (double)forces[3 * i + j] - (1.0 - lam) * (k * u);
    a[j] = kKappa * (g - m * coef[3 + j]) / m;   // the constrained force: sum_i of it is zero
    v[j] = st.v[3 * i + j];
    if (coef[1] != 0.0) v[j] += h * a[j];
  }
  if (coef[9] != 0.0) st.msd[i] += u2;
  if (act == 1.0) {   // finish only
    for (int j = 0; j < 3; ++j) st.v[3 * i + j] = v[j];
    return;
  }
  double xi[3] = {0.0, 0.0, 0.0};
  if (c1 < 1.0) gaussian3(st.seed[s], kTiKey, (uint64_t)(st.steps[s] - 1), (uint64_t)(i - st.ch.offsets[s]), 0, xi);
  const double sigma = sqrt(coef[10] / m);
  for (int j = 0; j < 3; ++j) {   // B A O A
    v[j] += h * a[j];
    x[j] += h * v[j];
    v[j] = c1 * v[j] + sigma * xi[j] - coef[6 + j];
    x[j] += h * v[j];
    st.v[3 * i + j] = v[j];
    pos[3 * i + j] = x[j];
  }
}

// nullptr when the parameters are valid, else what is wrong with them
const char* ti_params_error(const m3g_ti_params* p) {
  if (!p) return "null parameters";
  if (p->schedule != M3G_TI_LINEAR && p->schedule != M3G_TI_SMOOTH) return "unknown schedule";
  if (!finite_positive(p->dt)) return "dt must be finite and > 0";
  if (!(std::isfinite(p->friction) && p->friction >= 0.0)) return "friction must be finite and >= 0";
  return nullptr;
}

// every structure holds two atoms at least: the constraint leaves 3 n - 3 degrees of freedom
bool ti_sizes_ok(int64_t N, int64_t S) { return batch_sizes_ok(N, S) && N >= 2 * S; }
}  // namespace
}  // namespace m3g

using namespace m3g;

extern "C" int m3g_ti_state_bytes(int64_t n_atoms, int64_t n_structs, size_t* bytes) {
  if (!bytes || !ti_sizes_ok(n_atoms, n_structs)) {
    set_error("m3g_ti_state_bytes: bad sizes (every structure holds at least two atoms)");
    return M3G_ERR_VALUE;
  }
  *bytes = ti_view(n_atoms, n_structs, nullptr).bytes;
  return M3G_OK;
}

extern "C" int m3g_ti_state_view(int64_t n_atoms, int64_t n_structs, size_t* mass_offset, size_t* velocity_offset) {
  return state_view_offsets("m3g_ti_state_view", ti_sizes_ok(n_atoms, n_structs), [&] { return ti_view(n_atoms, n_structs, nullptr).view; },
                            mass_offset, velocity_offset);
}

extern "C" int m3g_ti_init(const m3g_ti_params* p, int64_t n_atoms, int64_t n_structs, const int64_t* host_offsets, const double* host_masses,
                           const double* host_springs, const double* host_temperatures, const uint64_t* host_seeds, const double* vel,
                           const double* reference, void* state, size_t state_bytes, void* stream_) {
  if (const char* why = ti_params_error(p)) { set_error("m3g_ti_init: invalid parameters: %s", why); return M3G_ERR_VALUE; }
  constexpr const char* fn = "m3g_ti_init";
  const int64_t N = n_atoms, S = n_structs;
  if (!init_args_ok(fn, N, S, host_offsets && host_masses && host_springs && host_temperatures && host_seeds && vel && reference && state))
    return M3G_ERR_VALUE;
  if (!offsets_ok(fn, host_offsets, N, S)) return M3G_ERR_VALUE;
  for (int64_t i = 0; i < N; ++i) {
    if (!mass_ok(fn, host_masses, i)) return M3G_ERR_VALUE;
    if (!(std::isfinite(host_springs[i]) && host_springs[i] >= 0.0)) {
      set_error("m3g_ti_init: spring constant of atom %lld is not finite and >= 0", (long long)i);
      return M3G_ERR_VALUE;
    }
  }
  std::vector<double> mtot(S);
  for (int64_t s = 0; s < S; ++s) {
    if (host_offsets[s + 1] - host_offsets[s] < 2) {
      set_error("m3g_ti_init: structure %lld needs at least two atoms (the held centre of mass leaves 3 n - 3 degrees of freedom)", (long long)s);
      return M3G_ERR_VALUE;
    }
    if (!temperature_ok(fn, host_temperatures, s)) return M3G_ERR_VALUE;
    double m = 0.0, k = 0.0;
    for (int64_t i = host_offsets[s]; i < host_offsets[s + 1]; ++i) {
      m += host_masses[i];
      k += host_springs[i];
    }
    if (!(k > 0.0)) { set_error("m3g_ti_init: every spring constant of structure %lld is zero", (long long)s); return M3G_ERR_VALUE; }
    mtot[s] = m;
  }
  const auto [st, total] = ti_view(N, S, state);
  if (!state_fits(fn, state_bytes, total, true)) return M3G_ERR_SIZE;
  const ChunkTable table(host_offsets, S);
  hipStream_t s = (hipStream_t)stream_;
  if (int rc = upload_batch(table, st, host_offsets, host_masses, host_temperatures, host_seeds, s)) return rc;
  M3G_HIP_CHECK(hipMemcpyAsync(st.spring, host_springs, 8 * N, hipMemcpyHostToDevice, s));
  M3G_HIP_CHECK(hipMemcpyAsync(st.mtot, mtot.data(), 8 * S, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_ti_init, grid_for(3 * N, kChunkRows), dim3(kChunkRows), 0, s, st, vel, reference);   // (3 N >= S)
  hipLaunchKernelGGL(k_ti_path, dim3((unsigned)chunk_bound(N, S)), dim3(kChunkRows), 0, s, st, (int64_t)0, (int64_t)0, 1);
  return launched_and_synced(s);   // (the host tables above go out of scope)
}

extern "C" int m3g_ti_path(int64_t n_atoms, int64_t n_structs, void* state, size_t state_bytes, const double* host_lambda_begin,
                           const double* host_lambda_end, int64_t n_switch, int64_t n_discard, void* stream_) {
  const int64_t N = n_atoms, S = n_structs;
  if (!ti_sizes_ok(N, S) || !state || !host_lambda_begin || !host_lambda_end) { set_error("m3g_ti_path: null argument or bad sizes"); return M3G_ERR_VALUE; }
  if (n_switch < 0 || n_discard < 0) { set_error("m3g_ti_path: n_switch and n_discard must be >= 0"); return M3G_ERR_VALUE; }
  for (int64_t s = 0; s < S; ++s)
    for (const double lam : {host_lambda_begin[s], host_lambda_end[s]})
      if (!(lam >= 0.0 && lam <= 1.0)) { set_error("m3g_ti_path: lambda of structure %lld is not in [0, 1]", (long long)s); return M3G_ERR_VALUE; }
  const auto [st, total] = ti_view(N, S, state);
  if (!state_fits("m3g_ti_path", state_bytes, total)) return M3G_ERR_SIZE;
  hipStream_t s = (hipStream_t)stream_;
  M3G_HIP_CHECK(hipMemcpyAsync(st.lam_b, host_lambda_begin, 8 * S, hipMemcpyHostToDevice, s));
  M3G_HIP_CHECK(hipMemcpyAsync(st.lam_e, host_lambda_end, 8 * S, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_ti_path, dim3((unsigned)chunk_bound(N, S)), dim3(kChunkRows), 0, s, st, n_switch, n_discard, 0);
  return launched_and_synced(s);   // (the caller's host arrays)
}

extern "C" int m3g_ti_step(const m3g_ti_params* p, int64_t n_atoms, int64_t n_structs, void* state, size_t state_bytes, const float* forces,
                           const float* energies, double* pos, int32_t finish_only, double* obs, void* stream_) {
  if (const char* why = ti_params_error(p)) { set_error("m3g_ti_step: invalid parameters: %s", why); return M3G_ERR_VALUE; }
  const int64_t N = n_atoms, S = n_structs;
  if (!ti_sizes_ok(N, S) || !state) { set_error("m3g_ti_step: null argument or bad sizes"); return M3G_ERR_VALUE; }
  if (!forces || !energies || !pos) { set_error("m3g_ti_step: missing forces, energies or pos"); return M3G_ERR_VALUE; }
  const auto [st, total] = ti_view(N, S, state);
  if (!state_fits("m3g_ti_step", state_bytes, total)) return M3G_ERR_SIZE;
  hipStream_t s = (hipStream_t)stream_;
  const double h = 0.5 * p->dt, c1 = std::exp(-p->friction * p->dt);   // (friction 0: c1 = 1, no noise drawn)
  const auto [chunks, waves] = step_grids(N, S);
  hipLaunchKernelGGL(k_ti_partials, chunks, dim3(kChunkRows), 0, s, st, p->schedule, h, c1, forces, pos);
  hipLaunchKernelGGL(k_ti_finalize, waves, dim3(kFinalizeThreads), 0, s, st, p->schedule, finish_only, h, c1, energies, obs);
  hipLaunchKernelGGL(k_ti_apply, chunks, dim3(kChunkRows), 0, s, st, h, c1, forces, pos);
  M3G_RETURN_LAUNCH_STATUS();
}

extern "C" int m3g_ti_read(int64_t n_atoms, int64_t n_structs, const void* state, size_t state_bytes, int32_t* host_flags, int64_t* host_steps,
                           double* host_work, int64_t* host_count, double* host_mean, double* host_m2, double* host_vel,
                           double* host_msd_sum, void* stream_) {
  const int64_t N = n_atoms, S = n_structs;
  if (!ti_sizes_ok(N, S) || !state) { set_error("m3g_ti_read: null argument or bad sizes"); return M3G_ERR_VALUE; }
  const auto [st, total] = ti_view(N, S, (void*)state);
  if (!state_fits("m3g_ti_read", state_bytes, total)) return M3G_ERR_SIZE;
  hipStream_t s = (hipStream_t)stream_;
  if (int rc = read_head(st, host_flags, host_steps, host_vel, s)) return rc;
  M3G_HIP_CHECK(read_back(host_work, st.work, S, s));
  M3G_HIP_CHECK(read_back(host_count, st.count, S, s));
  M3G_HIP_CHECK(read_back(host_mean, st.mean, S, s));
  M3G_HIP_CHECK(read_back(host_m2, st.m2, S, s));
  M3G_HIP_CHECK(read_back(host_msd_sum, st.msd, N, s));
  M3G_HIP_CHECK(hipStreamSynchronize(s));
  return M3G_OK;
}
