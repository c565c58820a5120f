// Batched molecular dynamics, the deterministic ensembles: Nose-Hoover chain NVT and isotropic Martyna-Tobias-Klein NPT (Martyna,
// Tuckerman, Tobias, Klein, Mol. Phys. 87, 1117 (1996)), every structure of a batch with its own target temperature, beside the
// ensembles of m3g_dynamics.hip and on the same layers (the chunk table of m3g_chunks.h, the constants of m3g_dyn_state.h; the chain
// half-step is m3g_nhc_chain.h, shared with m3g_mtk.hip).
// One step is T(h) B(h) A(dt) [forces] B(h) T(h), h = dt/2: T the thermostat (and, NPT, barostat) half-step, B the kick, A the drift.
// One call -- finish step k, observables, start step k+1 -- is three launches for the whole batch, as m3g_dyn_step:
//   k_nhc_partials   one workgroup per chunk: the finish kick in registers (its two coefficients are those of the start's kick: the
//                    barostat velocity has not changed since), then the partial sums of m |v|^2, m v, F and the non-finite count;
//   k_nhc_finalize   one wave per structure: the chunk partials in chunk order, the error verdict, then on lane 0 the serial chain
//                    arithmetic of the finish and of the next start (the kinetic energy after a uniform scale is s^2 times the sum,
//                    so there is no second pass over the atoms), the observables between them, the new cell and the coefficients;
//   k_nhc_apply      one workgroup per chunk: v = lambda (finish-kicked v), the start kick, the centre-of-mass momentum in closed
//                    form (it is linear in sum m v and sum F of the same partials), the drift.
// No atomics: every result depends on the structure's own rows only, so it is bitwise the same alone or in any batch.  No allocation,
// copy or wait in m3g_nhc_step (capture-safe).  The partials body (shared with m3g_dyn_*), the cell volume and the checks and copies
// of the entry points are m3g_integrator.h.
#include <cmath>

#include "m3g_integrator.h"
#include "m3g_nhc_chain.h"

namespace m3g {
namespace {
// per structure: action (0 none, 1 finish only, 2 finish + start), finish?, lambda (finish only: s1), the finish kick (v, a), the start
// kick (v, a: kept for the next call's finish), the drift (x, v), pbar [3]
constexpr int kNhcCoef = 12;
enum NhcCoef : int { kAct, kFinish, kLam, kFinV, kFinA, kKickV, kKickA, kDriftX, kDriftV, kPbar };

constexpr int chain_row(int M) { return 4 * M + 1; }   // xi[M], vxi[M], xib[M], vxib[M], veps

struct NhcView {
  int64_t N;
  int M;
  ChunkView ch;
  double *partial, *mass, *v, *t0, *coef, *chain;
  int32_t* flags;
  int64_t* steps;
};
inline Carved<NhcView> nhc_view(int64_t N, int64_t S, int M, void* state) {
  Carve c{state};
  NhcView st{N, M};
  st.ch = chunk_view(N, S, c);
  st.partial = c.take<double>(kPart * chunk_bound(N, S));
  st.mass = c.take<double>(N);
  st.v = c.take<double>(3 * N);
  st.t0 = c.take<double>(S);
  st.flags = c.take<int32_t>(S);
  st.steps = c.take<int64_t>(S);
  st.coef = c.take<double>(kNhcCoef * S);
  st.chain = c.take<double>(chain_row(M) * S);
  return {st, c.off};
}

// sinh(y) / y as its series to y^6.  The next term is y^8 / 362880: below 2^-53 for |y| < 0.05, and the arguments here are
// veps dt / 2 and alpha veps dt / 4 with veps ~ 1 / (taup sqrt(g + 3)), of the order of 1e-3 and less.
__device__ inline double sinhc(double y) {
  const double y2 = y * y;
  return 1.0 + y2 / 6.0 * (1.0 + y2 / 20.0 * (1.0 + y2 / 42.0));
}

// v after a kick (or x after a drift): both are linear maps with two coefficients of the structure
__device__ inline double axpby(double v, double cv, double a, double ca) { return v * cv + a * ca; }

__global__ void __launch_bounds__(kChunkRows) k_nhc_init(NhcView st, const double* __restrict__ vel) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < 3 * st.N) st.v[i] = vel[i];
  if (i < st.ch.S) {
    st.flags[i] = 0;
    st.steps[i] = 0;
    for (int k = 0; k < kNhcCoef; ++k) st.coef[kNhcCoef * i + k] = 0.0;
    for (int k = 0; k < chain_row(st.M); ++k) st.chain[chain_row(st.M) * i + k] = 0.0;
  }
}

__global__ void __launch_bounds__(kChunkRows) k_nhc_partials(NhcView st, const float* __restrict__ forces) {
  // the finish kick (written by k_nhc_apply)
  md_partials(st, forces, [&](int s, double v, double f, double m) {
    const double* coef = st.coef + kNhcCoef * s;
    return axpby(v, coef[kKickV], kKappa * f / m, coef[kKickA]);
  });
}

__global__ void __launch_bounds__(kWave * kFinalizeWaves) k_nhc_finalize(NhcView st, m3g_nhc_params p, int32_t finish_only,
                                                                         const float* __restrict__ stresses, double* __restrict__ lattice,
                                                                         float* __restrict__ lattice32, double* __restrict__ obs) {
  __shared__ double rows[kFinalizeWaves][chain_row(kMaxChain)];   // lane 0's chain row: the serial arithmetic runs out of LDS
  const int lane = threadIdx.x % kWave;
  const int64_t s = (int64_t)blockIdx.x * kFinalizeWaves + threadIdx.x / kWave;
  if (s >= st.ch.S) return;   // (whole waves: s is uniform across a wave)
  const int fl = st.flags[s];
  double* coef = st.coef + kNhcCoef * s;
  if (fl & M3G_DYN_ERROR) {
    if (lane == 0) coef[kAct] = 0.0;
    return;
  }
  double acc[kPart];
  wave_chunk_sum<kPart>(st.ch, s, st.partial, lane, acc);
  if (lane != 0) return;
  const bool npt = p.ensemble == M3G_NHC_NPT_MTK;
  bool bad = acc[7] != 0.0;
  const float* sv = stresses ? stresses + 6 * s : nullptr;
  if (npt)
    for (int k = 0; k < 6; ++k) bad = bad || !std::isfinite(sv[k]);
  if (bad) {   // never move a structure with non-finite forces
    st.flags[s] = fl | M3G_DYN_ERROR;
    coef[kAct] = 0.0;
    return;
  }
  const int M = st.M, n_c = p.chain_substeps;
  double* chain = st.chain + chain_row(M) * s;
  double* row = rows[threadIdx.x / kWave];
  for (int k = 0; k < chain_row(M); ++k) row[k] = chain[k];
  double *xi = row, *vxi = row + M, *xib = row + 2 * M, *vxib = row + 3 * M;
  double veps = row[4 * M];

  const double n = (double)(st.ch.offsets[s + 1] - st.ch.offsets[s]);
  const double g = p.fix_com ? 3.0 * n - 3.0 : 3.0 * n;
  const double kt = kBoltzmann * st.t0[s], gkt = g * kt;
  const double qk = kt * p.taut * p.taut, q0 = g * qk;
  const double qb = kt * p.taup * p.taup, wb = (g + 3.0) * qb;
  const double alpha = 1.0 + 3.0 / g;
  const double h = 0.5 * p.dt;
  double k2 = acc[0] / kKappa;   // twice the kinetic energy, eV
  double vol = NAN, trw = NAN;
  double* L = lattice ? lattice + 9 * s : nullptr;
  if (L) vol = cell_volume(L);
  if (L && sv) trw = virial_trace(vol, sv);
  auto g_eps = [&]() { return (alpha * k2 + trw - 3.0 * vol * p.pressure) / wb; };
  auto baro_chain = [&]() {
    double kb2 = wb * veps * veps;
    veps = veps * chain_half_step(qb, qb, xib, vxib, M, n_c, kb2, kt, kt, h);
  };

  double s1 = 1.0;
  if (fl & M3G_DYN_STARTED) {   // the T(h) that ends the step under way
    if (npt) {
      veps += h * g_eps();
      baro_chain();
    }
    s1 = chain_half_step(q0, qk, xi, vxi, M, n_c, k2, gkt, kt, h);
  }
  if (obs) {
    double ext = gkt * xi[0] + 0.5 * q0 * vxi[0] * vxi[0], tail = 0.0;
    for (int k = 1; k < M; ++k) {
      tail += xi[k];
      ext += 0.5 * qk * vxi[k] * vxi[k];
    }
    ext += kt * tail;
    if (npt) {
      double sum = 0.0;
      ext += p.pressure * vol + 0.5 * wb * veps * veps;
      for (int k = 0; k < M; ++k) {
        sum += xib[k];
        ext += 0.5 * qb * vxib[k] * vxib[k];
      }
      ext += kt * sum;
    }
    double* o = obs + M3G_NHC_OBS * s;
    o[0] = 0.5 * k2;
    o[1] = k2 / (3.0 * n * kBoltzmann);
    o[2] = (trw + k2) / (3.0 * vol);
    o[3] = vol;
    o[4] = ext;
    o[5] = 0.0;
  }
  coef[kFinish] = (fl & M3G_DYN_STARTED) ? 1.0 : 0.0;
  coef[kFinV] = coef[kKickV];
  coef[kFinA] = coef[kKickA];
  if (finish_only) {
    st.flags[s] = fl & ~M3G_DYN_STARTED;
    coef[kLam] = s1;
    coef[kAct] = 1.0;
    for (int k = 0; k < chain_row(M) - 1; ++k) chain[k] = row[k];
    chain[4 * M] = veps;
    return;
  }
  const double s2 = chain_half_step(q0, qk, xi, vxi, M, n_c, k2, gkt, kt, h);   // the T(h) that opens the next step
  const double lam = s1 * s2;
  double kv = 1.0, ka = h, dx = 1.0, dv = p.dt;
  if (npt) {
    baro_chain();
    veps += h * g_eps();
    double y = 0.5 * alpha * veps * h;
    kv = exp(-2.0 * y);
    ka = h * exp(-y) * sinhc(y);
    y = veps * h;
    dx = exp(2.0 * y);
    dv = p.dt * exp(y) * sinhc(y);
    for (int k = 0; k < 9; ++k) {
      const double l = dx * L[k];
      L[k] = l;
      if (lattice32) lattice32[9 * s + k] = (float)l;
    }
  }
  for (int k = 0; k < 3; ++k) coef[kPbar + k] = p.fix_com ? (kv * lam * acc[1 + k] + ka * kKappa * acc[4 + k]) / n : 0.0;
  coef[kLam] = lam;
  coef[kKickV] = kv;
  coef[kKickA] = ka;
  coef[kDriftX] = dx;
  coef[kDriftV] = dv;
  coef[kAct] = 2.0;
  for (int k = 0; k < chain_row(M) - 1; ++k) chain[k] = row[k];
  chain[4 * M] = veps;
  st.flags[s] = fl | M3G_DYN_STARTED;
  st.steps[s] += 1;
}

__global__ void __launch_bounds__(kChunkRows) k_nhc_apply(NhcView st, int32_t fix_com, const float* __restrict__ forces,
                                                          double* __restrict__ pos) {
  const int c = blockIdx.x;
  if (c >= st.ch.n_chunks()) return;
  const int s = st.ch.structure(c);
  const double* coef = st.coef + kNhcCoef * s;
  const double act = coef[kAct];
  if (act == 0.0) return;   // failed: bitwise untouched
  const int64_t i = st.ch.row(c, threadIdx.x);
  if (!st.ch.holds(s, i)) return;
  const double m = st.mass[i], lam = coef[kLam];
  double a[3], v[3];
  for (int k = 0; k < 3; ++k) {
    a[k] = kKappa * (double)forces[3 * i + k] / m;
    v[k] = st.v[3 * i + k];
    if (coef[kFinish] != 0.0) v[k] = axpby(v[k], coef[kFinV], a[k], coef[kFinA]);
    v[k] = lam * v[k];
  }
  if (act == 2.0) {
    for (int k = 0; k < 3; ++k) {
      v[k] = axpby(v[k], coef[kKickV], a[k], coef[kKickA]);
      if (fix_com) v[k] -= coef[kPbar + k] / m;
      pos[3 * i + k] = axpby(pos[3 * i + k], coef[kDriftX], v[k], coef[kDriftV]);
    }
  }
  for (int k = 0; k < 3; ++k) st.v[3 * i + k] = v[k];
}

// nullptr when the parameters are valid, else what is wrong with them
const char* nhc_params_error(const m3g_nhc_params* p) {
  if (!p) return "null parameters";
  if (p->ensemble != M3G_NHC_NVT && p->ensemble != M3G_NHC_NPT_MTK) return "unknown ensemble";
  if (p->fix_com != 0 && p->fix_com != 1) return "fix_com must be 0 or 1";
  if (p->chain_length < 1 || p->chain_length > kMaxChain) return "chain_length must be in 1 .. 8";
  if (p->chain_substeps < 1 || p->chain_substeps > kMaxChain) return "chain_substeps must be in 1 .. 8";
  if (!finite_positive(p->dt)) return "dt must be finite and > 0";
  if (!finite_positive(p->taut)) return "taut must be finite and > 0";
  if (p->ensemble == M3G_NHC_NPT_MTK) {
    if (!finite_positive(p->taup)) return "taup must be finite and > 0";
    if (!std::isfinite(p->pressure)) return "pressure must be finite";
  }
  return nullptr;
}
}  // namespace
}  // namespace m3g

using namespace m3g;

extern "C" int m3g_nhc_state_bytes(int64_t n_atoms, int64_t n_structs, int32_t chain_length, size_t* bytes) {
  if (!bytes || !batch_sizes_ok(n_atoms, n_structs) || !chain_ok(chain_length)) { set_error("m3g_nhc_state_bytes: bad sizes"); return M3G_ERR_VALUE; }
  *bytes = nhc_view(n_atoms, n_structs, chain_length, nullptr).bytes;
  return M3G_OK;
}

extern "C" int m3g_nhc_state_view(int64_t n_atoms, int64_t n_structs, int32_t chain_length, size_t* mass_offset, size_t* velocity_offset) {
  return state_view_offsets("m3g_nhc_state_view", batch_sizes_ok(n_atoms, n_structs) && chain_ok(chain_length),
                            [&] { return nhc_view(n_atoms, n_structs, chain_length, nullptr).view; }, mass_offset, velocity_offset);
}

extern "C" int m3g_nhc_init(const m3g_nhc_params* p, int64_t n_atoms, int64_t n_structs, const int64_t* host_offsets, const double* host_masses,
                            const double* host_temperatures, const double* vel, void* state, size_t state_bytes, void* stream_) {
  if (const char* why = nhc_params_error(p)) { set_error("m3g_nhc_init: invalid parameters: %s", why); return M3G_ERR_VALUE; }
  constexpr const char* fn = "m3g_nhc_init";
  const int64_t N = n_atoms, S = n_structs;
  if (!init_args_ok(fn, N, S, host_offsets && host_masses && host_temperatures && vel && state)) return M3G_ERR_VALUE;
  if (!offsets_ok(fn, host_offsets, N, S)) return M3G_ERR_VALUE;
  for (int64_t i = 0; i < N; ++i)
    if (!mass_ok(fn, host_masses, i)) return M3G_ERR_VALUE;
  for (int64_t s = 0; s < S; ++s) {
    if (!temperature_ok(fn, host_temperatures, s)) return M3G_ERR_VALUE;   // (the chain masses are proportional to it)
    if (p->fix_com && host_offsets[s + 1] - host_offsets[s] == 1) {
      set_error("m3g_nhc_init: structure %lld holds one atom, which fix_com leaves no degree of freedom", (long long)s);
      return M3G_ERR_VALUE;
    }
  }
  const auto [st, total] = nhc_view(N, S, p->chain_length, state);
  if (!state_fits(fn, state_bytes, total, true)) return M3G_ERR_SIZE;
  const ChunkTable table(host_offsets, S);
  hipStream_t s = (hipStream_t)stream_;
  if (int rc = upload_batch(table, st, host_offsets, host_masses, host_temperatures, nullptr, s)) return rc;
  const int64_t work = 3 * N > S ? 3 * N : S;
  hipLaunchKernelGGL(k_nhc_init, grid_for(work, kChunkRows), dim3(kChunkRows), 0, s, st, vel);
  return launched_and_synced(s);   // (the host tables above go out of scope)
}

extern "C" int m3g_nhc_step(const m3g_nhc_params* p, int64_t n_atoms, int64_t n_structs, void* state, size_t state_bytes, const float* forces,
                            const float* stresses, double* pos, double* lattice, float* lattice32, int32_t finish_only, double* obs, void* stream_) {
  if (const char* why = nhc_params_error(p)) { set_error("m3g_nhc_step: invalid parameters: %s", why); return M3G_ERR_VALUE; }
  const int64_t N = n_atoms, S = n_structs;
  if (!batch_sizes_ok(N, S) || !state || !forces || !pos) { set_error("m3g_nhc_step: null argument or bad sizes"); return M3G_ERR_VALUE; }
  if (p->ensemble == M3G_NHC_NPT_MTK && (!stresses || !lattice)) { set_error("m3g_nhc_step: NPT needs stresses and the fp64 lattice"); return M3G_ERR_VALUE; }
  const auto [st, total] = nhc_view(N, S, p->chain_length, state);
  if (!state_fits("m3g_nhc_step", state_bytes, total)) return M3G_ERR_SIZE;
  hipStream_t s = (hipStream_t)stream_;
  const auto [chunks, waves] = step_grids(N, S);
  hipLaunchKernelGGL(k_nhc_partials, chunks, dim3(kChunkRows), 0, s, st, forces);
  hipLaunchKernelGGL(k_nhc_finalize, waves, dim3(kFinalizeThreads), 0, s, st, *p, finish_only, stresses, lattice, lattice32, obs);
  hipLaunchKernelGGL(k_nhc_apply, chunks, dim3(kChunkRows), 0, s, st, p->fix_com, forces, pos);
  M3G_RETURN_LAUNCH_STATUS();
}

extern "C" int m3g_nhc_read(int64_t n_atoms, int64_t n_structs, int32_t chain_length, const void* state, size_t state_bytes, int32_t* host_flags,
                            int64_t* host_steps, double* host_vel, double* host_chain, void* stream_) {
  const int64_t N = n_atoms, S = n_structs;
  if (!batch_sizes_ok(N, S) || !chain_ok(chain_length) || !state) { set_error("m3g_nhc_read: null argument or bad sizes"); return M3G_ERR_VALUE; }
  const auto [st, total] = nhc_view(N, S, chain_length, (void*)state);
  if (!state_fits("m3g_nhc_read", state_bytes, total)) return M3G_ERR_SIZE;
  hipStream_t s = (hipStream_t)stream_;
  if (int rc = read_head(st, host_flags, host_steps, host_vel, s)) return rc;
  M3G_HIP_CHECK(read_back(host_chain, st.chain, (size_t)chain_row(chain_length) * S, s));
  M3G_HIP_CHECK(hipStreamSynchronize(s));
  return M3G_OK;
}
