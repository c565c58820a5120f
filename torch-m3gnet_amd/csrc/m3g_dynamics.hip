// Batched molecular dynamics: NVE (ASE's VelocityVerlet), NVT Berendsen (ASE's NVTBerendsen), NVT Langevin (BAOAB, not ASE's scheme)
// and isotropic NPT Berendsen (ASE's NPTBerendsen), every structure of a batch with its own target temperature and random stream.
// The m3gnet package the reference stands in for runs MD through ASE on the host, one structure at a time.  Here one call -- finish
// step k, observables, start step k+1 -- is three launches for the whole batch, over the chunk table of m3g_chunks.h:
//   k_dyn_partials   one workgroup per chunk (<= kChunkRows atoms of ONE structure): the finish kick in registers, then the partial
//                    sums of m |v|^2, m v, F and a count of non-finite forces, in a fixed tree order;
//   k_dyn_finalize   one wave per structure: the chunk partials in chunk order (lane-strided, then a fixed butterfly), the error
//                    verdict, KE, T, V, P, the thermostat / barostat scalars lambda and mu, the centre-of-mass momentum in closed form
//                    (lambda sum m v + dt/2 kappa sum F) / n -- no second pass over the atoms --, the new cell and the observables;
//   k_dyn_apply      one workgroup per chunk: the finish kick and the start step of every atom (Philox4x64-10 for Langevin).
// No atomics: every result depends on the structure's own rows only, so it is bitwise the same alone or in any batch.  No allocation,
// copy or wait in m3g_dyn_step (capture-safe).  What the five step families spell alike -- the partials body (shared with m3g_nhc_*),
// the Box-Muller draw, the cell volume, the checks and copies of the entry points -- is m3g_integrator.h.
#include <cmath>

#include "m3g_integrator.h"

namespace m3g {
namespace {
__global__ void __launch_bounds__(kChunkRows) k_dyn_init(DynView st, const double* __restrict__ vel) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < 3 * st.N) st.v[i] = vel[i];
  if (i < st.ch.S) {
    st.flags[i] = 0;
    st.steps[i] = 0;
    st.coef[kCoef * i] = 0.0;
  }
}

__global__ void __launch_bounds__(kChunkRows) k_dyn_partials(DynView st, double half_dt, const float* __restrict__ forces) {
  // the finish kick (written by k_dyn_apply)
  md_partials(st, forces, [=](int, double v, double f, double m) { return v + half_dt * (kKappa * f / m); });
}

__global__ void __launch_bounds__(kWave * kFinalizeWaves) k_dyn_finalize(DynView st, m3g_dyn_params p, int32_t finish_only, double c1,
                                                                         const float* __restrict__ stresses, double* __restrict__ lattice,
                                                                         float* __restrict__ lattice32, double* __restrict__ obs) {
  const int lane = threadIdx.x % kWave;
  const int64_t s = (int64_t)blockIdx.x * kFinalizeWaves + threadIdx.x / kWave;
  if (s >= st.ch.S) return;   // (whole waves: s is uniform across a wave)
  const int fl = st.flags[s];
  double* coef = st.coef + kCoef * s;
  if (fl & M3G_DYN_ERROR) {
    if (lane == 0) coef[0] = 0.0;
    return;
  }
  double acc[kPart];
  wave_chunk_sum<kPart>(st.ch, s, st.partial, lane, acc);
  if (lane != 0) return;
  const bool npt = p.ensemble == M3G_DYN_NPT_BERENDSEN;
  bool bad = acc[7] != 0.0;
  const float* sv = stresses ? stresses + 6 * s : nullptr;
  if (npt)
    for (int k = 0; k < 6; ++k) bad = bad || !std::isfinite(sv[k]);
  if (bad) {   // never move a structure with non-finite forces
    st.flags[s] = fl | M3G_DYN_ERROR;
    coef[0] = 0.0;
    return;
  }
  const double n = (double)(st.ch.offsets[s + 1] - st.ch.offsets[s]);
  const double ke = acc[0] / (2.0 * kKappa);
  const double two_ke = 2.0 * ke;
  const double temp = two_ke / (3.0 * n * kBoltzmann);
  double vol = NAN, trw = NAN;
  double* L = lattice ? lattice + 9 * s : nullptr;
  if (L) vol = cell_volume(L);
  if (L && sv) trw = virial_trace(vol, sv);
  if (obs) {
    obs[4 * s] = ke;
    obs[4 * s + 1] = temp;
    obs[4 * s + 2] = (trw + two_ke) / (3.0 * vol);
    obs[4 * s + 3] = vol;
  }
  coef[1] = (fl & M3G_DYN_STARTED) ? 1.0 : 0.0;   // finish kick in k_dyn_apply
  if (finish_only) {
    st.flags[s] = fl & ~M3G_DYN_STARTED;
    coef[0] = 1.0;
    return;
  }
  double lam = 1.0, mu = 1.0;
  if (p.ensemble == M3G_DYN_NVT_BERENDSEN || npt) {
    if (temp == 0.0) {
      lam = 1.1;
    } else {
      const double x = 1.0 + (p.dt / p.taut) * (st.t0[s] / temp - 1.0);
      lam = fmin(fmax(sqrt(fmax(x, 0.0)), 0.9), 1.1);
    }
  }
  if (npt) {
    const double pressure = (trw + lam * lam * two_ke) / (3.0 * vol);
    mu = 1.0 - (p.dt * p.compressibility / (3.0 * p.taup)) * (p.pressure - pressure);
    for (int k = 0; k < 9; ++k) {
      const double l = mu * L[k];
      L[k] = l;
      if (lattice32) lattice32[9 * s + k] = (float)l;
    }
  }
  const double hk = 0.5 * p.dt * kKappa;
  for (int k = 0; k < 3; ++k) coef[4 + k] = p.fix_com ? (lam * acc[1 + k] + hk * acc[4 + k]) / n : 0.0;
  coef[0] = 2.0;
  coef[2] = lam;
  coef[3] = mu;
  coef[7] = (1.0 - c1 * c1) * kBoltzmann * st.t0[s] * kKappa;
  st.flags[s] = fl | M3G_DYN_STARTED;
  st.steps[s] += 1;
}

__global__ void __launch_bounds__(kChunkRows) k_dyn_apply(DynView st, m3g_dyn_params p, double c1, const float* __restrict__ forces,
                                                          double* __restrict__ pos) {
  const int c = blockIdx.x;
  if (c >= st.ch.n_chunks()) return;
  const int s = st.ch.structure(c);
  const double* coef = st.coef + kCoef * s;
  const double act = coef[0];
  if (act == 0.0) return;   // failed: bitwise untouched
  const int64_t i = st.ch.row(c, threadIdx.x);
  if (!st.ch.holds(s, i)) return;
  const double m = st.mass[i], h = 0.5 * p.dt;
  double a[3], v[3], x[3];
  for (int k = 0; k < 3; ++k) {
    a[k] = kKappa * (double)forces[3 * i + k] / m;
    v[k] = st.v[3 * i + k];
    if (coef[1] != 0.0) v[k] += h * a[k];
  }
  if (act == 1.0) {   // finish only
    for (int k = 0; k < 3; ++k) st.v[3 * i + k] = v[k];
    return;
  }
  for (int k = 0; k < 3; ++k) x[k] = pos[3 * i + k];
  if (p.ensemble == M3G_DYN_NVT_LANGEVIN) {   // B A O A
    double xi[3];
    gaussian3(st.seed[s], kLangevinKey, (uint64_t)(st.steps[s] - 1), (uint64_t)(i - st.ch.offsets[s]), 0, xi);   // (start, atom of its structure)
    const double sigma = sqrt(coef[7] / m);
    for (int k = 0; k < 3; ++k) {
      v[k] += h * a[k];
      x[k] += h * v[k];
      v[k] = c1 * v[k] + sigma * xi[k];
      x[k] += h * v[k];
    }
  } else {
    const double lam = coef[2], mu = coef[3];
    for (int k = 0; k < 3; ++k) {
      v[k] = lam * v[k];
      v[k] += h * a[k];
      if (p.fix_com) v[k] -= coef[4 + k] / m;
      x[k] = mu * x[k];
      x[k] += p.dt * v[k];
    }
  }
  for (int k = 0; k < 3; ++k) {
    st.v[3 * i + k] = v[k];
    pos[3 * i + k] = x[k];
  }
}

// nullptr when the parameters are valid, else what is wrong with them
const char* dyn_params_error(const m3g_dyn_params* p) {
  if (!p) return "null parameters";
  if (p->ensemble < M3G_DYN_NVE || p->ensemble > M3G_DYN_NPT_BERENDSEN) return "unknown ensemble";
  if (p->fix_com != 0 && p->fix_com != 1) return "fix_com must be 0 or 1";
  if (!finite_positive(p->dt)) return "dt must be finite and > 0";
  if (!(std::isfinite(p->friction) && p->friction >= 0.0)) return "friction must be finite and >= 0";
  const bool berendsen = p->ensemble == M3G_DYN_NVT_BERENDSEN || p->ensemble == M3G_DYN_NPT_BERENDSEN;
  if (berendsen && !finite_positive(p->taut)) return "taut must be finite and > 0";
  if (p->ensemble == M3G_DYN_NPT_BERENDSEN) {
    if (!finite_positive(p->taup)) return "taup must be finite and > 0";
    if (!finite_positive(p->compressibility)) return "compressibility must be finite and > 0";
    if (!std::isfinite(p->pressure)) return "pressure must be finite";
  }
  if (p->ensemble == M3G_DYN_NVT_LANGEVIN && p->fix_com) return "fix_com is not supported with the Langevin thermostat";
  return nullptr;
}

double langevin_c1(const m3g_dyn_params* p) { return p->ensemble == M3G_DYN_NVT_LANGEVIN ? std::exp(-p->friction * p->dt) : 1.0; }
}  // namespace
}  // namespace m3g

using namespace m3g;

extern "C" int m3g_dyn_state_bytes(int64_t n_atoms, int64_t n_structs, size_t* bytes) {
  if (!bytes || !batch_sizes_ok(n_atoms, n_structs)) { set_error("m3g_dyn_state_bytes: bad sizes"); return M3G_ERR_VALUE; }
  *bytes = dyn_view(n_atoms, n_structs, nullptr).bytes;
  return M3G_OK;
}

extern "C" int m3g_dyn_state_view(int64_t n_atoms, int64_t n_structs, size_t* mass_offset, size_t* velocity_offset) {
  return state_view_offsets("m3g_dyn_state_view", batch_sizes_ok(n_atoms, n_structs), [&] { return dyn_view(n_atoms, n_structs, nullptr).view; },
                            mass_offset, velocity_offset);
}

extern "C" int m3g_dyn_init(const m3g_dyn_params* p, int64_t n_atoms, int64_t n_structs, const int64_t* host_offsets, const double* host_masses,
                            const double* host_temperatures, const uint64_t* host_seeds, const double* vel, void* state, size_t state_bytes,
                            void* stream_) {
  if (const char* why = dyn_params_error(p)) { set_error("m3g_dyn_init: invalid parameters: %s", why); return M3G_ERR_VALUE; }
  constexpr const char* fn = "m3g_dyn_init";
  const int64_t N = n_atoms, S = n_structs;
  if (!init_args_ok(fn, N, S, host_offsets && host_masses && host_temperatures && host_seeds && vel && state)) return M3G_ERR_VALUE;
  if (!offsets_ok(fn, host_offsets, N, S)) return M3G_ERR_VALUE;
  for (int64_t i = 0; i < N; ++i)
    if (!mass_ok(fn, host_masses, i)) return M3G_ERR_VALUE;
  for (int64_t s = 0; s < S; ++s)
    if (!temperature_ok(fn, host_temperatures, s, "structure", true)) return M3G_ERR_VALUE;
  const auto [st, total] = dyn_view(N, S, state);
  if (!state_fits(fn, state_bytes, total, true)) return M3G_ERR_SIZE;
  const ChunkTable table(host_offsets, S);
  hipStream_t s = (hipStream_t)stream_;
  if (int rc = upload_batch(table, st, host_offsets, host_masses, host_temperatures, host_seeds, s)) return rc;
  const int64_t work = 3 * N > S ? 3 * N : S;
  hipLaunchKernelGGL(k_dyn_init, grid_for(work, kChunkRows), dim3(kChunkRows), 0, s, st, vel);
  return launched_and_synced(s);   // (the host tables above go out of scope)
}

extern "C" int m3g_dyn_step(const m3g_dyn_params* p, int64_t n_atoms, int64_t n_structs, void* state, size_t state_bytes, const float* forces,
                            const float* stresses, double* pos, double* lattice, float* lattice32, int32_t finish_only, double* obs, void* stream_) {
  if (const char* why = dyn_params_error(p)) { set_error("m3g_dyn_step: invalid parameters: %s", why); return M3G_ERR_VALUE; }
  const int64_t N = n_atoms, S = n_structs;
  if (!batch_sizes_ok(N, S) || !state || !forces || !pos) { set_error("m3g_dyn_step: null argument or bad sizes"); return M3G_ERR_VALUE; }
  if (p->ensemble == M3G_DYN_NPT_BERENDSEN && (!stresses || !lattice)) { set_error("m3g_dyn_step: NPT needs stresses and the fp64 lattice"); return M3G_ERR_VALUE; }
  const auto [st, total] = dyn_view(N, S, state);
  if (!state_fits("m3g_dyn_step", state_bytes, total)) return M3G_ERR_SIZE;
  hipStream_t s = (hipStream_t)stream_;
  const double c1 = langevin_c1(p);
  const auto [chunks, waves] = step_grids(N, S);
  hipLaunchKernelGGL(k_dyn_partials, chunks, dim3(kChunkRows), 0, s, st, 0.5 * p->dt, forces);
  hipLaunchKernelGGL(k_dyn_finalize, waves, dim3(kFinalizeThreads), 0, s, st, *p, finish_only, c1, stresses, lattice, lattice32, obs);
  hipLaunchKernelGGL(k_dyn_apply, chunks, dim3(kChunkRows), 0, s, st, *p, c1, forces, pos);
  M3G_RETURN_LAUNCH_STATUS();
}

extern "C" int m3g_dyn_read(int64_t n_atoms, int64_t n_structs, const void* state, size_t state_bytes, int32_t* host_flags, int64_t* host_steps,
                            double* host_vel, void* stream_) {
  const int64_t N = n_atoms, S = n_structs;
  if (!batch_sizes_ok(N, S) || !state) { set_error("m3g_dyn_read: null argument or bad sizes"); return M3G_ERR_VALUE; }
  const auto [st, total] = dyn_view(N, S, (void*)state);
  if (!state_fits("m3g_dyn_read", state_bytes, total)) return M3G_ERR_SIZE;
  hipStream_t s = (hipStream_t)stream_;
  if (int rc = read_head(st, host_flags, host_steps, host_vel, s)) return rc;
  M3G_HIP_CHECK(hipStreamSynchronize(s));
  return M3G_OK;
}
