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
// copy or wait in m3g_dyn_step (capture-safe).
#include <cmath>

#include "m3g_dyn_state.h"

namespace m3g {
namespace {
// three standard normals of atom `local` (its index inside its structure) at start k of a structure seeded `seed`
__device__ inline void gaussian3(uint64_t seed, uint64_t k, uint64_t local, double xi[3]) {
  uint64_t c[4] = {k, local, 0, 0};
  philox4x64_10(c, seed, 0);
  constexpr double kTwoPi = 6.283185307179586;
  const double r0 = sqrt(-2.0 * log(uniform53(c[0]))), r1 = sqrt(-2.0 * log(uniform53(c[2])));
  xi[0] = r0 * cos(kTwoPi * uniform53(c[1]));
  xi[1] = r0 * sin(kTwoPi * uniform53(c[1]));
  xi[2] = r1 * cos(kTwoPi * uniform53(c[3]));
}

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
  __shared__ double sh[kPart][kChunkRows];
  const int c = blockIdx.x, t = threadIdx.x;
  if (c >= st.ch.n_chunks()) return;
  const int s = st.ch.structure(c);
  const int fl = st.flags[s];
  if (fl & M3G_DYN_ERROR) return;   // frozen: finalize reads nothing of it
  const int64_t i = st.ch.row(c, t);
  double val[kPart] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (st.ch.holds(s, i)) {
    const double m = st.mass[i];
    double f[3], v[3];
    for (int k = 0; k < 3; ++k) {
      f[k] = forces[3 * i + k];
      v[k] = st.v[3 * i + k];
      if (fl & M3G_DYN_STARTED) v[k] += half_dt * (kKappa * f[k] / m);   // the finish kick (written by k_dyn_apply)
    }
    val[0] = m * (v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    for (int k = 0; k < 3; ++k) {
      val[1 + k] = m * v[k];
      val[4 + k] = f[k];
    }
    val[7] = (std::isfinite(f[0]) && std::isfinite(f[1]) && std::isfinite(f[2])) ? 0.0 : 1.0;
  }
  chunk_tree_reduce<kPart>(sh, val, t);
  if (t < kPart) st.partial[kPart * c + t] = sh[t][0];
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
  if (L) vol = fabs(L[0] * (L[4] * L[8] - L[5] * L[7]) - L[1] * (L[3] * L[8] - L[5] * L[6]) + L[2] * (L[3] * L[7] - L[4] * L[6]));
  if (L && sv) trw = vol * (((double)sv[0] + (double)sv[1]) + (double)sv[2]);   // tr W, W = V * stresses
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
    gaussian3(st.seed[s], (uint64_t)(st.steps[s] - 1), (uint64_t)(i - st.ch.offsets[s]), xi);
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
  if (!mass_offset || !velocity_offset || !batch_sizes_ok(n_atoms, n_structs)) { set_error("m3g_dyn_state_view: null argument or bad sizes"); return M3G_ERR_VALUE; }
  const DynView at = dyn_view(n_atoms, n_structs, nullptr).view;   // (over a null state: the offsets)
  *mass_offset = carve_offset(at.mass);
  *velocity_offset = carve_offset(at.v);
  return M3G_OK;
}

extern "C" int m3g_dyn_init(const m3g_dyn_params* p, int64_t n_atoms, int64_t n_structs, const int64_t* host_offsets, const double* host_masses,
                            const double* host_temperatures, const uint64_t* host_seeds, const double* vel, void* state, size_t state_bytes,
                            void* stream_) {
  if (const char* why = dyn_params_error(p)) { set_error("m3g_dyn_init: invalid parameters: %s", why); return M3G_ERR_VALUE; }
  if (!batch_sizes_ok(n_atoms, n_structs) || !host_offsets || !host_masses || !host_temperatures || !host_seeds || !vel || !state) {
    set_error("m3g_dyn_init: null argument or bad sizes");
    return M3G_ERR_VALUE;
  }
  const int64_t N = n_atoms, S = n_structs;
  if (!offsets_ok("m3g_dyn_init", host_offsets, N, S)) return M3G_ERR_VALUE;
  for (int64_t i = 0; i < N; ++i)
    if (!finite_positive(host_masses[i])) { set_error("m3g_dyn_init: mass of atom %lld is not finite and > 0", (long long)i); return M3G_ERR_VALUE; }
  for (int64_t s = 0; s < S; ++s)
    if (!(std::isfinite(host_temperatures[s]) && host_temperatures[s] >= 0.0)) {
      set_error("m3g_dyn_init: temperature of structure %lld is not finite and >= 0", (long long)s);
      return M3G_ERR_VALUE;
    }
  const auto [st, total] = dyn_view(N, S, state);
  if (state_bytes < total) { set_error("m3g_dyn_init: state buffer too small (%zu < %zu)", state_bytes, total); return M3G_ERR_SIZE; }
  const ChunkTable table(host_offsets, S);
  hipStream_t s = (hipStream_t)stream_;
  if (int rc = table.upload(st.ch, host_offsets, s)) return rc;
  M3G_HIP_CHECK(hipMemcpyAsync(st.mass, host_masses, 8 * N, hipMemcpyHostToDevice, s));
  M3G_HIP_CHECK(hipMemcpyAsync(st.t0, host_temperatures, 8 * S, hipMemcpyHostToDevice, s));
  M3G_HIP_CHECK(hipMemcpyAsync(st.seed, host_seeds, 8 * S, hipMemcpyHostToDevice, s));
  const int64_t work = 3 * N > S ? 3 * N : S;
  hipLaunchKernelGGL(k_dyn_init, grid_for(work, kChunkRows), dim3(kChunkRows), 0, s, st, vel);
  M3G_HIP_CHECK(hipGetLastError());
  M3G_HIP_CHECK(hipStreamSynchronize(s));   // (the host tables above go out of scope)
  return M3G_OK;
}

extern "C" int m3g_dyn_step(const m3g_dyn_params* p, int64_t n_atoms, int64_t n_structs, void* state, size_t state_bytes, const float* forces,
                            const float* stresses, double* pos, double* lattice, float* lattice32, int32_t finish_only, double* obs, void* stream_) {
  if (const char* why = dyn_params_error(p)) { set_error("m3g_dyn_step: invalid parameters: %s", why); return M3G_ERR_VALUE; }
  const int64_t N = n_atoms, S = n_structs;
  if (!batch_sizes_ok(N, S) || !state || !forces || !pos) { set_error("m3g_dyn_step: null argument or bad sizes"); return M3G_ERR_VALUE; }
  if (p->ensemble == M3G_DYN_NPT_BERENDSEN && (!stresses || !lattice)) { set_error("m3g_dyn_step: NPT needs stresses and the fp64 lattice"); return M3G_ERR_VALUE; }
  const auto [st, total] = dyn_view(N, S, state);
  if (state_bytes < total) { set_error("m3g_dyn_step: state buffer too small"); return M3G_ERR_SIZE; }
  hipStream_t s = (hipStream_t)stream_;
  const double c1 = langevin_c1(p);
  const dim3 grid((unsigned)chunk_bound(N, S));   // workgroups beyond the table's chunk count return at once
  hipLaunchKernelGGL(k_dyn_partials, grid, dim3(kChunkRows), 0, s, st, 0.5 * p->dt, forces);
  hipLaunchKernelGGL(k_dyn_finalize, grid_for(S, kFinalizeWaves), dim3(kWave * kFinalizeWaves), 0, s, st, *p,
                     finish_only, c1, stresses, lattice, lattice32, obs);
  hipLaunchKernelGGL(k_dyn_apply, grid, dim3(kChunkRows), 0, s, st, *p, c1, forces, pos);
  M3G_RETURN_LAUNCH_STATUS();
}

extern "C" int m3g_dyn_read(int64_t n_atoms, int64_t n_structs, const void* state, size_t state_bytes, int32_t* host_flags, int64_t* host_steps,
                            double* host_vel, void* stream_) {
  const int64_t N = n_atoms, S = n_structs;
  if (!batch_sizes_ok(N, S) || !state) { set_error("m3g_dyn_read: null argument or bad sizes"); return M3G_ERR_VALUE; }
  const auto [st, total] = dyn_view(N, S, (void*)state);
  if (state_bytes < total) { set_error("m3g_dyn_read: state buffer too small"); return M3G_ERR_SIZE; }
  hipStream_t s = (hipStream_t)stream_;
  M3G_HIP_CHECK(read_back(host_flags, st.flags, S, s));
  M3G_HIP_CHECK(read_back(host_steps, st.steps, S, s));
  M3G_HIP_CHECK(read_back(host_vel, st.v, 3 * N, s));
  M3G_HIP_CHECK(hipStreamSynchronize(s));
  return M3G_OK;
}
