// Normal-mode analysis of a batch of MD supercells, accumulated on the device while they are integrated (or fed any frames): the
// mass-weighted velocities and displacements projected on harmonic eigenvectors at given q-points, the per-mode second moments and
// the mode-velocity autocorrelation over a ring of the last n_lags samples (definitions: include/m3gnet_hip.h).  The sibling of
// m3g_trajectory.hip.  One m3g_nma_sample is three launches:
//   k_nma_com         one workgroup per chunk of the chunk table (m3g_chunks.h): partial sums of m, m (r - r0), m v and the number of
//                     rows with a non-finite value, in the fixed tree order;
//   k_nma_project     one workgroup per (structure, q): the structure's centre of mass from the chunk partials in chunk order; stage 1,
//                     the lattice Fourier sum W[b,a] = N_c^(-1/2) sqrt(m_b) sum_l phase x over the cells, thread (g, o = 3 b + a) taking
//                     the cells l = g, g + G', ... in order (3 n_u consecutive doubles of a cell are read by consecutive threads), then
//                     the G' groups in order; stage 2, Qdot = E[q]^H W by wave 0 with E[q] staged in LDS and W passed between lanes;
//                     |Qdot|^2, |Q|^2 into their sums, Qdot into the ring slot of this sample.  The first q of a structure also sums
//                     m |v|^2 of the same velocities.  3 N_s complex multiply-adds per q and (3 n_u)^2 for the product: no 3 N x 3 N
//                     projector exists anywhere;
//   k_nma_accumulate  grid (q, blocks of 256 (mode, lag) pairs): acf[mode, lag] += conj(Qdot(t - lag)) Qdot(t) from the ring; the first
//                     q of a structure advances its counters.
// No atomics and fixed orders that depend on the structure's own sizes only: every number is bitwise the same alone or in any batch.
// The ring position of a structure is its own sample count, kept in the state in two words (`done`, read by k_nma_project and written
// by k_nma_accumulate; `begun`, the other way round) so that no launch reads a word the same launch writes: no allocation, copy or wait
// in m3g_nma_sample (capture-safe).  A structure with a non-finite input is found from the chunk partials before anything of it is
// written, flagged, and skipped from then on.
#include <cmath>
#include <cstring>

#include "m3g_chunks.h"
#include "m3g_internal.h"

namespace m3g {
namespace {
constexpr int kMaxN = M3G_NMA_MAX_N;
constexpr int kMaxLags = M3G_NMA_MAX_LAGS;
constexpr int kPart = 8;                       // per chunk: sum m, sum m (r - r0) [3], sum m v [3], rows with a non-finite value
static_assert(kMaxN <= kWave, "stage 2 runs in one wave, lane nu on mode nu");

struct NmaView {
  int64_t N, S, n_q, n_modes;
  int32_t G;
  ChunkView ch;
  const int32_t *n_unit, *n_cells;          // [S]
  const int64_t* q_first;                    // [S]: the structure's first q
  const int32_t* q_struct;                   // [n_q]
  const int64_t *q_eig, *q_phase, *q_mode;   // [n_q]: where E[q], the phases of q and its modes begin
  const double *mass, *r0;                   // [N], [N,3]
  const double2 *phase, *eig;
  int64_t *done, *begun;                     // [S]: samples accumulated (the accumulators from here up to `part` are cleared by the init call)
  int32_t *took, *bad_now, *flags;           // [S]: this sample is accumulated / held a non-finite value; M3G_NMA_*
  double *kin_now, *kinetic_sum;             // [S]
  double *qdot2_sum, *q2_sum;                // [n_modes]
  double2 *last_qdot, *last_q;               // [n_modes]
  int64_t* lag_count;                        // [S, G]
  double2 *acf, *ring;                       // [n_modes, G]: lag, ring slot fastest
  double* part;                              // [chunks, kPart]
};
Carved<NmaView> nma_view(const m3g_nma_sizes& z, void* state) {
  const int64_t N = z.n_atoms, S = z.n_structs, Q = z.n_qpoints, M = z.n_modes, G = z.n_lags;
  Carve c{state};
  NmaView st{N, S, Q, M, z.n_lags};
  st.ch = chunk_view(N, S, c);
  st.n_unit = c.take<int32_t>(S);
  st.n_cells = c.take<int32_t>(S);
  st.q_first = c.take<int64_t>(S);
  st.q_struct = c.take<int32_t>(Q);
  st.q_eig = c.take<int64_t>(Q);
  st.q_phase = c.take<int64_t>(Q);
  st.q_mode = c.take<int64_t>(Q);
  st.mass = c.take<double>(N);
  st.r0 = c.take<double>(3 * N);
  st.phase = c.take<double2>(z.n_phase);
  st.eig = c.take<double2>(z.n_eig);
  st.done = c.take<int64_t>(S);
  st.begun = c.take<int64_t>(S);
  st.took = c.take<int32_t>(S);
  st.bad_now = c.take<int32_t>(S);
  st.flags = c.take<int32_t>(S);
  st.kin_now = c.take<double>(S);
  st.kinetic_sum = c.take<double>(S);
  st.qdot2_sum = c.take<double>(M);
  st.q2_sum = c.take<double>(M);
  st.last_qdot = c.take<double2>(M);
  st.last_q = c.take<double2>(M);
  st.lag_count = c.take<int64_t>(S * G);
  st.acf = c.take<double2>(M * G);
  st.ring = c.take<double2>(M * G);
  st.part = c.take<double>(kPart * chunk_bound(N, S));
  return {st, c.off};
}

// component k of the full-step velocity of row i: v + kick kappa F / m, the completion of m3g_traj_sample (m3g_trajectory.hip)
__device__ inline double sampled_velocity(double m, int64_t i, int k, const double* __restrict__ vel, const float* __restrict__ forces,
                                          double kick) {
  double v = vel[3 * i + k];
  if (forces) v += kick * (kKappa * (double)forces[3 * i + k] / m);
  return v;
}

__global__ void __launch_bounds__(kChunkRows) k_nma_com(NmaView st, const double* __restrict__ pos, const double* __restrict__ vel,
                                                         const float* __restrict__ forces, double kick) {
  __shared__ double sh[kPart][kChunkRows];
  const int c = blockIdx.x, t = threadIdx.x;
  if (c >= st.ch.n_chunks()) return;
  const int s = st.ch.structure(c);
  const int64_t i = st.ch.row(c, t);
  double val[kPart] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (st.ch.holds(s, i)) {
    const double m = st.mass[i];
    bool finite = true;
    val[0] = m;
    for (int k = 0; k < 3; ++k) {
      const double u = pos[3 * i + k] - st.r0[3 * i + k], v = sampled_velocity(m, i, k, vel, forces, kick);
      finite = finite && std::isfinite(u) && std::isfinite(v);
      val[1 + k] = m * u;
      val[4 + k] = m * v;
    }
    val[7] = finite ? 0.0 : 1.0;
  }
  chunk_tree_reduce<kPart>(sh, val, t);
  if (t < kPart) st.part[kPart * c + t] = sh[t][0];
}

template <int NCAP>
__global__ void __launch_bounds__(kChunkRows) k_nma_project(NmaView st, int32_t remove_com, const double* __restrict__ pos,
                                                             const double* __restrict__ vel, const float* __restrict__ forces, double kick) {
  __shared__ double2 E[NCAP * NCAP];
  __shared__ double sh[5][kChunkRows];   // per thread: re, im of the sum over v, re, im of that over u, sum m v^2
  const int64_t gq = blockIdx.x;
  const int t = threadIdx.x;
  const int s = st.q_struct[gq];
  const int nu = st.n_unit[s], R = 3 * nu, cells = st.n_cells[s];
  const bool first = gq == st.q_first[s];
  const int64_t done = st.done[s];
  double com[kPart];
  wave_chunk_sum<kPart>(st.ch, s, st.part, t % kWave, com);   // (whole waves: every lane ends with the same bits)
  const bool bad = com[7] != 0.0;
  const bool skip = bad || (st.flags[s] & M3G_NMA_NONFINITE) != 0;   // the same in every thread of every workgroup of the structure
  if (first && t == 0) {
    st.took[s] = skip ? 0 : 1;
    st.bad_now[s] = bad ? 1 : 0;
    if (!skip) st.begun[s] = done + 1;
  }
  if (skip) return;
  const double2* eig = st.eig + st.q_eig[gq];
  for (int e = t; e < R * R; e += kChunkRows) E[e] = eig[e];
  // stage 1
  const int groups = kChunkRows / R, o = t % R, g = t / R;   // groups >= 4
  const int64_t lo = st.ch.offsets[s];
  double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  if (g < groups) {
    const int b = o / 3, k = o % 3;
    const double2* ph = st.phase + st.q_phase[gq];
    const double ucm = com[1 + k] / com[0], vcm = remove_com ? com[4 + k] / com[0] : 0.0;
    for (int l = g; l < cells; l += groups) {
      const int64_t j = (int64_t)l * nu + b, i = lo + j;
      const double m = st.mass[i];
      double v = sampled_velocity(m, i, k, vel, forces, kick);
      if (remove_com) v -= vcm;
      const double u = (pos[3 * i + k] - st.r0[3 * i + k]) - ucm;
      const double2 f = ph[j];
      a[0] += f.x * v;
      a[1] += f.y * v;
      a[2] += f.x * u;
      a[3] += f.y * u;
      a[4] += m * (v * v);
    }
  }
  for (int k = 0; k < 5; ++k) sh[k][t] = a[k];
  __syncthreads();
  if (t >= kWave) return;   // wave 0 from here on: lane t < R holds row t of W, then mode t
  double w[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  if (t < R) {
    for (int x = 0; x < groups; ++x)
      for (int k = 0; k < 5; ++k) w[k] += sh[k][x * R + t];
    const double scale = sqrt(st.mass[lo + t / 3]) / sqrt((double)cells);   // (the home copy of unit atom b is row b)
    for (int k = 0; k < 4; ++k) w[k] *= scale;
  }
  double kin = w[4];   // lanes >= R hold +0.0
#pragma unroll
  for (int x = kWave / 2; x > 0; x >>= 1) kin += __shfl_xor(kin, x, kWave);
  // stage 2: conj(e) w = (e.x w.x + e.y w.y) + i (e.x w.y - e.y w.x), rows in order
  double q[4] = {0.0, 0.0, 0.0, 0.0};
  for (int r = 0; r < R; ++r) {
    const double vx = __shfl(w[0], r, kWave), vy = __shfl(w[1], r, kWave), ux = __shfl(w[2], r, kWave), uy = __shfl(w[3], r, kWave);
    if (t < R) {
      const double2 e = E[r * R + t];
      q[0] += e.x * vx + e.y * vy;
      q[1] += e.x * vy - e.y * vx;
      q[2] += e.x * ux + e.y * uy;
      q[3] += e.x * uy - e.y * ux;
    }
  }
  if (t < R) {
    const int64_t mode = st.q_mode[gq] + t;
    st.qdot2_sum[mode] += q[0] * q[0] + q[1] * q[1];
    st.q2_sum[mode] += q[2] * q[2] + q[3] * q[3];
    st.last_qdot[mode] = make_double2(q[0], q[1]);
    st.last_q[mode] = make_double2(q[2], q[3]);
    if (st.G > 0) st.ring[mode * st.G + done % st.G] = make_double2(q[0], q[1]);
  }
  if (first && t == 0) st.kin_now[s] = kin;
}

__global__ void __launch_bounds__(kChunkRows) k_nma_accumulate(NmaView st) {
  const int64_t gq = blockIdx.x;
  const int t = threadIdx.x;
  const int s = st.q_struct[gq];
  const bool lead = gq == st.q_first[s] && blockIdx.y == 0;   // the workgroup that advances the structure's counters
  if (!st.took[s]) {
    if (lead && t == 0 && st.bad_now[s]) st.flags[s] |= M3G_NMA_NONFINITE;
    return;
  }
  const int64_t begun = st.begun[s], G = st.G;   // begun >= 1 samples, this one included: the lags 0 .. min(begun, G) - 1 are stored
  const int R = 3 * st.n_unit[s];
  const int64_t idx = (int64_t)blockIdx.y * kChunkRows + t;
  if (G > 0 && idx < R * G) {
    const int64_t lag = idx % G, mode = st.q_mode[gq] + idx / G;
    if (lag < begun) {
      const double2 cur = st.ring[mode * G + (begun - 1) % G], old = st.ring[mode * G + (begun - 1 - lag) % G];
      double2 c = st.acf[mode * G + lag];
      c.x += old.x * cur.x + old.y * cur.y;
      c.y += old.x * cur.y - old.y * cur.x;
      st.acf[mode * G + lag] = c;
    }
  }
  if (lead) {
    for (int64_t lag = t; lag < G && lag < begun; lag += kChunkRows) st.lag_count[s * G + lag] += 1;
    if (t == 0) {
      st.done[s] = begun;
      st.kinetic_sum[s] += st.kin_now[s];
    }
  }
}

// nullptr when the sizes are valid, else what is wrong with them
const char* nma_error(const m3g_nma_sizes* z) {
  if (!z) return "null sizes";
  if (!batch_sizes_ok(z->n_atoms, z->n_structs)) return "bad sizes";
  if (z->n_unit_atoms < z->n_structs || z->n_unit_atoms > z->n_atoms) return "n_unit_atoms must be n_structs .. n_atoms";
  if (z->max_n < 3 || z->max_n > kMaxN || z->max_n % 3) return "max_n must be a multiple of 3 in 3 .. 64 (M3G_NMA_MAX_N)";
  if (z->n_lags < 0 || z->n_lags > kMaxLags) return "n_lags must be 0 .. 4096";
  if (z->n_qpoints < z->n_structs || z->n_qpoints > INT32_MAX) return "n_qpoints must be n_structs .. 2^31 - 1";
  if (z->n_modes < 3 * z->n_qpoints || z->n_modes > z->n_qpoints * z->max_n) return "n_modes does not fit n_qpoints and max_n";
  if (z->n_eig < 3 * z->n_modes || z->n_eig > z->n_modes * z->max_n) return "n_eig does not fit n_modes and max_n";
  if (z->n_phase < z->n_qpoints || z->n_phase > z->n_qpoints * z->n_atoms) return "n_phase does not fit n_qpoints and n_atoms";
  return nullptr;
}
bool params_ok(const m3g_nma_params* p) { return p && (p->remove_com == 0 || p->remove_com == 1); }
}  // namespace
}  // namespace m3g

using namespace m3g;

extern "C" int m3g_nma_state_bytes(const m3g_nma_sizes* sizes, size_t* bytes) {
  if (const char* why = nma_error(sizes)) { set_error("m3g_nma_state_bytes: %s", why); return M3G_ERR_VALUE; }
  if (!bytes) { set_error("m3g_nma_state_bytes: null argument"); return M3G_ERR_VALUE; }
  *bytes = nma_view(*sizes, nullptr).bytes;
  return M3G_OK;
}

extern "C" int m3g_nma_init(const m3g_nma_sizes* sizes, const m3g_nma_params* params, const int64_t* host_unit_offsets,
                            const int32_t* host_supercells, const double* host_lattices, const double* host_frac, const double* host_masses,
                            const int64_t* host_q_offsets, const double* host_qpoints, const double* host_eigenvectors, void* state,
                            size_t state_bytes, void* stream_) {
  const char* fn = "m3g_nma_init";
  if (const char* why = nma_error(sizes)) { set_error("%s: %s", fn, why); return M3G_ERR_VALUE; }
  if (!params_ok(params)) { set_error("%s: null parameters, or remove_com not 0 or 1", fn); return M3G_ERR_VALUE; }
  if (!host_unit_offsets || !host_supercells || !host_lattices || !host_frac || !host_masses || !host_q_offsets || !host_qpoints ||
      !host_eigenvectors || !state) {
    set_error("%s: null argument", fn);
    return M3G_ERR_VALUE;
  }
  const int64_t N = sizes->n_atoms, S = sizes->n_structs, U = sizes->n_unit_atoms, Q = sizes->n_qpoints;
  if (!offsets_ok(fn, host_unit_offsets, U, S, "unit offsets", "n_unit_atoms")) return M3G_ERR_VALUE;
  if (!offsets_ok(fn, host_q_offsets, Q, S, "q offsets", "n_qpoints")) return M3G_ERR_VALUE;
  std::vector<int64_t> offsets(S + 1, 0);   // atoms of the MD supercells
  int64_t modes = 0, eig = 0, phase = 0;
  int max_n = 0;
  for (int64_t s = 0; s < S; ++s) {
    const int64_t nu = host_unit_offsets[s + 1] - host_unit_offsets[s], nq = host_q_offsets[s + 1] - host_q_offsets[s];
    if (3 * nu > sizes->max_n) { set_error("%s: structure %lld has 3 n_u = %lld above max_n = %d", fn, (long long)s, (long long)(3 * nu), (int)sizes->max_n); return M3G_ERR_VALUE; }
    int64_t cells = 1;
    for (int k = 0; k < 3; ++k) {
      const int64_t c = host_supercells[3 * s + k];
      if (c < 1 || cells * c > INT32_MAX) { set_error("%s: supercell of structure %lld must be >= 1 and hold fewer than 2^31 cells", fn, (long long)s); return M3G_ERR_VALUE; }
      cells *= c;
    }
    if (!lattice_ok(fn, host_lattices + 9 * s, s)) return M3G_ERR_VALUE;
    if (nu * cells > N) { set_error("%s: the supercells hold more than n_atoms atoms", fn); return M3G_ERR_VALUE; }
    offsets[s + 1] = offsets[s] + nu * cells;
    modes += nq * 3 * nu;
    eig += nq * 9 * nu * nu;
    phase += nq * nu * cells;
    if (3 * nu > max_n) max_n = (int)(3 * nu);
  }
  if (offsets[S] != N || modes != sizes->n_modes || eig != sizes->n_eig || phase != sizes->n_phase || max_n != sizes->max_n) {
    set_error("%s: the sizes do not follow from the offsets and supercells", fn);
    return M3G_ERR_VALUE;
  }
  for (int64_t u = 0; u < U; ++u) {
    if (!mass_ok(fn, host_masses, u, "unit atom")) return M3G_ERR_VALUE;
    for (int k = 0; k < 3; ++k)
      if (!std::isfinite(host_frac[3 * u + k])) { set_error("%s: fractional coordinate of unit atom %lld is not finite", fn, (long long)u); return M3G_ERR_VALUE; }
  }
  for (int64_t k = 0; k < 3 * Q; ++k)
    if (!std::isfinite(host_qpoints[k])) { set_error("%s: q-point %lld is not finite", fn, (long long)(k / 3)); return M3G_ERR_VALUE; }
  for (int64_t k = 0; k < 2 * eig; ++k)
    if (!std::isfinite(host_eigenvectors[k])) { set_error("%s: an eigenvector element is not finite", fn); return M3G_ERR_VALUE; }
  const auto [st, total] = nma_view(*sizes, state);
  if (!state_fits(fn, state_bytes, total, true)) return M3G_ERR_SIZE;
  // the tables from n_unit up to the accumulators, built in a host image of that part of the state and sent in one copy
  std::vector<char> image(carve_offset(nma_view(*sizes, nullptr).view.done), 0);
  const NmaView im = nma_view(*sizes, image.data()).view;
  int64_t mode_at = 0, eig_at = 0, phase_at = 0;
  for (int64_t s = 0; s < S; ++s) {
    const int64_t nu = host_unit_offsets[s + 1] - host_unit_offsets[s], ns = offsets[s + 1] - offsets[s];
    const int32_t* sc = host_supercells + 3 * s;
    const double* L = host_lattices + 9 * s;
    ((int32_t*)im.n_unit)[s] = (int32_t)nu;
    ((int32_t*)im.n_cells)[s] = (int32_t)(ns / nu);
    ((int64_t*)im.q_first)[s] = host_q_offsets[s];
    std::vector<double> f(3 * ns);
    for (int64_t j = 0; j < ns; ++j) {
      const int64_t l = j / nu, b = j % nu, i = offsets[s] + j;
      const int64_t cell[3] = {l / ((int64_t)sc[1] * sc[2]), l / sc[2] % sc[1], l % sc[2]};
      for (int k = 0; k < 3; ++k) f[3 * j + k] = host_frac[3 * (host_unit_offsets[s] + b) + k] + (double)cell[k];
      ((double*)im.mass)[i] = host_masses[host_unit_offsets[s] + b];
      for (int k = 0; k < 3; ++k) ((double*)im.r0)[3 * i + k] = (f[3 * j] * L[k] + f[3 * j + 1] * L[3 + k]) + f[3 * j + 2] * L[6 + k];
    }
    for (int64_t gq = host_q_offsets[s]; gq < host_q_offsets[s + 1]; ++gq) {
      const double* q = host_qpoints + 3 * gq;
      ((int32_t*)im.q_struct)[gq] = (int32_t)s;
      ((int64_t*)im.q_eig)[gq] = eig_at;
      ((int64_t*)im.q_phase)[gq] = phase_at;
      ((int64_t*)im.q_mode)[gq] = mode_at;
      for (int64_t j = 0; j < ns; ++j) {
        double x = (q[0] * f[3 * j] + q[1] * f[3 * j + 1]) + q[2] * f[3 * j + 2];
        x -= std::rint(x);   // exp(-2 pi i x) has period 1 in x: the argument stays within pi
        ((double2*)im.phase)[phase_at + j] = make_double2(std::cos(kTwoPi * x), -std::sin(kTwoPi * x));
      }
      eig_at += 9 * nu * nu;
      phase_at += ns;
      mode_at += 3 * nu;
    }
  }
  std::memcpy((void*)im.eig, host_eigenvectors, 16 * (size_t)eig);
  hipStream_t s = (hipStream_t)stream_;
  M3G_HIP_CHECK(hipMemsetAsync(st.done, 0, (size_t)((const char*)st.part - (const char*)st.done), s));
  return upload_image(image, state, st.n_unit, st.done, st.ch, offsets.data(), s);
}

extern "C" int m3g_nma_sample(const m3g_nma_sizes* sizes, const m3g_nma_params* params, void* state, size_t state_bytes, const double* pos,
                              const double* vel, const float* forces, double kick, void* stream_) {
  if (const char* why = nma_error(sizes)) { set_error("m3g_nma_sample: %s", why); return M3G_ERR_VALUE; }
  if (!params_ok(params)) { set_error("m3g_nma_sample: null parameters, or remove_com not 0 or 1"); return M3G_ERR_VALUE; }
  if (!state || !pos || !vel) { set_error("m3g_nma_sample: null argument"); return M3G_ERR_VALUE; }
  if (forces && !std::isfinite(kick)) { set_error("m3g_nma_sample: kick must be finite"); return M3G_ERR_VALUE; }
  const auto [st, total] = nma_view(*sizes, state);
  if (!state_fits("m3g_nma_sample", state_bytes, total)) return M3G_ERR_SIZE;
  hipStream_t s = (hipStream_t)stream_;
  const dim3 chunks((unsigned)chunk_bound(sizes->n_atoms, sizes->n_structs)), per_q((unsigned)sizes->n_qpoints);
  hipLaunchKernelGGL(k_nma_com, chunks, dim3(kChunkRows), 0, s, st, pos, vel, forces, kick);   // workgroups beyond the chunk count return at once
  // one instantiation per capacity, so that a small unit cell does not pay the LDS footprint of the largest (as m3g_eigh.hip)
  if (sizes->max_n <= 12)
    hipLaunchKernelGGL(k_nma_project<12>, per_q, dim3(kChunkRows), 0, s, st, params->remove_com, pos, vel, forces, kick);
  else if (sizes->max_n <= 30)
    hipLaunchKernelGGL(k_nma_project<30>, per_q, dim3(kChunkRows), 0, s, st, params->remove_com, pos, vel, forces, kick);
  else
    hipLaunchKernelGGL(k_nma_project<kMaxN>, per_q, dim3(kChunkRows), 0, s, st, params->remove_com, pos, vel, forces, kick);
  const int64_t pairs = (int64_t)sizes->max_n * sizes->n_lags;
  hipLaunchKernelGGL(k_nma_accumulate, dim3(per_q.x, (unsigned)(pairs ? (pairs + kChunkRows - 1) / kChunkRows : 1)), dim3(kChunkRows), 0, s, st);
  M3G_RETURN_LAUNCH_STATUS();
}

extern "C" int m3g_nma_read(const m3g_nma_sizes* sizes, const void* state, size_t state_bytes, int64_t* host_n_samples, double* host_kinetic_sum,
                            double* host_qdot2_sum, double* host_q2_sum, double* host_acf, int64_t* host_lag_count, int32_t* host_flags,
                            void* stream_) {
  if (const char* why = nma_error(sizes)) { set_error("m3g_nma_read: %s", why); return M3G_ERR_VALUE; }
  if (!state) { set_error("m3g_nma_read: null argument"); return M3G_ERR_VALUE; }
  const auto [st, total] = nma_view(*sizes, (void*)state);
  if (!state_fits("m3g_nma_read", state_bytes, total)) return M3G_ERR_SIZE;
  const size_t S = sizes->n_structs, M = sizes->n_modes, G = sizes->n_lags;
  return read_all((hipStream_t)stream_,
                  {rb(host_n_samples, st.done, S), rb(host_kinetic_sum, st.kinetic_sum, S), rb(host_qdot2_sum, st.qdot2_sum, M),
                   rb(host_q2_sum, st.q2_sum, M), rb((double2*)host_acf, st.acf, M * G), rb(host_lag_count, st.lag_count, S * G),
                   rb(host_flags, st.flags, S)});
}

extern "C" int m3g_nma_frame(const m3g_nma_sizes* sizes, const void* state, size_t state_bytes, double* host_qdot, double* host_q,
                             void* stream_) {
  if (const char* why = nma_error(sizes)) { set_error("m3g_nma_frame: %s", why); return M3G_ERR_VALUE; }
  if (!state || !host_qdot || !host_q) { set_error("m3g_nma_frame: null argument"); return M3G_ERR_VALUE; }
  const auto [st, total] = nma_view(*sizes, (void*)state);
  if (!state_fits("m3g_nma_frame", state_bytes, total)) return M3G_ERR_SIZE;
  return read_all((hipStream_t)stream_,
                  {rb((double2*)host_qdot, st.last_qdot, sizes->n_modes), rb((double2*)host_q, st.last_q, sizes->n_modes)});
}
