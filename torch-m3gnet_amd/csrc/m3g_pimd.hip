// Batched path-integral molecular dynamics: ring polymers of P beads under the PILE-L thermostat (Ceriotti, Parrinello, Markland,
// Manolopoulos, J. Chem. Phys. 133, 124104 (2010)), integrated BAOAB (Liu, Li, Liu, J. Chem. Phys. 145, 024103 (2016)).  A fourth MD
// family beside m3g_dynamics.hip, m3g_nhc.hip and m3g_mtk.hip, on the same layers (the chunk table of m3g_chunks.h, the constants and
// the generator of m3g_dyn_state.h).  The S = R P structures of the batch are R rings laid out ring by ring: bead j of ring g is
// structure g P + j, all beads of a ring with the same atoms.  The chunk table is built over RINGS (R entries of n atoms): a workgroup
// owns up to kChunkRows atoms of one ring and thread t walks its atom through the P beads, whose rows lie n apart.
// One step is B(h) A(h) O(dt) A(h) [forces] B(h), h = dt / 2: B the kick of every bead by the full force, A the exact evolution of the
// free ring polymer and O the Langevin thermostat, both in the ring's normal modes.  One call -- finish step k, observables, start
// step k+1 -- is three launches for the whole batch, as m3g_dyn_step:
//   k_pimd_partials  one workgroup per ring chunk: the finish kick in registers; per thread a fixed ascending walk over the beads
//                    (the centroid first), then the chunk sums of m |v|^2, m |q_j - q_j+1|^2, (q - centroid) . F and the non-finite
//                    count, in a fixed tree order;
//   k_pimd_finalize  one wave per ring: the chunk partials in chunk order, the error verdict, the heat partials the previous call's
//                    apply left, the observables row;
//   k_pimd_apply     one workgroup per ring chunk: finish kick, B, the transform to normal modes, A O A, the transform back, and the
//                    chunk's share of the kinetic energy the thermostat added, for the next finalize.
// The transform is the direct O(P^2) product with the [P,P] table (any P in 1 .. 64), the table in LDS and one component's beads in
// registers.  Its two directions work IN PLACE on the thread's own rows of pos and of the velocities: every value of a component is
// in registers before the first is written, and no other thread touches the rows of this atom.  So between the forward and the
// inverse pass those rows hold normal-mode coordinates, and the mode loop in between draws the noise of (atom, mode) once for the
// three components.  x and v go through the table one after the other: P fp64 values live, not 2 P.
// No atomics: every result depends on the ring's own rows only, so it is bitwise the same alone or in any batch.  No allocation,
// copy or wait in m3g_pimd_step (capture-safe).  The Box-Muller draw and its key word, the row prologue, verdict and epilogue of the
// partials and the checks and copies of the entry points are m3g_integrator.h.
#include <cmath>
#include <vector>

#include "m3g_integrator.h"

namespace m3g {
namespace {
constexpr double kHbar = 0.6582119569;   // eV fs
constexpr int kPimdPart = 4;    // per chunk: sum m |v|^2, sum m |q_j - q_j+1|^2, sum (q - centroid) . F, non-finite forces
constexpr int kPimdMode = 5;    // per ring and mode: cos(w h), sin(w h) / w, w sin(w h), c1, c2
enum PimdAct : int32_t { kActNone = 0, kActFinishOnly = 1, kActStep = 2, kActFinishKick = 4 };   // action | finish kick?

struct PimdView {
  int64_t N;
  int P;
  ChunkView ch;   // over rings: S = R, offsets = the rings' atom offsets (N / P in all)
  double *partial, *heat_part, *mass, *v, *t0, *heat, *table, *mode;
  uint64_t* seed;
  int32_t *flags, *act;
  int64_t* steps;
};
inline Carved<PimdView> pimd_view(int64_t N, int64_t S, int P, void* state) {
  Carve c{state};
  PimdView st{N, P};
  const int64_t R = S / P, Nr = N / P;
  st.ch = chunk_view(Nr, R, c);
  st.partial = c.take<double>(kPimdPart * chunk_bound(Nr, R));
  st.heat_part = c.take<double>(chunk_bound(Nr, R));
  st.mass = c.take<double>(N);
  st.v = c.take<double>(3 * N);
  st.t0 = c.take<double>(R);
  st.seed = c.take<uint64_t>(R);
  st.flags = c.take<int32_t>(R);
  st.act = c.take<int32_t>(R);
  st.steps = c.take<int64_t>(R);
  st.heat = c.take<double>(R);
  st.table = c.take<double>((size_t)P * P);
  st.mode = c.take<double>((size_t)kPimdMode * P * R);
  return {st, c.off};
}

// where the thread on row i of ring g's table works: atom `local` of the ring, whose bead j is row first + j n of the batch
struct RingRow {
  bool holds;
  int64_t first, n, local;
};
__device__ inline RingRow ring_row(const PimdView& st, int g, int64_t i) {
  const int64_t o = st.ch.offsets[g];
  return {st.ch.holds(g, i), st.P * o + (i - o), st.ch.offsets[g + 1] - o, i - o};
}

__global__ void __launch_bounds__(kChunkRows) k_pimd_init(PimdView st, int64_t chunks, const double* __restrict__ vel) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < 3 * st.N) st.v[i] = vel[i];
  if (i < st.ch.S) {
    st.flags[i] = 0;
    st.act[i] = kActNone;
    st.steps[i] = 0;
    st.heat[i] = 0.0;
  }
  if (i < chunks) st.heat_part[i] = 0.0;
}

__global__ void __launch_bounds__(kChunkRows) k_pimd_partials(PimdView st, double half_dt, const float* __restrict__ forces,
                                                              const double* __restrict__ pos) {
  const int c = blockIdx.x, t = threadIdx.x;
  const ChunkRow row = chunk_row(st, c, t);
  if (!row.live) return;
  const int fl = row.fl;
  const RingRow at = ring_row(st, row.s, row.i);
  double val[kPimdPart] = {0.0, 0.0, 0.0, 0.0};
  if (at.holds) {
    const int P = st.P;
    const double m = st.mass[at.first];
    double mean[3] = {0.0, 0.0, 0.0}, q0[3], prev[3];
    for (int j = 0; j < P; ++j)
      for (int k = 0; k < 3; ++k) mean[k] += pos[3 * (at.first + j * at.n) + k];
    for (int k = 0; k < 3; ++k) mean[k] /= (double)P;
    double v2 = 0.0, d2 = 0.0, qf = 0.0, bad = 0.0;
    for (int j = 0; j < P; ++j) {
      const int64_t i = at.first + j * at.n;
      double f[3], q[3];
      for (int k = 0; k < 3; ++k) {
        f[k] = forces[3 * i + k];
        q[k] = pos[3 * i + k];
        double v = st.v[3 * i + k];
        if (fl & M3G_DYN_STARTED) v += half_dt * (kKappa * f[k] / m);   // the finish kick (written by k_pimd_apply)
        v2 += v * v;
        qf += (q[k] - mean[k]) * f[k];
        if (j == 0) q0[k] = q[k];
        else d2 += (q[k] - prev[k]) * (q[k] - prev[k]);
        prev[k] = q[k];
      }
      if (!forces_finite(f)) bad += 1.0;
    }
    for (int k = 0; k < 3; ++k) d2 += (q0[k] - prev[k]) * (q0[k] - prev[k]);   // the bond that closes the ring (0 when P = 1)
    val[0] = m * v2;
    val[1] = m * d2;
    val[2] = qf;
    val[3] = bad;
  }
  reduce_store<kPimdPart>(val, c, t, st.partial);
}

__global__ void __launch_bounds__(kWave * kFinalizeWaves) k_pimd_finalize(PimdView st, int32_t finish_only, double* __restrict__ obs) {
  const int lane = threadIdx.x % kWave;
  const int64_t g = (int64_t)blockIdx.x * kFinalizeWaves + threadIdx.x / kWave;
  if (g >= st.ch.S) return;   // (whole waves: g is uniform across a wave)
  const int fl = st.flags[g];
  if (fl & M3G_DYN_ERROR) {
    if (lane == 0) st.act[g] = kActNone;
    return;
  }
  double acc[kPimdPart], added[1];
  wave_chunk_sum<kPimdPart>(st.ch, g, st.partial, lane, acc);
  wave_chunk_sum<1>(st.ch, g, st.heat_part, lane, added);
  if (lane != 0) return;
  if (acc[3] != 0.0) {   // never move a ring with a non-finite force on any bead
    st.flags[g] = fl | M3G_DYN_ERROR;
    st.act[g] = kActNone;
    return;
  }
  const double n = (double)(st.ch.offsets[g + 1] - st.ch.offsets[g]), P = (double)st.P;
  const double kt = kBoltzmann * st.t0[g], wp = P * kt / kHbar;
  const double heat = st.heat[g] + added[0] / (2.0 * kKappa);
  st.heat[g] = heat;
  const double ke = acc[0] / (2.0 * kKappa);
  const double spring = wp * wp * acc[1] / (2.0 * kKappa);
  if (obs) {
    double* o = obs + M3G_PIMD_OBS * g;
    o[0] = ke;
    o[1] = 2.0 * ke / (3.0 * n * P * P * kBoltzmann);
    o[2] = spring;
    o[3] = 1.5 * n * P * kt - spring / P;
    o[4] = 1.5 * n * kt - acc[2] / (2.0 * P);
    o[5] = heat;
    o[6] = 0.0;
    o[7] = 0.0;
  }
  const int kick = (fl & M3G_DYN_STARTED) ? kActFinishKick : 0;
  if (finish_only) {
    st.flags[g] = fl & ~M3G_DYN_STARTED;
    st.act[g] = kActFinishOnly | kick;
    return;
  }
  st.act[g] = kActStep | kick;
  st.flags[g] = fl | M3G_DYN_STARTED;
  st.steps[g] += 1;
}

// One component of an atom through the table, in place: out_r = sum_i tab[i * kSumStride + r * kOutStride] u_i over the P rows
// (`stride` doubles apart) behind `a`, u_i = load(i).  Every u is in registers before the first row is written.  The register row
// is loaded without a branch, so that its loads are all in flight together: beyond P it holds row P - 1 again, against the zeros
// of the table.
template <int PB, int kSumStride, int kOutStride, class Load>
__device__ inline void ring_product(const double* tab, int P, Load load, double* a, int64_t stride) {
  double u[PB];
#pragma unroll
  for (int i = 0; i < PB; ++i) u[i] = load(i < P ? i : P - 1);
  for (int r = 0; r < P; ++r) {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < PB; ++i) s += tab[i * kSumStride + r * kOutStride] * u[i];
    a[r * stride] = s;
  }
}

// PB: the bead-count bucket (P <= PB), the size of the register row and of the LDS table's side
template <int PB>
__global__ void __launch_bounds__(kChunkRows) k_pimd_apply(PimdView st, int32_t thermostat, double h, const float* __restrict__ forces,
                                                           double* pos) {
  __shared__ double tab[PB * PB];   // tab[j * PB + k] = C[j][k], zero beyond P
  __shared__ double sh[1][kChunkRows];
  const int c = blockIdx.x, t = threadIdx.x;
  if (c >= st.ch.n_chunks()) return;
  const int g = st.ch.structure(c);
  const int act = st.act[g];
  if (act == kActNone) return;   // failed: bitwise untouched (the whole workgroup: act is the ring's)
  const int P = st.P;
  const bool kick = act & kActFinishKick, step = act & kActStep;
  if (step) {
    for (int i = t; i < PB * PB; i += kChunkRows) {
      const int j = i / PB, k = i % PB;
      tab[i] = (j < P && k < P) ? st.table[j * P + k] : 0.0;
    }
    __syncthreads();
  }
  const RingRow at = ring_row(st, g, st.ch.row(c, t));
  double added[1] = {0.0};
  if (at.holds) {
    const double m = st.mass[at.first];
    const int64_t stride = 3 * at.n;
    // the velocity of bead j, component k, after the finish kick and (a step) the opening B(h)
    auto kicked = [&](int j, int k) {
      const int64_t i = 3 * (at.first + j * at.n) + k;
      const double a = kKappa * (double)forces[i] / m;
      double v = st.v[i];
      if (kick) v += h * a;
      if (step) v += h * a;
      return v;
    };
    if (!step) {   // finish only
      for (int j = 0; j < P; ++j)
        for (int k = 0; k < 3; ++k) st.v[3 * (at.first + j * at.n) + k] = kicked(j, k);
    } else {
      double* x = pos + 3 * at.first;
      double* v = st.v + 3 * at.first;
#pragma unroll 1
      for (int k = 0; k < 3; ++k) {   // to normal modes: row k' of this atom now holds mode k'
        ring_product<PB, PB, 1>(tab, P, [&](int j) { return x[j * stride + k]; }, x + k, stride);
        ring_product<PB, PB, 1>(tab, P, [&](int j) { return kicked(j, k); }, v + k, stride);
      }
      const double* mode = st.mode + (size_t)kPimdMode * P * g;
      const double sigma = sqrt(P * kBoltzmann * st.t0[g] * kKappa / m);
      const uint64_t seed = st.seed[g], start = (uint64_t)(st.steps[g] - 1);
      for (int w = 0; w < P; ++w) {   // A(h) O(dt) A(h) of mode w
        const double cs = mode[w], sw = mode[P + w], ws = mode[2 * P + w], c1 = mode[3 * P + w], c2 = mode[4 * P + w];
        double xi[3] = {0.0, 0.0, 0.0};
        if (thermostat == M3G_PIMD_PILE_L) gaussian3(seed, kPimdKey, start, (uint64_t)at.local, (uint64_t)w, xi);
        for (int k = 0; k < 3; ++k) {
          double xm = x[w * stride + k], vm = v[w * stride + k];
          for (int half = 0; half < 2; ++half) {
            if (w == 0) {
              xm += h * vm;
            } else {
              const double x1 = cs * xm + sw * vm;
              vm = cs * vm - ws * xm;
              xm = x1;
            }
            if (half == 0 && thermostat == M3G_PIMD_PILE_L) {
              const double v1 = c1 * vm + c2 * sigma * xi[k];
              added[0] += m * (v1 * v1 - vm * vm);
              vm = v1;
            }
          }
          x[w * stride + k] = xm;
          v[w * stride + k] = vm;
        }
      }
#pragma unroll 1
      for (int k = 0; k < 3; ++k) {   // back to beads
        ring_product<PB, 1, PB>(tab, P, [&](int w) { return x[w * stride + k]; }, x + k, stride);
        ring_product<PB, 1, PB>(tab, P, [&](int w) { return v[w * stride + k]; }, v + k, stride);
      }
    }
  }
  chunk_tree_reduce<1>(sh, added, t);
  if (t == 0) st.heat_part[c] = sh[0][0];
}

// nullptr when the parameters are valid, else what is wrong with them
const char* pimd_params_error(const m3g_pimd_params* p) {
  if (!p) return "null parameters";
  if (p->thermostat != M3G_PIMD_NONE && p->thermostat != M3G_PIMD_PILE_L) return "unknown thermostat";
  if (p->n_beads < 1 || p->n_beads > M3G_PIMD_MAX_BEADS) return "n_beads must be in 1 .. 64";
  if (!finite_positive(p->dt)) return "dt must be finite and > 0";
  if (!(std::isfinite(p->centroid_friction) && p->centroid_friction >= 0.0)) return "centroid_friction must be finite and >= 0";
  if (!(std::isfinite(p->pile_lambda) && p->pile_lambda >= 0.0)) return "pile_lambda must be finite and >= 0";
  return nullptr;
}

// S structures of N atoms as rings of P beads
bool ring_sizes_ok(int64_t N, int64_t S, int P) {
  return batch_sizes_ok(N, S) && P >= 1 && P <= M3G_PIMD_MAX_BEADS && S % P == 0 && N % P == 0;
}
}  // namespace
}  // namespace m3g

using namespace m3g;

extern "C" int m3g_pimd_state_bytes(int64_t n_atoms, int64_t n_structs, int32_t n_beads, size_t* bytes) {
  if (!bytes || !ring_sizes_ok(n_atoms, n_structs, n_beads)) {
    set_error("m3g_pimd_state_bytes: bad sizes (n_beads must be in 1 .. 64 and divide n_structs and n_atoms)");
    return M3G_ERR_VALUE;
  }
  *bytes = pimd_view(n_atoms, n_structs, n_beads, nullptr).bytes;
  return M3G_OK;
}

extern "C" int m3g_pimd_state_view(int64_t n_atoms, int64_t n_structs, int32_t n_beads, size_t* mass_offset, size_t* velocity_offset) {
  return state_view_offsets("m3g_pimd_state_view", ring_sizes_ok(n_atoms, n_structs, n_beads),
                            [&] { return pimd_view(n_atoms, n_structs, n_beads, nullptr).view; }, mass_offset, velocity_offset);
}

extern "C" int m3g_pimd_init(const m3g_pimd_params* p, int64_t n_atoms, int64_t n_structs, const int64_t* host_offsets, const double* host_masses,
                             const double* host_temperatures, const uint64_t* host_seeds, const double* vel, void* state, size_t state_bytes,
                             void* stream_) {
  if (const char* why = pimd_params_error(p)) { set_error("m3g_pimd_init: invalid parameters: %s", why); return M3G_ERR_VALUE; }
  constexpr const char* fn = "m3g_pimd_init";
  const int64_t N = n_atoms, S = n_structs;
  if (!init_args_ok(fn, N, S, host_offsets && host_masses && host_temperatures && host_seeds && vel && state)) return M3G_ERR_VALUE;
  const int P = p->n_beads;
  if (S % P != 0) { set_error("m3g_pimd_init: n_structs (%lld) is not a multiple of n_beads (%d)", (long long)S, P); return M3G_ERR_VALUE; }
  if (!offsets_ok(fn, host_offsets, N, S)) return M3G_ERR_VALUE;
  for (int64_t i = 0; i < N; ++i)
    if (!mass_ok(fn, host_masses, i)) return M3G_ERR_VALUE;
  const int64_t R = S / P;
  std::vector<int64_t> ring_offsets(R + 1, 0);
  for (int64_t g = 0; g < R; ++g) {
    const int64_t first = host_offsets[g * P], n = host_offsets[g * P + 1] - first;
    for (int j = 1; j < P; ++j) {
      const int64_t o = host_offsets[g * P + j];
      if (host_offsets[g * P + j + 1] - o != n) {
        set_error("m3g_pimd_init: bead %d of ring %lld holds another atom count than bead 0", j, (long long)g);
        return M3G_ERR_VALUE;
      }
      for (int64_t a = 0; a < n; ++a)
        if (host_masses[o + a] != host_masses[first + a]) {
          set_error("m3g_pimd_init: bead %d of ring %lld holds other masses than bead 0", j, (long long)g);
          return M3G_ERR_VALUE;
        }
    }
    if (!temperature_ok(fn, host_temperatures, g, "ring")) return M3G_ERR_VALUE;   // (the spring constant and the noise are proportional to it)
    ring_offsets[g + 1] = ring_offsets[g] + n;
  }
  const auto [st, total] = pimd_view(N, S, P, state);
  if (!state_fits(fn, state_bytes, total, true)) return M3G_ERR_SIZE;
  // the orthogonal matrix C[j][k] of the normal modes and, per ring, the coefficients of A(h) and O(dt) of every mode
  std::vector<double> table((size_t)P * P), mode((size_t)kPimdMode * P * R);
  const double h = 0.5 * p->dt;
  for (int j = 0; j < P; ++j)
    for (int k = 0; k < P; ++k) {
      const double arg = 2.0 * M_PI * (double)((j * k) % P) / (double)P;
      double c;
      if (k == 0) c = std::sqrt(1.0 / P);
      else if (2 * k < P) c = std::sqrt(2.0 / P) * std::cos(arg);
      else if (2 * k == P) c = std::sqrt(1.0 / P) * (j % 2 ? -1.0 : 1.0);
      else c = std::sqrt(2.0 / P) * std::sin(arg);
      table[(size_t)j * P + k] = c;
    }
  for (int64_t g = 0; g < R; ++g) {
    const double wp = P * kBoltzmann * host_temperatures[g] / kHbar;
    double* row = mode.data() + (size_t)kPimdMode * P * g;
    for (int k = 0; k < P; ++k) {
      const double w = 2.0 * wp * std::sin(k * M_PI / P);
      const double gamma = k == 0 ? p->centroid_friction : 2.0 * p->pile_lambda * w;
      const double c1 = std::exp(-gamma * p->dt);
      row[k] = std::cos(w * h);
      row[P + k] = k == 0 ? h : std::sin(w * h) / w;
      row[2 * P + k] = w * std::sin(w * h);
      row[3 * P + k] = c1;
      row[4 * P + k] = std::sqrt(1.0 - c1 * c1);
    }
  }
  const ChunkTable chunks(ring_offsets.data(), R);
  hipStream_t s = (hipStream_t)stream_;
  if (int rc = upload_batch(chunks, st, ring_offsets.data(), host_masses, host_temperatures, host_seeds, s)) return rc;   // (per ring)
  M3G_HIP_CHECK(hipMemcpyAsync(st.table, table.data(), 8 * table.size(), hipMemcpyHostToDevice, s));
  M3G_HIP_CHECK(hipMemcpyAsync(st.mode, mode.data(), 8 * mode.size(), hipMemcpyHostToDevice, s));
  const int64_t work = 3 * N;   // (>= R and >= the chunk bound)
  hipLaunchKernelGGL(k_pimd_init, grid_for(work, kChunkRows), dim3(kChunkRows), 0, s, st, chunk_bound(N / P, R), vel);
  return launched_and_synced(s);   // (the host tables above go out of scope)
}

extern "C" int m3g_pimd_step(const m3g_pimd_params* p, int64_t n_atoms, int64_t n_structs, void* state, size_t state_bytes, const float* forces,
                             double* pos, int32_t finish_only, double* obs, void* stream_) {
  if (const char* why = pimd_params_error(p)) { set_error("m3g_pimd_step: invalid parameters: %s", why); return M3G_ERR_VALUE; }
  const int64_t N = n_atoms, S = n_structs;
  const int P = p->n_beads;
  if (!ring_sizes_ok(N, S, P) || !state) { set_error("m3g_pimd_step: null argument or bad sizes"); return M3G_ERR_VALUE; }
  if (!forces || !pos) { set_error("m3g_pimd_step: missing forces or pos"); return M3G_ERR_VALUE; }
  const auto [st, total] = pimd_view(N, S, P, state);
  if (!state_fits("m3g_pimd_step", state_bytes, total)) return M3G_ERR_SIZE;
  hipStream_t s = (hipStream_t)stream_;
  const double h = 0.5 * p->dt;
  const auto [grid, waves] = step_grids(N / P, S / P);   // (over rings)
  hipLaunchKernelGGL(k_pimd_partials, grid, dim3(kChunkRows), 0, s, st, h, forces, pos);
  hipLaunchKernelGGL(k_pimd_finalize, waves, dim3(kFinalizeThreads), 0, s, st, finish_only, obs);
  if (P <= 8) hipLaunchKernelGGL(k_pimd_apply<8>, grid, dim3(kChunkRows), 0, s, st, p->thermostat, h, forces, pos);
  else if (P <= 16) hipLaunchKernelGGL(k_pimd_apply<16>, grid, dim3(kChunkRows), 0, s, st, p->thermostat, h, forces, pos);
  else if (P <= 32) hipLaunchKernelGGL(k_pimd_apply<32>, grid, dim3(kChunkRows), 0, s, st, p->thermostat, h, forces, pos);
  else hipLaunchKernelGGL(k_pimd_apply<64>, grid, dim3(kChunkRows), 0, s, st, p->thermostat, h, forces, pos);
  M3G_RETURN_LAUNCH_STATUS();
}

extern "C" int m3g_pimd_read(int64_t n_atoms, int64_t n_structs, int32_t n_beads, const void* state, size_t state_bytes, int32_t* host_flags,
                             int64_t* host_steps, double* host_heat, double* host_vel, void* stream_) {
  const int64_t N = n_atoms, S = n_structs;
  if (!ring_sizes_ok(N, S, n_beads) || !state) { set_error("m3g_pimd_read: null argument or bad sizes"); return M3G_ERR_VALUE; }
  const auto [st, total] = pimd_view(N, S, n_beads, (void*)state);
  if (!state_fits("m3g_pimd_read", state_bytes, total)) return M3G_ERR_SIZE;
  hipStream_t s = (hipStream_t)stream_;
  if (int rc = read_head(st, host_flags, host_steps, host_vel, s)) return rc;   // (flags and steps per ring)
  M3G_HIP_CHECK(read_back(host_heat, st.heat, S / n_beads, s));
  M3G_HIP_CHECK(hipStreamSynchronize(s));
  return M3G_OK;
}
