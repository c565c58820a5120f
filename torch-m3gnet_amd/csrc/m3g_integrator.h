// The layer under the five MD step families that advance velocities and positions on the device: m3g_dynamics.hip (m3g_dyn_*),
// m3g_nhc.hip, m3g_mtk.hip, m3g_pimd.hip and m3g_ti.hip -- and only those five include it (m3g_remd.hip, m3g_mc.hip and
// m3g_rnemd.hip work on the state of m3g_dyn_* and include m3g_dyn_state.h alone).  All five have the same skeleton: a carved state
// view; k_*_init, k_*_partials, k_*_finalize, k_*_apply; the C entry points state_bytes, state_view, init, step, read.  Here is one
// copy of what they spell alike: on the device the Box-Muller draw, the row prologue, verdict and epilogue of the partials kernels,
// the 8-sum partials body of m3g_dyn_* and m3g_nhc_*, the cell volume and tr W; on the host what only the integrators have: the
// upload of a batch, the offsets of state_view, the grids of a step and the head of read.  (The checks of init, the size check of
// a state buffer and the tail of an init are shared with the eleven drivers that do not integrate: m3g_chunks.h, which this
// header reaches through m3g_dyn_state.h.)  Everything a family does on
// its own stays in its file, and so does an idiom where the shared copy would change a kernel's vector instructions or registers:
// the compiler's listing decides (profiles/integrator_layer.txt names each).
// Contraction: unlike m3g_chunks.h ("no device function here multiplies") the device helpers below do multiply.  That rule is about
// kernels that switch floating-point contraction off lexically; none of the five units has one.  So: these helpers may be called
// only from kernels compiled in the default contraction mode, where they round as the same text did inside the kernel.
#pragma once
#include "m3g_dyn_state.h"

namespace m3g {
// The second Philox key word, (seed, word), keeps the streams of one seed apart.  Who owns which:
//   0  the Langevin O step of m3g_dyn_*   (k_dyn_apply; counter: start, atom)
//   1  replica exchange                   (m3g_remd.hip, its own draw)
//   2  swap Monte Carlo                   (m3g_mc.hip, its own draw)
//   3  path integrals                     (k_pimd_apply; counter: start, atom, mode)
//   4  thermodynamic integration          (k_ti_partials and k_ti_apply; counter: start, atom)
constexpr uint64_t kLangevinKey = 0, kPimdKey = 3, kTiKey = 4;

// three standard normals: Box-Muller on the Philox block of counter (c0, c1, c2, 0) under key (seed, key1)
__device__ inline void gaussian3(uint64_t seed, uint64_t key1, uint64_t c0, uint64_t c1, uint64_t c2, double xi[3]) {
  uint64_t c[4] = {c0, c1, c2, 0};
  philox4x64_10(c, seed, key1);
  const double r0 = sqrt(-2.0 * log(uniform53(c[0]))), r1 = sqrt(-2.0 * log(uniform53(c[2])));
  xi[0] = r0 * cos(kTwoPi * uniform53(c[1]));
  xi[1] = r0 * sin(kTwoPi * uniform53(c[1]));
  xi[2] = r1 * cos(kTwoPi * uniform53(c[3]));
}

// ---- k_*_partials: one workgroup per chunk ---------------------------------------------------------------------------------------
// Where thread t of chunk c works: row i of structure s, whose flags are fl.  `live` is false for a chunk past the table and for a
// frozen structure (finalize reads nothing of it): the whole workgroup returns.  `holds`: a structure's last chunk may be part-filled.
struct ChunkRow { bool live; int s, fl; int64_t i; bool holds; };
template <class View>
__device__ inline ChunkRow chunk_row(const View& st, int c, int t) {
  if (c >= st.ch.n_chunks()) return {false};
  const int s = st.ch.structure(c);
  const int fl = st.flags[s];
  if (fl & M3G_DYN_ERROR) return {false};
  const int64_t i = st.ch.row(c, t);
  return {true, s, fl, i, st.ch.holds(s, i)};
}

__device__ inline bool forces_finite(const double (&f)[3]) { return std::isfinite(f[0]) && std::isfinite(f[1]) && std::isfinite(f[2]); }

// the K sums of chunk c, thread t contributing val[], in the fixed tree order, into the chunk's K words of `partial` ([chunk][K])
template <int K>
__device__ inline void reduce_store(const double (&val)[K], int c, int t, double* partial) {
  __shared__ double sh[K][kChunkRows];
  chunk_tree_reduce<K>(sh, val, t);
  if (t < K) partial[K * c + t] = sh[t][0];
}

// The partials of m3g_dyn_* and m3g_nhc_* (kPart): sum m |v|^2, sum m v, sum F and the non-finite count over the finish-kicked
// velocities.  `kick(s, v, f, m)`: the family's finish kick of one component, the velocity k_*_apply left and the force on it.
template <class View, class Kick>
__device__ inline void md_partials(const View& st, const float* __restrict__ forces, Kick kick) {
  const int c = blockIdx.x, t = threadIdx.x;
  const ChunkRow at = chunk_row(st, c, t);
  if (!at.live) return;
  const int64_t i = at.i;
  double val[kPart] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (at.holds) {
    const double m = st.mass[i];
    double f[3], v[3];
    for (int k = 0; k < 3; ++k) {
      f[k] = forces[3 * i + k];
      v[k] = st.v[3 * i + k];
      if (at.fl & M3G_DYN_STARTED) v[k] = kick(at.s, v[k], f[k], m);
    }
    val[0] = m * (v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    for (int k = 0; k < 3; ++k) {
      val[1 + k] = m * v[k];
      val[4 + k] = f[k];
    }
    val[7] = forces_finite(f) ? 0.0 : 1.0;
  }
  reduce_store<kPart>(val, c, t, st.partial);
}

// ---- k_*_finalize: one wave per structure ----------------------------------------------------------------------------------------
// The opening of the five finalize kernels (structure of the wave, frozen early-out that clears the action word, wave_chunk_sum) is
// NOT here: as a function it changes the register allocation of four of them (profiles/integrator_layer.txt), so each keeps its text.
// |det L|, rows = lattice vectors
__device__ inline double cell_volume(const double* L) {
  return fabs(L[0] * (L[4] * L[8] - L[5] * L[7]) - L[1] * (L[3] * L[8] - L[5] * L[6]) + L[2] * (L[3] * L[7] - L[4] * L[6]));
}
// tr W, W = V * stresses (sv: one structure's six, Voigt)
__device__ inline double virial_trace(double vol, const float* sv) { return vol * (((double)sv[0] + (double)sv[1]) + (double)sv[2]); }

// ---- the C entry points (host) ---------------------------------------------------------------------------------------------------
// (The checks of init, state_fits and launched_and_synced are in m3g_chunks.h, shared with the drivers that do not integrate.)
// Queues the chunk table, the masses [N], the temperatures [S of the table] and, where the view has seeds, those.  Asynchronous
// copies from the caller's arrays and from `table`: keep them alive until the stream has been synchronised.
template <class View>
inline int upload_batch(const ChunkTable& table, const View& st, const int64_t* host_offsets, const double* host_masses,
                        const double* host_temperatures, const uint64_t* host_seeds, hipStream_t s) {
  if (int rc = table.upload(st.ch, host_offsets, s)) return rc;
  M3G_HIP_CHECK(hipMemcpyAsync(st.mass, host_masses, 8 * st.N, hipMemcpyHostToDevice, s));
  M3G_HIP_CHECK(hipMemcpyAsync(st.t0, host_temperatures, 8 * st.ch.S, hipMemcpyHostToDevice, s));
  if constexpr (requires { st.seed; }) M3G_HIP_CHECK(hipMemcpyAsync(st.seed, host_seeds, 8 * st.ch.S, hipMemcpyHostToDevice, s));
  return M3G_OK;
}

// m3g_*_state_view: the (mass, velocity) byte offsets of the view `carve()` returns, carved over a null state once `sizes_ok`
template <class CarveView>
inline int state_view_offsets(const char* fn, bool sizes_ok, CarveView carve, size_t* mass_offset, size_t* velocity_offset) {
  if (!mass_offset || !velocity_offset || !sizes_ok) { set_error("%s: null argument or bad sizes", fn); return M3G_ERR_VALUE; }
  const auto at = carve();
  *mass_offset = carve_offset(at.mass);
  *velocity_offset = carve_offset(at.v);
  return M3G_OK;
}

// The two grids of a step over N atoms in S structures (rings): `chunks` for the row kernels, kChunkRows threads each (workgroups
// beyond the table's chunk count return at once), `waves` for finalize, kFinalizeWaves waves each.
struct StepGrids { dim3 chunks, waves; };
inline StepGrids step_grids(int64_t N, int64_t S) { return {dim3((unsigned)chunk_bound(N, S)), grid_for(S, kFinalizeWaves)}; }
constexpr int kFinalizeThreads = kWave * kFinalizeWaves;

// the head of m3g_*_read: flags and step counts [S of the table], velocities [N, 3] (queued: the caller synchronises)
template <class View>
inline int read_head(const View& st, int32_t* host_flags, int64_t* host_steps, double* host_vel, hipStream_t s) {
  M3G_HIP_CHECK(read_back(host_flags, st.flags, st.ch.S, s));
  M3G_HIP_CHECK(read_back(host_steps, st.steps, st.ch.S, s));
  M3G_HIP_CHECK(read_back(host_vel, st.v, 3 * st.N, s));
  return M3G_OK;
}
}  // namespace m3g
