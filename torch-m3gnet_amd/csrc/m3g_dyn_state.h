// The device state of m3g_dyn_* (m3g_dynamics.hip) and its random generator, shared with the callers that work on that state between
// two m3g_dyn_step calls: m3g_remd.hip (the target temperatures, velocities, flags and chunk table of a replica-exchange batch) and
// m3g_mc.hip (the flags, masses and velocities of a hybrid Monte Carlo batch; its own draws use philox4x64_10 and uniform53 too).
// The five step families (m3g_dynamics.hip, m3g_nhc.hip, m3g_mtk.hip, m3g_pimd.hip, m3g_ti.hip) include it through
// m3g_integrator.h, where the Box-Muller draw over this generator, the list of its key words and what their kernels and entry
// points share now live; DynView, its sizes, Philox and uniform53 stay here.  kKappa and kBoltzmann are in m3g_chunks.h, where the
// samplers that take no dynamics state (m3g_trajectory.hip, m3g_nma.hip) find them too.
#pragma once
#include "m3g_chunks.h"
#include "m3g_internal.h"

namespace m3g {
constexpr int kPart = 8;   // per chunk: sum m|v|^2, sum m v [3], sum F [3], non-finite forces
constexpr int kCoef = 8;    // per structure: action (0 none, 1 finish only, 2 finish + start), finish?, lambda, mu, pbar [3], noise^2

struct DynView {
  int64_t N;
  ChunkView ch;
  double *partial, *mass, *v, *t0, *coef;
  uint64_t* seed;
  int32_t* flags;
  int64_t* steps;
};
inline Carved<DynView> dyn_view(int64_t N, int64_t S, void* state) {
  Carve c{state};
  DynView st{N};
  st.ch = chunk_view(N, S, c);
  st.partial = c.take<double>(kPart * chunk_bound(N, S));
  st.mass = c.take<double>(N);
  st.v = c.take<double>(3 * N);
  st.t0 = c.take<double>(S);
  st.seed = c.take<uint64_t>(S);
  st.flags = c.take<int32_t>(S);
  st.steps = c.take<int64_t>(S);
  st.coef = c.take<double>(kCoef * S);
  return {st, c.off};
}

// Philox4x64-10 (Salmon et al., SC'11; the generator of numpy.random.Philox)
__device__ inline void philox4x64_10(uint64_t c[4], uint64_t k0, uint64_t k1) {
  constexpr uint64_t M0 = 0xD2E7470EE14C6C93ull, M1 = 0xCA5A826395121157ull, W0 = 0x9E3779B97F4A7C15ull, W1 = 0xBB67AE8584CAA73Bull;
  for (int r = 0; r < 10; ++r) {
    if (r) { k0 += W0; k1 += W1; }
    const uint64_t lo0 = M0 * c[0], hi0 = __umul64hi(M0, c[0]), lo1 = M1 * c[2], hi1 = __umul64hi(M1, c[2]);
    const uint64_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
    c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
  }
}

__device__ inline double uniform53(uint64_t w) { return ((double)(w >> 11) + 0.5) * 0x1.0p-53; }
}  // namespace m3g
