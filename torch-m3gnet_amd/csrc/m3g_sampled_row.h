// What the samplers that complete the integrator's half-step velocities share on the device (m3g_trajectory.hip, m3g_scattering.hip):
// the sampled row itself and the chunk partials of the centre of mass, as inline device functions over the chunk table of
// m3g_chunks.h.  Each unit keeps its own kernel around com_chunk_partials and its own state view.
#pragma once
#include "m3g_chunks.h"

namespace m3g {
constexpr int kComPart = 7;   // per chunk: sum m, sum m r [3], sum m v [3]

// position and full-step velocity of row i: v + kick kappa F / m, the finish kick of k_dyn_apply (m3g_dynamics.hip)
__device__ inline void sampled_row(const double* __restrict__ mass, int64_t i, const double* __restrict__ pos, const double* __restrict__ vel,
                                   const float* __restrict__ forces, double kick, double (&r)[3], double (&v)[3]) {
  const double m = mass[i];
  for (int k = 0; k < 3; ++k) {
    r[k] = pos[3 * i + k];
    v[k] = vel[3 * i + k];
    if (forces) v[k] += kick * (kKappa * (double)forces[3 * i + k] / m);
  }
}

// The body of a centre-of-mass kernel, one workgroup of kChunkRows threads per chunk: the partial sums of m, m r and m v over the
// chunk's rows in the fixed tree order, into com[kComPart * chunk ..].
__device__ inline void com_chunk_partials(const ChunkView& ch, const double* __restrict__ mass, double* __restrict__ com,
                                          const double* __restrict__ pos, const double* __restrict__ vel, const float* __restrict__ forces,
                                          double kick) {
  __shared__ double sh[kComPart][kChunkRows];
  const int c = blockIdx.x, t = threadIdx.x;
  if (c >= ch.n_chunks()) return;
  const int s = ch.structure(c);
  const int64_t i = ch.row(c, t);
  double val[kComPart] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (ch.holds(s, i)) {
    double r[3], v[3];
    sampled_row(mass, i, pos, vel, forces, kick, r, v);
    const double m = mass[i];
    val[0] = m;
    for (int k = 0; k < 3; ++k) {
      val[1 + k] = m * r[k];
      val[4 + k] = m * v[k];
    }
  }
  chunk_tree_reduce<kComPart>(sh, val, t);
  if (t < kComPart) com[kComPart * c + t] = sh[t][0];
}
}  // namespace m3g
