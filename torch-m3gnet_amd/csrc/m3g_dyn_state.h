// The device state of m3g_dyn_* (m3g_dynamics.hip) and its random generator, shared with the callers that work on that state between
// two m3g_dyn_step calls (m3g_remd.hip: the target temperatures, velocities, flags and chunk table of a replica-exchange batch).
#pragma once
#include "m3g_chunks.h"
#include "m3g_internal.h"

namespace m3g {
constexpr double kKappa = 9.648533215665e-3;   // A/fs^2 per eV/(A amu)
constexpr double kBoltzmann = 8.617333262e-5;  // eV/K
constexpr int kPart = 8;    // per chunk: sum m|v|^2, sum m v [3], sum F [3], non-finite forces
constexpr int kCoef = 8;    // per structure: action (0 none, 1 finish only, 2 finish + start), finish?, lambda, mu, pbar [3], noise^2

struct DynLayout {
  ChunkLayout chunks;
  size_t partial, mass, v, t0, seed, flags, steps, coef, total;
};
inline DynLayout dyn_layout(int64_t N, int64_t S) {
  DynLayout L{};
  StateArena arena;
  L.chunks = chunk_layout(N, S, arena);
  L.partial = arena.take(8 * kPart * chunk_bound(N, S));
  L.mass = arena.take(8 * N);
  L.v = arena.take(8 * 3 * N);
  L.t0 = arena.take(8 * S);
  L.seed = arena.take(8 * S);
  L.flags = arena.take(4 * S);
  L.steps = arena.take(8 * S);
  L.coef = arena.take(8 * kCoef * S);
  L.total = arena.total;
  return L;
}

struct DynView {
  int64_t N;
  ChunkView ch;
  double *partial, *mass, *v, *t0, *coef;
  uint64_t* seed;
  int32_t* flags;
  int64_t* steps;
};
inline DynView dyn_view(int64_t N, int64_t S, void* state) {
  const DynLayout L = dyn_layout(N, S);
  char* b = (char*)state;
  return DynView{N, chunk_view(L.chunks, state), (double*)(b + L.partial), (double*)(b + L.mass), (double*)(b + L.v), (double*)(b + L.t0),
                 (double*)(b + L.coef), (uint64_t*)(b + L.seed), (int32_t*)(b + L.flags), (int64_t*)(b + L.steps)};
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
