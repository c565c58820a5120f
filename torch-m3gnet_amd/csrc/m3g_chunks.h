// The device and C-ABI layer all nineteen batched drivers share.  Eleven of them include it themselves: m3g_relax.hip (FIRE),
// m3g_lbfgs.hip, m3g_neb.hip, m3g_phonons.hip, m3g_elastic.hip, m3g_trajectory.hip, m3g_scattering.hip, m3g_local_order.hip,
// m3g_thermo.hip, m3g_nma.hip and m3g_meta.hip.  m3g_remd.hip,
// m3g_mc.hip and m3g_rnemd.hip, which work on the state of m3g_dyn_*, reach it through m3g_dyn_state.h; the five step families
// m3g_dynamics.hip, m3g_nhc.hip, m3g_mtk.hip, m3g_pimd.hip and m3g_ti.hip through m3g_integrator.h, which includes
// m3g_dyn_state.h.  (m3g_eigh.hip, no driver, includes it too, for kWave and its checks.)  Here is one copy of what their C entry
// points spell alike on the host: the checks of an init (init_args_ok, batch32_sizes_ok, structure_fits_int32, offsets_ok,
// lattice_ok, mass_ok, temperature_ok), the size check of a state buffer (state_fits), the tails of a launch, of an init and of
// a read (M3G_RETURN_LAUNCH_STATUS, launched_and_synced, upload_image, read_all), and the constants kKappa, kBoltzmann and kTwoPi.
// Every state buffer is described once, by the function that carves its view (chunk_view below, then the driver's own regions;
// see Carved), and read back through read_back.
// The chunk table: the N atoms of S structures cut into chunks of <= kChunkRows atoms that never straddle a
// structure, so a reduction over a chunk's rows (chunk_tree_reduce) followed by one over a structure's chunks in chunk order
// (wave_chunk_sum, or a serial walk) depends on that structure's own rows only -- bitwise the same alone or in any batch.  Device
// side: the offsets [S+1] (int64), the structure of every chunk and its first atom, and every structure's first chunk ([S] = the
// number of chunks), built on the host from the caller's offsets and copied into the state buffer by the init call.
// No device function here multiplies: a kernel's own floating-point contraction mode (some switch it off, lexically) must keep
// deciding every rounding, and a helper would bring its own.  det3 / inv3 are host code.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <vector>

#include "m3g_internal.h"

namespace m3g {
constexpr int kChunkRows = 256;       // atoms per chunk == threads per workgroup of the row kernels
constexpr int kWave = 64;
constexpr int kFinalizeWaves = 4;     // structures (one wave each) per workgroup of the wave-per-structure kernels
constexpr double kKappa = 9.648533215665e-3;   // A/fs^2 per eV/(A amu)
constexpr double kBoltzmann = 8.617333262e-5;  // eV/K
constexpr double kTwoPi = 6.283185307179586;

// chunks of a batch, at most (a bound that needs no offsets, so launch grids and buffer sizes follow from N and S alone)
inline int64_t chunk_bound(int64_t N, int64_t S) { return (N + kChunkRows - 1) / kChunkRows + S; }

// The device side of the table.  Row kernels run one workgroup per chunk (a grid of chunk_bound() workgroups: those beyond the
// table's chunk count return at once), thread t on row t of the chunk.
struct ChunkView {
  int64_t S;
  const int64_t* offsets;
  const int32_t* chunk_struct;
  const int64_t* chunk_begin;
  const int32_t* first_chunk;
  __device__ int n_chunks() const { return first_chunk[S]; }
  __device__ int structure(int c) const { return chunk_struct[c]; }   // c < n_chunks()
  __device__ int64_t row(int c, int t) const { return chunk_begin[c] + t; }
  __device__ bool holds(int s, int64_t row) const { return row < offsets[s + 1]; }   // (a structure's last chunk may be part-filled)
  __device__ int chunks_begin(int64_t s) const { return first_chunk[s]; }
  __device__ int chunks_end(int64_t s) const { return first_chunk[s + 1]; }
};
// carves the table from a driver's state: the first four regions of every state buffer
inline ChunkView chunk_view(int64_t N, int64_t S, Carve& c) {
  const int64_t C = chunk_bound(N, S);
  ChunkView v{S};
  v.offsets = c.take<int64_t>(S + 1);
  v.chunk_struct = c.take<int32_t>(C);
  v.chunk_begin = c.take<int64_t>(C);
  v.first_chunk = c.take<int32_t>(S + 1);   // [S] = number of chunks
  return v;
}

// Every driver describes its state once, as `Carved<XView> x_view(sizes..., void* state)`: one Carve::take per region, in allocation
// order.  Over a null state the same function measures: `bytes` is the size of the buffer, and each pointer of `view` the byte offset
// of its region (carve_offset).
template <class View>
struct Carved { View view; size_t bytes; };

// read-back: a null destination (or an empty region) is skipped, otherwise `count` elements are queued device-to-host on s (the
// caller synchronises)
template <class T>
inline hipError_t read_back(T* host, const T* dev, size_t count, hipStream_t s) {
  return host && count ? hipMemcpyAsync(host, dev, sizeof(T) * count, hipMemcpyDeviceToHost, s) : hipSuccess;
}

__device__ inline double max_nan(double m, double x) { return (x > m || x != x) ? x : m; }   // a NaN row stays visible

// K columns over the kChunkRows threads of a workgroup, thread t contributing val[]: the result of column j is sh[j][0].  A fixed
// tree, so the order depends on the row's place in its chunk only.  The first K - KMax columns are sums, the last KMax max_nan.
template <int K, int KMax = 0, class T>
__device__ inline void chunk_tree_reduce(T (&sh)[K][kChunkRows], const T (&val)[K], int t) {
  for (int j = 0; j < K; ++j) sh[j][t] = val[j];
  __syncthreads();
  for (int w = kChunkRows / 2; w > 0; w >>= 1) {
    if (t < w) {
      for (int j = 0; j < K - KMax; ++j) sh[j][t] += sh[j][t + w];
      if constexpr (KMax > 0)
        for (int j = K - KMax; j < K; ++j) sh[j][t] = max_nan(sh[j][t], sh[j][t + w]);
    }
    __syncthreads();
  }
}

// The sums of structure s's chunk partials ([chunk][K]) by one wave: lane-strided in chunk order, then a butterfly (a + b on both
// partners, so every lane ends with the same bits).
template <int K>
__device__ inline void wave_chunk_sum(const ChunkView& ch, int64_t s, const double* partial, int lane, double (&acc)[K]) {
  for (int j = 0; j < K; ++j) acc[j] = 0.0;
  for (int c = ch.chunks_begin(s) + lane; c < ch.chunks_end(s); c += kWave)
    for (int j = 0; j < K; ++j) acc[j] += partial[K * c + j];
#pragma unroll   // (as the compiler did of its own accord while this loop stood in the kernels)
  for (int w = kWave / 2; w > 0; w >>= 1)
    for (int j = 0; j < K; ++j) acc[j] += __shfl_xor(acc[j], w, kWave);
}

// Host checks; the _ok ones set the library error ("<fn>: ...") and return false.
inline bool finite_positive(double x) { return std::isfinite(x) && x > 0.0; }
inline bool batch_sizes_ok(int64_t N, int64_t S) { return N >= 1 && S >= 1 && S <= N; }   // every structure holds an atom

// 0 = o_0 < o_1 < ... < o_S = N; `what` names the offsets and `upto` their end in the message
inline bool offsets_ok(const char* fn, const int64_t* host_offsets, int64_t N, int64_t S, const char* what = "offsets",
                       const char* upto = "n_atoms") {
  if (host_offsets[0] != 0 || host_offsets[S] != N) { set_error("%s: %s must run from 0 to %s", fn, what, upto); return false; }
  for (int64_t s = 0; s < S; ++s)
    if (host_offsets[s + 1] <= host_offsets[s]) { set_error("%s: %s must increase strictly (every structure holds an atom)", fn, what); return false; }
  return true;
}

// rows = lattice vectors (host arithmetic: the kernels spell their own determinants out)
inline double det3(const double* L) {
  return L[0] * (L[4] * L[8] - L[5] * L[7]) - L[1] * (L[3] * L[8] - L[5] * L[6]) + L[2] * (L[3] * L[7] - L[4] * L[6]);
}
inline void inv3(const double* L, double inv[9]) {   // from the adjugate
  const double det = det3(L);
  inv[0] = (L[4] * L[8] - L[5] * L[7]) / det; inv[1] = (L[2] * L[7] - L[1] * L[8]) / det; inv[2] = (L[1] * L[5] - L[2] * L[4]) / det;
  inv[3] = (L[5] * L[6] - L[3] * L[8]) / det; inv[4] = (L[0] * L[8] - L[2] * L[6]) / det; inv[5] = (L[2] * L[3] - L[0] * L[5]) / det;
  inv[6] = (L[3] * L[7] - L[4] * L[6]) / det; inv[7] = (L[1] * L[6] - L[0] * L[7]) / det; inv[8] = (L[0] * L[4] - L[1] * L[3]) / det;
}

// the lattice of structure s: finite, |det| >= 1e-12 (one structure per call, so a driver can keep it in its per-structure order)
inline bool lattice_ok(const char* fn, const double* L, int64_t s) {
  for (int k = 0; k < 9; ++k)
    if (!std::isfinite(L[k])) { set_error("%s: lattice of structure %lld is not finite", fn, (long long)s); return false; }
  if (!(std::fabs(det3(L)) >= 1e-12)) { set_error("%s: singular cell of structure %lld", fn, (long long)s); return false; }
  return true;
}

// The checks of m3g_*_init, each naming the caller `fn`; they set the library error and return false.  They come in pieces
// because every init keeps the order of its checks, its own between them: the first thing wrong is the one reported.
inline bool init_args_ok(const char* fn, int64_t N, int64_t S, bool pointers) {
  if (batch_sizes_ok(N, S) && pointers) return true;
  set_error("%s: null argument or bad sizes", fn);
  return false;
}
// a batch whose structure indices fit int32_t as well
inline bool batch32_sizes_ok(int64_t N, int64_t S) { return batch_sizes_ok(N, S) && S <= INT32_MAX; }
// ... and a structure whose row indices do
inline bool structure_fits_int32(const char* fn, const int64_t* host_offsets, int64_t s) {
  if (host_offsets[s + 1] - host_offsets[s] <= INT32_MAX) return true;
  set_error("%s: structure %lld holds too many atoms", fn, (long long)s);
  return false;
}
// `of`: what a mass belongs to (a unit atom in m3g_nma_init)
inline bool mass_ok(const char* fn, const double* host_masses, int64_t i, const char* of = "atom") {
  if (finite_positive(host_masses[i])) return true;
  set_error("%s: mass of %s %lld is not finite and > 0", fn, of, (long long)i);
  return false;
}
// `of`: what a temperature belongs to (a ring in m3g_pimd_init); `zero_ok`: m3g_dyn_init alone takes T = 0
inline bool temperature_ok(const char* fn, const double* host_temperatures, int64_t s, const char* of = "structure", bool zero_ok = false) {
  const double t = host_temperatures[s];
  if (zero_ok ? std::isfinite(t) && t >= 0.0 : finite_positive(t)) return true;
  set_error("%s: temperature of %s %lld is not finite and %s 0", fn, of, (long long)s, zero_ok ? ">=" : ">");
  return false;
}
// the caller's state buffer holds the carved view (init says both sizes); `which` names the buffer of a call that takes two
inline bool state_fits(const char* fn, size_t state_bytes, size_t total, bool say_sizes = false, const char* which = "") {
  if (state_bytes >= total) return true;
  if (say_sizes) set_error("%s: state buffer too small (%zu < %zu)", fn, state_bytes, total);
  else set_error("%s: %s%sstate buffer too small", fn, which, *which ? " " : "");
  return false;
}

// the tail of a call that launched (a macro, as M3G_HIP_CHECK: the error names the caller's file and line)
#define M3G_RETURN_LAUNCH_STATUS() do { M3G_HIP_CHECK(hipGetLastError()); return M3G_OK; } while (0)

// the tail of an init (or of m3g_ti_path) after its launches: only now may the host arrays the copies read go out of scope
inline int launched_and_synced(hipStream_t s) {
  M3G_HIP_CHECK(hipGetLastError());
  M3G_HIP_CHECK(hipStreamSynchronize(s));
  return M3G_OK;
}

// The tail of m3g_*_read: every read-back of the list queued on s (read_back: a null destination or an empty region is skipped),
// then the wait.  rb() makes an entry and keeps read_back's rule that the host and the device element types agree.
struct ReadBack { void* host; const void* dev; size_t bytes; };
template <class T>
inline ReadBack rb(T* host, const T* dev, size_t count) { return {host, dev, sizeof(T) * count}; }
inline int read_all(hipStream_t s, std::initializer_list<ReadBack> list) {
  for (const ReadBack& r : list) M3G_HIP_CHECK(read_back((char*)r.host, (const char*)r.dev, r.bytes, s));
  M3G_HIP_CHECK(hipStreamSynchronize(s));
  return M3G_OK;
}

// The host side of the table.  upload() queues asynchronous copies from these vectors: keep the object alive until the stream has
// been synchronised.
struct ChunkTable {
  std::vector<int32_t> chunk_struct, first_chunk;
  std::vector<int64_t> chunk_begin;

  ChunkTable(const int64_t* host_offsets, int64_t S) : first_chunk(S + 1) {
    for (int64_t s = 0; s < S; ++s) {
      first_chunk[s] = (int32_t)chunk_struct.size();
      for (int64_t b = host_offsets[s]; b < host_offsets[s + 1]; b += kChunkRows) {
        chunk_struct.push_back((int32_t)s);
        chunk_begin.push_back(b);
      }
    }
    first_chunk[S] = (int32_t)chunk_struct.size();
  }

  int upload(const ChunkView& v, const int64_t* host_offsets, hipStream_t s) const {
    M3G_HIP_CHECK(hipMemcpyAsync((void*)v.offsets, host_offsets, 8 * (v.S + 1), hipMemcpyHostToDevice, s));
    M3G_HIP_CHECK(hipMemcpyAsync((void*)v.chunk_struct, chunk_struct.data(), 4 * chunk_struct.size(), hipMemcpyHostToDevice, s));
    M3G_HIP_CHECK(hipMemcpyAsync((void*)v.chunk_begin, chunk_begin.data(), 8 * chunk_begin.size(), hipMemcpyHostToDevice, s));
    M3G_HIP_CHECK(hipMemcpyAsync((void*)v.first_chunk, first_chunk.data(), 4 * (v.S + 1), hipMemcpyHostToDevice, s));
    return M3G_OK;
  }
};

// The tail of an init that filled a host image of its state (a buffer carved as the state is, so every region stands at its offset):
// the chunk table of `host_offsets` into `ch`, the image's bytes from the region `first` up to `end` -- pointers into the device
// state, as its view names them -- in one copy to the same place of the state, then the wait: only now may the image and the
// caller's arrays go out of scope.  (m3g_remd_init, whose state has no chunk table, sends its whole image itself.)
inline int upload_image(const std::vector<char>& image, const void* state, const void* first, const void* end, const ChunkView& ch,
                        const int64_t* host_offsets, hipStream_t s) {
  const ChunkTable table(host_offsets, ch.S);
  if (int rc = table.upload(ch, host_offsets, s)) return rc;
  const size_t begin = (size_t)((const char*)first - (const char*)state), bytes = (size_t)((const char*)end - (const char*)first);
  M3G_HIP_CHECK(hipMemcpyAsync((void*)first, image.data() + begin, bytes, hipMemcpyHostToDevice, s));
  M3G_HIP_CHECK(hipStreamSynchronize(s));
  return M3G_OK;
}
}  // namespace m3g
