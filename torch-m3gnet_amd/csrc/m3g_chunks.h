// The per-structure chunk table of the batched integrators (FIRE in m3g_relax.hip, MD in m3g_dynamics.hip): the N atoms of S
// structures cut into chunks of <= kChunkRows atoms that never straddle a structure, so a reduction over a chunk's rows followed by
// one over a structure's chunks in chunk order depends on that structure's own rows only -- bitwise the same alone or in any batch.
// Device side: the offsets [S+1] (int64), the structure of every chunk and its first atom, and every structure's first chunk
// ([S] = the number of chunks), built on the host from the caller's offsets and copied into the state buffer by the init call.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "m3g_internal.h"

namespace m3g {
constexpr int kChunkRows = 256;   // atoms per chunk == threads per workgroup of the row kernels

// chunks of a batch, at most (a bound that needs no offsets, so launch grids and buffer sizes follow from N and S alone)
inline int64_t chunk_bound(int64_t N, int64_t S) { return (N + kChunkRows - 1) / kChunkRows + S; }

struct ChunkLayout {
  size_t offsets, chunk_struct, chunk_begin, first_chunk;
};
// `take(bytes)` returns the offset of the next region of the caller's state buffer
template <class Take>
ChunkLayout chunk_layout(int64_t N, int64_t S, Take&& take) {
  const int64_t C = chunk_bound(N, S);
  ChunkLayout L{};
  L.offsets = take(8 * (S + 1));
  L.chunk_struct = take(4 * C);
  L.chunk_begin = take(8 * C);
  L.first_chunk = take(4 * (S + 1));   // [S] = number of chunks
  return L;
}

// 0 = o_0 < o_1 < ... < o_S = N; otherwise sets the library error ("<fn>: offsets ...") and returns false
inline bool chunk_offsets_ok(const char* fn, const int64_t* host_offsets, int64_t N, int64_t S) {
  if (host_offsets[0] != 0 || host_offsets[S] != N) { set_error("%s: offsets must run from 0 to n_atoms", fn); return false; }
  for (int64_t s = 0; s < S; ++s)
    if (host_offsets[s + 1] <= host_offsets[s]) { set_error("%s: offsets must increase strictly (every structure holds an atom)", fn); return false; }
  return true;
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

  int upload(const ChunkLayout& L, char* state, const int64_t* host_offsets, int64_t S, hipStream_t s) const {
    M3G_HIP_CHECK(hipMemcpyAsync(state + L.offsets, host_offsets, 8 * (S + 1), hipMemcpyHostToDevice, s));
    M3G_HIP_CHECK(hipMemcpyAsync(state + L.chunk_struct, chunk_struct.data(), 4 * chunk_struct.size(), hipMemcpyHostToDevice, s));
    M3G_HIP_CHECK(hipMemcpyAsync(state + L.chunk_begin, chunk_begin.data(), 8 * chunk_begin.size(), hipMemcpyHostToDevice, s));
    M3G_HIP_CHECK(hipMemcpyAsync(state + L.first_chunk, first_chunk.data(), 4 * (S + 1), hipMemcpyHostToDevice, s));
    return M3G_OK;
  }
};
}  // namespace m3g
