// Batched complex Hermitian eigensolver for small matrices (numpy.linalg.eigh over a batch): one workgroup per matrix, the matrix
// and the eigenvectors in LDS, the solver of m3g_eigh.h.  One instantiation per capacity (8, 16, 32, 64 rows) so that a small matrix
// does not pay the LDS footprint of the largest: 2 x 16 n^2 bytes, 131 KB at n = 64 (one workgroup per CU), 4.6 KB at n = 12.
// No atomics, nothing shared between matrices: a matrix's outputs have the same bits wherever it stands in a batch.  No allocation,
// copy or wait (capture-safe).
#include "m3g_chunks.h"
#include "m3g_eigh.h"

namespace m3g {
namespace {
template <int NCAP, int THREADS>
__global__ void __launch_bounds__(THREADS) k_eigh_batched(int n, const double* __restrict__ a, int want_vectors, double* __restrict__ w,
                                                          double* __restrict__ v, int32_t* __restrict__ info) {
#pragma clang fp contract(off)
  __shared__ double A[2 * NCAP * NCAP];
  __shared__ double V[2 * NCAP * NCAP];
  __shared__ EighScratch<NCAP> sc;
  const int64_t mat = blockIdx.x;
  const int t = threadIdx.x;
  const int nn = n * n;
  const double* src = a + 2 * (int64_t)nn * mat;
  for (int e = t; e < 2 * nn; e += THREADS) A[e] = src[e];
  __syncthreads();
  const int status = eigh_jacobi_lds<NCAP>(A, want_vectors ? V : nullptr, n, sc, t, THREADS);
  const bool failed = (status & ~M3G_EIGH_SWEEPS_MASK) != 0;
  if (t == 0) info[mat] = status;
  for (int k = t; k < n; k += THREADS) w[(int64_t)n * mat + k] = sc.d[sc.order[k]];
  if (want_vectors) {
    double* dst = v + 2 * (int64_t)nn * mat;
    for (int e = t; e < nn; e += THREADS) {
      const int i = e / n, k = e % n;
      const int col = sc.order[k];
      dst[2 * e] = failed ? (double)NAN : V[2 * (i * n + col)];
      dst[2 * e + 1] = failed ? (double)NAN : V[2 * (i * n + col) + 1];
    }
  }
}

template <int NCAP, int THREADS>
void launch_eigh(int64_t M, int n, const double* a, int want_vectors, double* w, double* v, int32_t* info, hipStream_t s) {
  hipLaunchKernelGGL((k_eigh_batched<NCAP, THREADS>), dim3((unsigned)M), dim3(THREADS), 0, s, n, a, want_vectors, w, v, info);
}
}  // namespace
}  // namespace m3g

using namespace m3g;

extern "C" int m3g_eigh_batched(int64_t n_matrices, int32_t n, const double* a, int32_t want_vectors, double* eigenvalues,
                                double* eigenvectors, int32_t* info, void* stream_) {
  if (n_matrices < 0 || n_matrices > INT32_MAX || n < 1 || n > kEighMaxN || (want_vectors != 0 && want_vectors != 1)) {
    set_error("m3g_eigh_batched: need 0 <= n_matrices < 2^31, 1 <= n <= %d (M3G_EIGH_MAX_N) and want_vectors 0 / 1; got n_matrices %lld, n %d",
              kEighMaxN, (long long)n_matrices, (int)n);
    return M3G_ERR_VALUE;
  }
  if (!a || !eigenvalues || !info || (want_vectors && !eigenvectors)) {
    set_error("m3g_eigh_batched: null argument");
    return M3G_ERR_VALUE;
  }
  if (n_matrices == 0) return M3G_OK;
  hipStream_t s = (hipStream_t)stream_;
  // a round has n / 2 pairs of n elements: a wave covers it up to n = 16, four waves beyond
  if (n <= 8) launch_eigh<8, 64>(n_matrices, n, a, want_vectors, eigenvalues, eigenvectors, info, s);
  else if (n <= 16) launch_eigh<16, 64>(n_matrices, n, a, want_vectors, eigenvalues, eigenvectors, info, s);
  else if (n <= 32) launch_eigh<32, 256>(n_matrices, n, a, want_vectors, eigenvalues, eigenvectors, info, s);
  else launch_eigh<64, 256>(n_matrices, n, a, want_vectors, eigenvalues, eigenvectors, info, s);
  M3G_RETURN_LAUNCH_STATUS();
}
