// Batched nudged-elastic-band force projection: climbing-image NEB with the improved tangent (Henkelman & Jonsson 2000; ASE's
// NEB(method="improvedtangent", climb=...).get_forces), every band of a batch with its own spring constant and climbing switch.
// Without it, a barrier search leaves the engine for an ASE NEB + FIRE loop on the host, one image at a time.  Here the interior
// images of every band are one batch of structures (the chunk table of m3g_chunks.h with the images as its structures), and one
// projection of the whole batch is three launches:
//   k_neb_partials   one workgroup per chunk (<= kChunkRows atoms of ONE interior image): tau+ = R_i+1 - R_i and tau- = R_i - R_i-1
//                    of its rows (the neighbour rows may be a band's fixed endpoints), the partial sums |tau+|^2, |tau-|^2,
//                    tau+.tau-, F.tau+, F.tau- and a count of non-finite inputs, in a fixed tree order;
//   k_neb_finalize   one wave per band: per interior image the chunk partials in chunk order (lane-strided, then a fixed butterfly),
//                    the tangent branch from the energies, the climbing image (argmax over the band's interior energies, lowest
//                    index on ties), and the two scalars alpha, beta of F_neb = F + alpha tau+ + beta tau- in closed form;
//   k_neb_apply      one workgroup per chunk: F_neb of every row in fp64, stored as fp32.
// No atomics: every result depends on the band's own rows only, so it is bitwise the same alone or in any batch.  No allocation,
// copy or wait in m3g_neb_forces (capture-safe).
#include <cmath>

#include "m3g_chunks.h"
#include "m3g_internal.h"

namespace m3g {
namespace {
constexpr int kPart = 6;    // per chunk: |tau+|^2, |tau-|^2, tau+.tau-, F.tau+, F.tau-, non-finite inputs
constexpr int kRows = 5;    // observables per image: |tau+|, |tau-|, F.tau_hat, spring term, climbing flag

struct NebView {
  int64_t N, B;
  ChunkView ch;   // the interior images are its structures (ch.S of them)
  double* partial;
  const int64_t *img_prev, *img_next;   // first row of the neighbour image: >= 0 in pos, -1 - r for row r of the endpoint rows
  const int32_t* band_images;           // [B+1]
  const double* k;
  const int32_t* climb;
  const double *ep_pos, *ep_energy;     // per band: initial rows, final rows; energies [2B] (initial, final)
  double* coef;                         // [I, 2]: alpha, beta
};
// the endpoint rows (2 n_b per band) never exceed 2N: every band holds an interior image of n_b atoms
Carved<NebView> neb_view(int64_t N, int64_t I, int64_t B, void* state) {
  Carve c{state};
  NebView st{N, B};
  st.ch = chunk_view(N, I, c);
  st.partial = c.take<double>(kPart * chunk_bound(N, I));
  st.img_prev = c.take<int64_t>(I);
  st.img_next = c.take<int64_t>(I);
  st.band_images = c.take<int32_t>(B + 1);
  st.k = c.take<double>(B);
  st.climb = c.take<int32_t>(B);
  st.ep_pos = c.take<double>(3 * 2 * N);
  st.ep_energy = c.take<double>(2 * B);
  st.coef = c.take<double>(2 * I);
  return {st, c.off};
}

__device__ inline const double* neighbour_row(int64_t enc, int64_t local, const double* pos, const double* ep) {
  return enc >= 0 ? pos + 3 * (enc + local) : ep + 3 * (-1 - enc + local);
}

// tau+ and tau- of row r (of image i) and whether all twelve inputs of the row are finite
__device__ inline bool row_taus(const NebView& st, int i, int64_t r, const double* __restrict__ pos, const float* __restrict__ forces,
                                double tp[3], double tm[3], double f[3]) {
  const int64_t local = r - st.ch.offsets[i];
  const double* x = pos + 3 * r;
  const double* xp = neighbour_row(st.img_prev[i], local, pos, st.ep_pos);
  const double* xn = neighbour_row(st.img_next[i], local, pos, st.ep_pos);
  bool ok = true;
  for (int c = 0; c < 3; ++c) {
    tp[c] = xn[c] - x[c];
    tm[c] = x[c] - xp[c];
    f[c] = forces[3 * r + c];
    ok = ok && std::isfinite(x[c]) && std::isfinite(xp[c]) && std::isfinite(xn[c]) && std::isfinite(f[c]);
  }
  return ok;
}

__global__ void __launch_bounds__(kChunkRows) k_neb_partials(NebView st, const double* __restrict__ pos, const float* __restrict__ forces) {
  __shared__ double sh[kPart][kChunkRows];
  const int c = blockIdx.x, t = threadIdx.x;
  if (c >= st.ch.n_chunks()) return;
  const int i = st.ch.structure(c);
  const int64_t r = st.ch.row(c, t);
  double val[kPart] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (st.ch.holds(i, r)) {
    double tp[3], tm[3], f[3];
    val[5] = row_taus(st, i, r, pos, forces, tp, tm, f) ? 0.0 : 1.0;
    val[0] = tp[0] * tp[0] + tp[1] * tp[1] + tp[2] * tp[2];
    val[1] = tm[0] * tm[0] + tm[1] * tm[1] + tm[2] * tm[2];
    val[2] = tp[0] * tm[0] + tp[1] * tm[1] + tp[2] * tm[2];
    val[3] = f[0] * tp[0] + f[1] * tp[1] + f[2] * tp[2];
    val[4] = f[0] * tm[0] + f[1] * tm[1] + f[2] * tm[2];
  }
  chunk_tree_reduce<kPart>(sh, val, t);
  if (t < kPart) st.partial[kPart * c + t] = sh[t][0];
}

__global__ void __launch_bounds__(kWave * kFinalizeWaves) k_neb_finalize(NebView st, const float* __restrict__ energies, double* __restrict__ rows) {
  const int lane = threadIdx.x % kWave;
  const int64_t b = (int64_t)blockIdx.x * kFinalizeWaves + threadIdx.x / kWave;
  if (b >= st.B) return;   // (whole waves: b is uniform across a wave)
  const int i0 = st.band_images[b], i1 = st.band_images[b + 1];
  // the climbing image: highest interior energy, lowest index on ties (a NaN energy is never chosen; its image fails below anyway)
  int imax = -1;
  if (st.climb[b]) {
    double best = 0.0;
    for (int i = i0; i < i1; ++i) {
      const double e = energies[i];
      if (e == e && (imax < 0 || e > best)) { best = e; imax = i; }
    }
  }
  const double kb = st.k[b];
  for (int i = i0; i < i1; ++i) {
    double acc[kPart];
    wave_chunk_sum<kPart>(st.ch, i, st.partial, lane, acc);
    if (lane != 0) continue;
    const double vi = energies[i];
    const double vp = i == i0 ? st.ep_energy[2 * b] : (double)energies[i - 1];
    const double vn = i == i1 - 1 ? st.ep_energy[2 * b + 1] : (double)energies[i + 1];
    double a, c;   // tau = a tau+ + c tau-
    if (vn > vi && vi > vp) {
      a = 1.0; c = 0.0;
    } else if (vn < vi && vi < vp) {
      a = 0.0; c = 1.0;
    } else {
      const double dn = fabs(vn - vi), dp = fabs(vp - vi);
      const double dmax = fmax(dn, dp), dmin = fmin(dn, dp);
      if (vn > vp) { a = dmax; c = dmin; } else { a = dmin; c = dmax; }
    }
    const double pp = acc[0], mm = acc[1], pm = acc[2], fp = acc[3], fm = acc[4];
    const double tt = a * a * pp + 2.0 * a * c * pm + c * c * mm;   // |tau|^2
    const double nt = sqrt(tt);
    const double ft = (a * fp + c * fm) / nt;                        // F . tau_hat
    const bool climbing = i == imax;
    const double spring = climbing ? 0.0 : kb * (sqrt(pp) - sqrt(mm));
    const double s = climbing ? -2.0 * ft : spring - ft;            // F_neb = F + s tau_hat
    double alpha = s * a / nt, beta = s * c / nt;
    const bool bad = acc[5] != 0.0 || !(std::isfinite(vi) && std::isfinite(vp) && std::isfinite(vn)) || !(tt > 0.0) ||
                     !(std::isfinite(alpha) && std::isfinite(beta));
    if (bad) alpha = beta = NAN;   // NaN rows: FIRE flags the band M3G_FIRE_ERROR and freezes it
    st.coef[2 * i] = alpha;
    st.coef[2 * i + 1] = beta;
    if (rows) {
      double* o = rows + kRows * (int64_t)i;
      o[0] = sqrt(pp);
      o[1] = sqrt(mm);
      o[2] = ft;
      o[3] = spring;
      o[4] = climbing ? 1.0 : 0.0;
    }
  }
}

__global__ void __launch_bounds__(kChunkRows) k_neb_apply(NebView st, const double* __restrict__ pos, const float* __restrict__ forces,
                                                          float* __restrict__ neb_forces) {
  const int c = blockIdx.x;
  if (c >= st.ch.n_chunks()) return;
  const int i = st.ch.structure(c);
  const int64_t r = st.ch.row(c, threadIdx.x);
  if (!st.ch.holds(i, r)) return;
  const double alpha = st.coef[2 * i], beta = st.coef[2 * i + 1];
  double tp[3], tm[3], f[3];
  row_taus(st, i, r, pos, forces, tp, tm, f);
  for (int k = 0; k < 3; ++k) neb_forces[3 * r + k] = (float)(f[k] + alpha * tp[k] + beta * tm[k]);
}

bool neb_sizes_ok(int64_t N, int64_t I, int64_t B) { return N >= 1 && I >= 1 && B >= 1 && B <= I && I <= N; }
}  // namespace
}  // namespace m3g

using namespace m3g;

extern "C" int m3g_neb_state_bytes(int64_t n_atoms, int64_t n_images, int64_t n_bands, size_t* bytes) {
  if (!bytes || !neb_sizes_ok(n_atoms, n_images, n_bands)) { set_error("m3g_neb_state_bytes: bad sizes (need 1 <= n_bands <= n_images <= n_atoms)"); return M3G_ERR_VALUE; }
  *bytes = neb_view(n_atoms, n_images, n_bands, nullptr).bytes;
  return M3G_OK;
}

extern "C" int m3g_neb_init(int64_t n_atoms, int64_t n_images, int64_t n_bands, const int64_t* host_image_offsets, const int32_t* host_band_images,
                            const double* host_k, const int32_t* host_climb, const double* endpoint_pos, const double* host_endpoint_energies,
                            void* state, size_t state_bytes, void* stream_) {
  const int64_t N = n_atoms, I = n_images, B = n_bands;
  if (!neb_sizes_ok(N, I, B) || !host_image_offsets || !host_band_images || !host_k || !host_climb || !endpoint_pos ||
      !host_endpoint_energies || !state) {
    set_error("m3g_neb_init: null argument or bad sizes (need 1 <= n_bands <= n_images <= n_atoms)");
    return M3G_ERR_VALUE;
  }
  if (!offsets_ok("m3g_neb_init", host_image_offsets, N, I)) return M3G_ERR_VALUE;
  if (host_band_images[0] != 0 || host_band_images[B] != I) { set_error("m3g_neb_init: band image offsets must run from 0 to n_images"); return M3G_ERR_VALUE; }
  std::vector<int64_t> img_prev(I), img_next(I);
  int64_t ep_rows = 0;
  for (int64_t b = 0; b < B; ++b) {
    const int64_t i0 = host_band_images[b], i1 = host_band_images[b + 1];
    if (i1 <= i0) { set_error("m3g_neb_init: band %lld has no interior image", (long long)b); return M3G_ERR_VALUE; }
    if (i1 > I) { set_error("m3g_neb_init: band image offsets must increase to n_images"); return M3G_ERR_VALUE; }
    const int64_t n = host_image_offsets[i0 + 1] - host_image_offsets[i0];
    for (int64_t i = i0; i < i1; ++i)
      if (host_image_offsets[i + 1] - host_image_offsets[i] != n) {
        set_error("m3g_neb_init: the images of band %lld have different atom counts", (long long)b);
        return M3G_ERR_VALUE;
      }
    if (!finite_positive(host_k[b])) { set_error("m3g_neb_init: spring constant k of band %lld must be finite and > 0", (long long)b); return M3G_ERR_VALUE; }
    if (host_climb[b] != 0 && host_climb[b] != 1) { set_error("m3g_neb_init: climb of band %lld must be 0 or 1", (long long)b); return M3G_ERR_VALUE; }
    if (!(std::isfinite(host_endpoint_energies[2 * b]) && std::isfinite(host_endpoint_energies[2 * b + 1]))) {
      set_error("m3g_neb_init: endpoint energies of band %lld are not finite", (long long)b);
      return M3G_ERR_VALUE;
    }
    for (int64_t i = i0; i < i1; ++i) {
      img_prev[i] = i == i0 ? -1 - ep_rows : host_image_offsets[i - 1];
      img_next[i] = i == i1 - 1 ? -1 - (ep_rows + n) : host_image_offsets[i + 1];
    }
    ep_rows += 2 * n;
  }
  const auto [st, total] = neb_view(N, I, B, state);
  if (!state_fits("m3g_neb_init", state_bytes, total, true)) return M3G_ERR_SIZE;
  const ChunkTable table(host_image_offsets, I);
  hipStream_t s = (hipStream_t)stream_;
  if (int rc = table.upload(st.ch, host_image_offsets, s)) return rc;
  M3G_HIP_CHECK(hipMemcpyAsync((void*)st.img_prev, img_prev.data(), 8 * I, hipMemcpyHostToDevice, s));
  M3G_HIP_CHECK(hipMemcpyAsync((void*)st.img_next, img_next.data(), 8 * I, hipMemcpyHostToDevice, s));
  M3G_HIP_CHECK(hipMemcpyAsync((void*)st.band_images, host_band_images, 4 * (B + 1), hipMemcpyHostToDevice, s));
  M3G_HIP_CHECK(hipMemcpyAsync((void*)st.k, host_k, 8 * B, hipMemcpyHostToDevice, s));
  M3G_HIP_CHECK(hipMemcpyAsync((void*)st.climb, host_climb, 4 * B, hipMemcpyHostToDevice, s));
  M3G_HIP_CHECK(hipMemcpyAsync((void*)st.ep_pos, endpoint_pos, 8 * 3 * ep_rows, hipMemcpyDeviceToDevice, s));
  M3G_HIP_CHECK(hipMemcpyAsync((void*)st.ep_energy, host_endpoint_energies, 8 * 2 * B, hipMemcpyHostToDevice, s));
  M3G_HIP_CHECK(hipStreamSynchronize(s));   // (the host tables above go out of scope)
  return M3G_OK;
}

extern "C" int m3g_neb_forces(int64_t n_atoms, int64_t n_images, int64_t n_bands, void* state, size_t state_bytes, const double* pos,
                              const float* energies, const float* forces, float* neb_forces, double* rows, void* stream_) {
  const int64_t N = n_atoms, I = n_images, B = n_bands;
  if (!neb_sizes_ok(N, I, B) || !state || !pos || !energies || !forces || !neb_forces) {
    set_error("m3g_neb_forces: null argument or bad sizes");
    return M3G_ERR_VALUE;
  }
  const auto [st, total] = neb_view(N, I, B, state);
  if (!state_fits("m3g_neb_forces", state_bytes, total)) return M3G_ERR_SIZE;
  hipStream_t s = (hipStream_t)stream_;
  const dim3 grid((unsigned)chunk_bound(N, I));   // workgroups beyond the table's chunk count return at once
  hipLaunchKernelGGL(k_neb_partials, grid, dim3(kChunkRows), 0, s, st, pos, forces);
  hipLaunchKernelGGL(k_neb_finalize, grid_for(B, kFinalizeWaves), dim3(kWave * kFinalizeWaves), 0, s, st, energies, rows);
  hipLaunchKernelGGL(k_neb_apply, grid, dim3(kChunkRows), 0, s, st, pos, forces, neb_forces);
  M3G_RETURN_LAUNCH_STATUS();
}
