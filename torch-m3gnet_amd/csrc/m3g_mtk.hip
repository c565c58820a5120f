// Batched molecular dynamics, the flexible-cell ensemble: the fully anisotropic Martyna-Tobias-Klein NPT barostat with Nose-Hoover
// chains (Martyna, Tobias, Klein, J. Chem. Phys. 101, 4177 (1994); Martyna, Tuckerman, Tobias, Klein, Mol. Phys. 87, 1117 (1996)),
// every structure of a batch with its own target temperature, beside m3g_dynamics.hip and m3g_nhc.hip and on the same layers (the
// chunk table of m3g_chunks.h, the constants of m3g_dyn_state.h, the chain half-step of m3g_nhc_chain.h).  The barostat variable is a symmetric 3x3 rate vg, 6 numbers in
// Voigt order xx, yy, zz, yz, zx, xy; positions and lattice rows are row vectors, so a symmetric matrix acts from the right.
// One step is T(h) B(h) A(dt) [forces] B(h) T(h), h = dt/2, split over calls as m3g_nhc_step.  One call -- finish step k,
// observables, start step k+1 -- is three launches for the whole batch:
//   k_mtk_partials   one workgroup per chunk: the finish kick v KV + a KA in registers (the two symmetric matrices the previous
//                    call's opening stored: vg has not changed since), then the partial sums of the 6 components of m v v^T, of
//                    m v, of F and the non-finite count;
//   k_mtk_finalize   one wave per structure: the chunk partials in chunk order, the error verdict, then on lane 0 the serial chain
//                    arithmetic of the finish and of the next start (K after a uniform scale is s^2 K, so there is no second pass
//                    over the atoms) with the observables between them and the rate verdict at its end -- nothing is written before
//                    it -- then on lanes 0 .. 3, one each, the four matrix functions exp(-B), phi1(-B), exp(A), phi1(A) by Horner,
//                    and from them pbar (lane 0), the new cell (lane 2) and the coefficient block;
//   k_mtk_apply      one workgroup per chunk: the finish kick and lambda, the opening kick, pbar / m, the drift.  The only writer of
//                    velocities and positions, after the verdict: a flagged structure keeps its bits.
// No atomics: every result depends on the structure's own rows only, so it is bitwise the same alone or in any batch.  No allocation,
// copy or wait in m3g_mtk_step (capture-safe).  The row prologue and the epilogue of the partials, the cell volume and the checks and
// copies of the entry points are m3g_integrator.h.
#include <cmath>

#include "m3g_integrator.h"
#include "m3g_nhc_chain.h"

namespace m3g {
namespace {
constexpr int kMtkPart = 13;    // per chunk: sum m v v^T [6, Voigt], sum m v [3], sum F [3], non-finite forces
enum MtkPart : int { kPK = 0, kPMv = 6, kPF = 9, kPBad = 12 };
// per structure: action (0 none, 1 finish only, 2 finish + start), finish?, lambda (finish only: s1), the finish kick (two symmetric
// matrices), the start kick (two: kept for the next call's finish), the drift (two), pbar [3]
constexpr int kMtkCoef = 42;
enum MtkCoef : int { kAct, kFinish, kLam, kFinV = 3, kFinA = 9, kKickV = 15, kKickA = 21, kDriftX = 27, kDriftV = 33, kPbar = 39 };
constexpr int kOrder = 12;        // exp and phi1 as their series to A^12, by Horner
constexpr double kMaxRate = 0.05; // max |vg_ab| dt: the first dropped term is then below 2^-53

constexpr int chain_row(int M) { return 4 * M + 6; }   // xi[M], vxi[M], xib[M], vxib[M], vg[6]

struct MtkView {
  int64_t N;
  int M;
  ChunkView ch;
  double *partial, *mass, *v, *t0, *coef, *chain;
  int32_t* flags;
  int64_t* steps;
};
inline Carved<MtkView> mtk_view(int64_t N, int64_t S, int M, void* state) {
  Carve c{state};
  MtkView st{N, M};
  st.ch = chunk_view(N, S, c);
  st.partial = c.take<double>(kMtkPart * chunk_bound(N, S));
  st.mass = c.take<double>(N);
  st.v = c.take<double>(3 * N);
  st.t0 = c.take<double>(S);
  st.flags = c.take<int32_t>(S);
  st.steps = c.take<int64_t>(S);
  st.coef = c.take<double>(kMtkCoef * S);
  st.chain = c.take<double>(chain_row(M) * S);
  return {st, c.off};
}

// row vector times symmetric matrix (Voigt: xx yy zz yz zx xy)
__device__ inline void vec_sym(const double (&v)[3], const double* m, double (&out)[3]) {
  out[0] = v[0] * m[0] + v[1] * m[5] + v[2] * m[4];
  out[1] = v[0] * m[5] + v[1] * m[1] + v[2] * m[3];
  out[2] = v[0] * m[4] + v[1] * m[3] + v[2] * m[2];
}
// v M + a B: a kick or a drift, both linear maps with two matrices of the structure
__device__ inline void axpby(double (&v)[3], const double* mv, const double (&a)[3], const double* ma) {
  double p[3], q[3];
  vec_sym(v, mv, p);
  vec_sym(a, ma, q);
  for (int k = 0; k < 3; ++k) v[k] = p[k] + q[k];
}
// q = I + r a q for two polynomials of the same symmetric matrix: the product's upper triangle only, so it stays symmetric
__device__ inline void horner_step(const double (&a)[6], double (&q)[6], double r) {
  const double t0 = a[0] * q[0] + a[5] * q[5] + a[4] * q[4];
  const double t1 = a[5] * q[5] + a[1] * q[1] + a[3] * q[3];
  const double t2 = a[4] * q[4] + a[3] * q[3] + a[2] * q[2];
  const double t3 = a[5] * q[4] + a[1] * q[3] + a[3] * q[2];
  const double t4 = a[0] * q[4] + a[5] * q[3] + a[4] * q[2];
  const double t5 = a[0] * q[5] + a[5] * q[1] + a[4] * q[3];
  q[0] = 1.0 + t0 * r;
  q[1] = 1.0 + t1 * r;
  q[2] = 1.0 + t2 * r;
  q[3] = t3 * r;
  q[4] = t4 * r;
  q[5] = t5 * r;
}

__global__ void __launch_bounds__(kChunkRows) k_mtk_init(MtkView st, const double* __restrict__ vel) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < 3 * st.N) st.v[i] = vel[i];
  if (i < st.ch.S) {
    st.flags[i] = 0;
    st.steps[i] = 0;
    for (int k = 0; k < kMtkCoef; ++k) st.coef[kMtkCoef * i + k] = 0.0;
    for (int k = 0; k < chain_row(st.M); ++k) st.chain[chain_row(st.M) * i + k] = 0.0;
  }
}

__global__ void __launch_bounds__(kChunkRows) k_mtk_partials(MtkView st, const float* __restrict__ forces) {
  const int c = blockIdx.x, t = threadIdx.x;
  const auto [live, s, fl, i, holds] = chunk_row(st, c, t);
  if (!live) return;
  double val[kMtkPart];
  for (int k = 0; k < kMtkPart; ++k) val[k] = 0.0;
  if (holds) {
    const double* coef = st.coef + kMtkCoef * s;
    const double m = st.mass[i];
    double f[3], a[3], v[3];
    for (int k = 0; k < 3; ++k) {
      f[k] = forces[3 * i + k];
      a[k] = kKappa * f[k] / m;
      v[k] = st.v[3 * i + k];
    }
    if (fl & M3G_DYN_STARTED) axpby(v, coef + kKickV, a, coef + kKickA);   // the finish kick (k_mtk_apply writes it)
    val[kPK + 0] = m * v[0] * v[0];
    val[kPK + 1] = m * v[1] * v[1];
    val[kPK + 2] = m * v[2] * v[2];
    val[kPK + 3] = m * v[1] * v[2];
    val[kPK + 4] = m * v[2] * v[0];
    val[kPK + 5] = m * v[0] * v[1];
    for (int k = 0; k < 3; ++k) {
      val[kPMv + k] = m * v[k];
      val[kPF + k] = f[k];
    }
    val[kPBad] = (std::isfinite(f[0]) && std::isfinite(f[1]) && std::isfinite(f[2])) ? 0.0 : 1.0;   // (not forces_finite: it moves this kernel's compares)
  }
  reduce_store<kMtkPart>(val, c, t, st.partial);
}

__global__ void __launch_bounds__(kWave * kFinalizeWaves) k_mtk_finalize(MtkView st, m3g_mtk_params p, int32_t finish_only,
                                                                         const float* __restrict__ stresses, double* __restrict__ lattice,
                                                                         float* __restrict__ lattice32, double* __restrict__ obs) {
  __shared__ double rows[kFinalizeWaves][chain_row(kMaxChain)];   // lane 0's chain row: the serial arithmetic runs out of LDS
  const int lane = threadIdx.x % kWave;
  const int64_t s = (int64_t)blockIdx.x * kFinalizeWaves + threadIdx.x / kWave;
  if (s >= st.ch.S) return;   // (whole waves: s is uniform across a wave)
  const int fl = st.flags[s];
  double* coef = st.coef + kMtkCoef * s;
  if (fl & M3G_DYN_ERROR) {
    if (lane == 0) coef[kAct] = 0.0;
    return;
  }
  double acc[kMtkPart];
  wave_chunk_sum<kMtkPart>(st.ch, s, st.partial, lane, acc);
  const double n = (double)(st.ch.offsets[s + 1] - st.ch.offsets[s]);
  const double g = p.fix_com ? 3.0 * n - 3.0 : 3.0 * n;
  const double h = 0.5 * p.dt;
  double* L = lattice + 9 * s;

  // ---- lane 0: the verdicts, both T(h) and the observables; the other lanes wait for its verdict, lambda and vg ------------------
  int verdict = 0;   // 0 flagged, 1 finished only, 2 finished and started
  double lam = 1.0, vg[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (lane == 0) {
    const float* sv = stresses + 6 * s;
    bool bad = acc[kPBad] != 0.0;
    for (int k = 0; k < 6; ++k) bad = bad || !std::isfinite(sv[k]);
    if (!bad) {   // never move a structure with non-finite forces or stresses
      const int M = st.M, n_c = p.chain_substeps;
      const bool full = p.cell_mask == M3G_MTK_CELL_FULL;
      double* chain = st.chain + chain_row(M) * s;
      double* row = rows[threadIdx.x / kWave];
      for (int k = 0; k < chain_row(M); ++k) row[k] = chain[k];
      double *xi = row, *vxi = row + M, *xib = row + 2 * M, *vxib = row + 3 * M;
      for (int k = 0; k < 6; ++k) vg[k] = row[4 * M + k];

      const double n_cell = full ? 6.0 : 3.0;
      const double kt = kBoltzmann * st.t0[s], gkt = g * kt;
      const double qk = kt * p.taut * p.taut, q0 = g * qk;
      const double qbk = kt * p.taup * p.taup, qb0 = n_cell * qbk, wg = (g + 3.0) * qbk / 3.0;
      double K[6], W[6];
      for (int k = 0; k < 6; ++k) K[k] = acc[kPK + k] / kKappa;
      const double vol = cell_volume(L);
      for (int k = 0; k < 6; ++k) W[k] = vol * (double)sv[k];   // the virial, W = V * stresses
      auto kick_vg = [&]() {   // vg += h G
        const double iso = (K[0] + K[1] + K[2]) / g - vol * p.pressure;
        for (int k = 0; k < 3; ++k) vg[k] += h * ((K[k] + W[k] + iso) / wg);
        if (full)
          for (int k = 3; k < 6; ++k) vg[k] += h * ((K[k] + W[k]) / wg);
      };
      auto norm2 = [&]() { return vg[0] * vg[0] + vg[1] * vg[1] + vg[2] * vg[2] + 2.0 * (vg[3] * vg[3] + vg[4] * vg[4] + vg[5] * vg[5]); };
      auto baro_chain = [&]() {
        double kb2 = wg * norm2();
        const double sb = chain_half_step(qb0, qbk, xib, vxib, M, n_c, kb2, n_cell * kt, kt, h);
        for (int k = 0; k < 6; ++k) vg[k] *= sb;
      };
      auto scale_k = [&](double sc) {
        for (int k = 0; k < 6; ++k) K[k] *= sc * sc;
      };

      double s1 = 1.0, k2 = K[0] + K[1] + K[2];
      if (fl & M3G_DYN_STARTED) {   // the T(h) that ends the step under way
        kick_vg();
        baro_chain();
        s1 = chain_half_step(q0, qk, xi, vxi, M, n_c, k2, gkt, kt, h);
        scale_k(s1);
      }
      k2 = K[0] + K[1] + K[2];
      double o[M3G_MTK_OBS];
      {
        double ext = gkt * xi[0] + 0.5 * q0 * vxi[0] * vxi[0], tail = 0.0, tailb = 0.0;
        for (int k = 1; k < M; ++k) {
          tail += xi[k];
          ext += 0.5 * qk * vxi[k] * vxi[k];
        }
        ext += kt * tail;
        ext += p.pressure * vol + 0.5 * wg * norm2();
        ext += n_cell * kt * xib[0] + 0.5 * qb0 * vxib[0] * vxib[0];
        for (int k = 1; k < M; ++k) {
          tailb += xib[k];
          ext += 0.5 * qbk * vxib[k] * vxib[k];
        }
        ext += kt * tailb;
        for (int k = 0; k < 6; ++k) o[6 + k] = (W[k] + K[k]) / vol;
        o[0] = 0.5 * k2;
        o[1] = k2 / (3.0 * n * kBoltzmann);
        o[2] = (o[6] + o[7] + o[8]) / 3.0;
        o[3] = vol;
        o[4] = ext;
        o[5] = 0.0;
      }
      lam = s1;
      if (!finish_only) {   // the T(h) that opens the next step
        const double s2 = chain_half_step(q0, qk, xi, vxi, M, n_c, k2, gkt, kt, h);
        scale_k(s2);
        lam = s1 * s2;
        baro_chain();
        kick_vg();
      }
      double rate = 0.0;
      for (int k = 0; k < 6; ++k) rate = max_nan(rate, fabs(vg[k]) * p.dt);
      bad = !(rate <= kMaxRate);   // the matrix series below are exact to fp64 up to this rate only
      if (!bad) {   // nothing of this call was written before this line
        if (obs)
          for (int k = 0; k < M3G_MTK_OBS; ++k) obs[M3G_MTK_OBS * s + k] = o[k];
        for (int k = 0; k < 4 * M; ++k) chain[k] = row[k];
        for (int k = 0; k < 6; ++k) chain[4 * M + k] = vg[k];
        coef[kFinish] = (fl & M3G_DYN_STARTED) ? 1.0 : 0.0;
        for (int k = 0; k < 12; ++k) coef[kFinV + k] = coef[kKickV + k];
        coef[kLam] = lam;
        if (finish_only) {
          st.flags[s] = fl & ~M3G_DYN_STARTED;
          coef[kAct] = 1.0;
          verdict = 1;
        } else {
          st.flags[s] = fl | M3G_DYN_STARTED;
          st.steps[s] += 1;
          coef[kAct] = 2.0;
          verdict = 2;
        }
      }
    }
    if (bad) {
      st.flags[s] = fl | M3G_DYN_ERROR;
      coef[kAct] = 0.0;
    }
  }
  verdict = __shfl(verdict, 0, kWave);
  if (verdict != 2) return;   // (uniform across the wave)
  lam = __shfl(lam, 0, kWave);
  for (int k = 0; k < 6; ++k) vg[k] = __shfl(vg[k], 0, kWave);

  // ---- lanes 0 .. 3, one matrix function each: exp(-B), h phi1(-B), exp(A), dt phi1(A); B = (vg + (tr vg / g) I) h, A = vg dt --------
  const int fn = lane & 3;   // (the lanes above 3 repeat these four and write nothing)
  const bool kick = fn < 2, phi = fn & 1;
  const double iso = kick ? (vg[0] + vg[1] + vg[2]) / g : 0.0, by = kick ? -h : p.dt;
  double a[6], q[6] = {1.0, 1.0, 1.0, 0.0, 0.0, 0.0};
  for (int k = 0; k < 6; ++k) a[k] = (vg[k] + (k < 3 ? iso : 0.0)) * by;
#pragma unroll
  for (int k = kOrder; k > 0; --k) horner_step(a, q, phi ? 1.0 / (k + 1) : 1.0 / k);
  if (phi)
    for (int k = 0; k < 6; ++k) q[k] *= kick ? h : p.dt;
  if (lane < 4)
    for (int k = 0; k < 6; ++k) coef[kKickV + 6 * fn + k] = q[k];
  double ka[6];
  for (int k = 0; k < 6; ++k) ka[k] = __shfl(q[k], 1, kWave);
  if (lane == 0) {   // q = KV
    double mv[3] = {lam * acc[kPMv], lam * acc[kPMv + 1], lam * acc[kPMv + 2]};
    const double fs[3] = {kKappa * acc[kPF], kKappa * acc[kPF + 1], kKappa * acc[kPF + 2]};
    axpby(mv, q, fs, ka);
    for (int k = 0; k < 3; ++k) coef[kPbar + k] = p.fix_com ? mv[k] / n : 0.0;
  }
  if (lane == 2) {   // q = exp(A): lattice = lattice exp(A), row by row
    for (int r = 0; r < 3; ++r) {
      const double x[3] = {L[3 * r], L[3 * r + 1], L[3 * r + 2]};
      double y[3];
      vec_sym(x, q, y);
      for (int k = 0; k < 3; ++k) {
        L[3 * r + k] = y[k];
        if (lattice32) lattice32[9 * s + 3 * r + k] = (float)y[k];
      }
    }
  }
}

__global__ void __launch_bounds__(kChunkRows) k_mtk_apply(MtkView st, int32_t fix_com, const float* __restrict__ forces,
                                                          double* __restrict__ pos) {
  const int c = blockIdx.x;
  if (c >= st.ch.n_chunks()) return;
  const int s = st.ch.structure(c);
  const double* coef = st.coef + kMtkCoef * s;
  const double act = coef[kAct];
  if (act == 0.0) return;   // failed: bitwise untouched
  const int64_t i = st.ch.row(c, threadIdx.x);
  if (!st.ch.holds(s, i)) return;
  const double m = st.mass[i], lam = coef[kLam];
  double a[3], v[3];
  for (int k = 0; k < 3; ++k) {
    a[k] = kKappa * (double)forces[3 * i + k] / m;
    v[k] = st.v[3 * i + k];
  }
  if (coef[kFinish] != 0.0) axpby(v, coef + kFinV, a, coef + kFinA);
  for (int k = 0; k < 3; ++k) v[k] = lam * v[k];
  if (act == 2.0) {
    axpby(v, coef + kKickV, a, coef + kKickA);
    if (fix_com)
      for (int k = 0; k < 3; ++k) v[k] -= coef[kPbar + k] / m;
    double x[3] = {pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]};
    axpby(x, coef + kDriftX, v, coef + kDriftV);
    for (int k = 0; k < 3; ++k) pos[3 * i + k] = x[k];
  }
  for (int k = 0; k < 3; ++k) st.v[3 * i + k] = v[k];
}

// nullptr when the parameters are valid, else what is wrong with them
const char* mtk_params_error(const m3g_mtk_params* p) {
  if (!p) return "null parameters";
  if (p->cell_mask != M3G_MTK_CELL_FULL && p->cell_mask != M3G_MTK_CELL_ORTHORHOMBIC) return "unknown cell_mask";
  if (p->fix_com != 0 && p->fix_com != 1) return "fix_com must be 0 or 1";
  if (p->chain_length < 1 || p->chain_length > kMaxChain) return "chain_length must be in 1 .. 8";
  if (p->chain_substeps < 1 || p->chain_substeps > kMaxChain) return "chain_substeps must be in 1 .. 8";
  if (!finite_positive(p->dt)) return "dt must be finite and > 0";
  if (!finite_positive(p->taut)) return "taut must be finite and > 0";
  if (!finite_positive(p->taup)) return "taup must be finite and > 0";
  if (!std::isfinite(p->pressure)) return "pressure must be finite";
  return nullptr;
}
}  // namespace
}  // namespace m3g

using namespace m3g;

extern "C" int m3g_mtk_state_bytes(int64_t n_atoms, int64_t n_structs, int32_t chain_length, size_t* bytes) {
  if (!bytes || !batch_sizes_ok(n_atoms, n_structs) || !chain_ok(chain_length)) { set_error("m3g_mtk_state_bytes: bad sizes"); return M3G_ERR_VALUE; }
  *bytes = mtk_view(n_atoms, n_structs, chain_length, nullptr).bytes;
  return M3G_OK;
}

extern "C" int m3g_mtk_state_view(int64_t n_atoms, int64_t n_structs, int32_t chain_length, size_t* mass_offset, size_t* velocity_offset) {
  return state_view_offsets("m3g_mtk_state_view", batch_sizes_ok(n_atoms, n_structs) && chain_ok(chain_length),
                            [&] { return mtk_view(n_atoms, n_structs, chain_length, nullptr).view; }, mass_offset, velocity_offset);
}

extern "C" int m3g_mtk_init(const m3g_mtk_params* p, int64_t n_atoms, int64_t n_structs, const int64_t* host_offsets, const double* host_masses,
                            const double* host_temperatures, const double* vel, void* state, size_t state_bytes, void* stream_) {
  if (const char* why = mtk_params_error(p)) { set_error("m3g_mtk_init: invalid parameters: %s", why); return M3G_ERR_VALUE; }
  constexpr const char* fn = "m3g_mtk_init";
  const int64_t N = n_atoms, S = n_structs;
  if (!init_args_ok(fn, N, S, host_offsets && host_masses && host_temperatures && vel && state)) return M3G_ERR_VALUE;
  if (!offsets_ok(fn, host_offsets, N, S)) return M3G_ERR_VALUE;
  for (int64_t i = 0; i < N; ++i)
    if (!mass_ok(fn, host_masses, i)) return M3G_ERR_VALUE;
  for (int64_t s = 0; s < S; ++s) {
    if (!temperature_ok(fn, host_temperatures, s)) return M3G_ERR_VALUE;   // (the chain and barostat masses are proportional to it)
    if (p->fix_com && host_offsets[s + 1] - host_offsets[s] == 1) {
      set_error("m3g_mtk_init: structure %lld holds one atom, which fix_com leaves no degree of freedom", (long long)s);
      return M3G_ERR_VALUE;
    }
  }
  const auto [st, total] = mtk_view(N, S, p->chain_length, state);
  if (!state_fits(fn, state_bytes, total, true)) return M3G_ERR_SIZE;
  const ChunkTable table(host_offsets, S);
  hipStream_t s = (hipStream_t)stream_;
  if (int rc = upload_batch(table, st, host_offsets, host_masses, host_temperatures, nullptr, s)) return rc;
  const int64_t work = 3 * N > S ? 3 * N : S;
  hipLaunchKernelGGL(k_mtk_init, grid_for(work, kChunkRows), dim3(kChunkRows), 0, s, st, vel);
  return launched_and_synced(s);   // (the host tables above go out of scope)
}

extern "C" int m3g_mtk_step(const m3g_mtk_params* p, int64_t n_atoms, int64_t n_structs, void* state, size_t state_bytes, const float* forces,
                            const float* stresses, double* pos, double* lattice, float* lattice32, int32_t finish_only, double* obs, void* stream_) {
  if (const char* why = mtk_params_error(p)) { set_error("m3g_mtk_step: invalid parameters: %s", why); return M3G_ERR_VALUE; }
  const int64_t N = n_atoms, S = n_structs;
  if (!batch_sizes_ok(N, S) || !state || !forces || !pos) { set_error("m3g_mtk_step: null argument or bad sizes"); return M3G_ERR_VALUE; }
  if (!stresses || !lattice) { set_error("m3g_mtk_step: needs the stresses and the fp64 lattice"); return M3G_ERR_VALUE; }
  const auto [st, total] = mtk_view(N, S, p->chain_length, state);
  if (!state_fits("m3g_mtk_step", state_bytes, total)) return M3G_ERR_SIZE;
  hipStream_t s = (hipStream_t)stream_;
  const auto [chunks, waves] = step_grids(N, S);
  hipLaunchKernelGGL(k_mtk_partials, chunks, dim3(kChunkRows), 0, s, st, forces);
  hipLaunchKernelGGL(k_mtk_finalize, waves, dim3(kFinalizeThreads), 0, s, st, *p, finish_only, stresses, lattice, lattice32, obs);
  hipLaunchKernelGGL(k_mtk_apply, chunks, dim3(kChunkRows), 0, s, st, p->fix_com, forces, pos);
  M3G_RETURN_LAUNCH_STATUS();
}

extern "C" int m3g_mtk_read(int64_t n_atoms, int64_t n_structs, int32_t chain_length, const void* state, size_t state_bytes, int32_t* host_flags,
                            int64_t* host_steps, double* host_vel, double* host_chain, void* stream_) {
  const int64_t N = n_atoms, S = n_structs;
  if (!batch_sizes_ok(N, S) || !chain_ok(chain_length) || !state) { set_error("m3g_mtk_read: null argument or bad sizes"); return M3G_ERR_VALUE; }
  const auto [st, total] = mtk_view(N, S, chain_length, (void*)state);
  if (!state_fits("m3g_mtk_read", state_bytes, total)) return M3G_ERR_SIZE;
  hipStream_t s = (hipStream_t)stream_;
  if (int rc = read_head(st, host_flags, host_steps, host_vel, s)) return rc;
  M3G_HIP_CHECK(read_back(host_chain, st.chain, (size_t)chain_row(chain_length) * S, s));
  M3G_HIP_CHECK(hipStreamSynchronize(s));
  return M3G_OK;
}
