// Batched L-BFGS structure relaxation beside FIRE (m3g_relax.hip), fixed or variable cell: ASE's LBFGS without line search applied to
// every structure on its own, in the dot-product-space form -- the two-loop recursion runs on coefficient vectors over the basis
// {s_i}, {y_i}, grad, from that structure's Gram matrix, so no pass over the rows depends on another and one iteration of the whole
// batch is FIVE launches whatever the memory, the history depth reached and the batch (three when check_only):
//   k_lbfgs_gather     one workgroup per chunk (<= kChunkRows atoms of ONE structure): grad = -g of its rows, s_new = X - X_prev and
//                      y_new = grad - grad_prev into the ring's spare slot, the chunk partials of their inner products with each other
//                      and with every stored s_i, y_i, and max_i |g_i|^2;
//   k_lbfgs_solve      one wave per structure: the partials in chunk order plus the three cell rows, the convergence / error verdict,
//                      the new pair committed (y.s finite and non-zero) or rejected, the Gram matrix updated, both loops on the
//                      coefficients, and the coefficients of p = c_g grad + sum_i (c_y,i y_i + c_s,i s_i) (and p of the cell rows);
//   k_lbfgs_direction  one workgroup per chunk: p of its rows, the chunk maximum of |p_row|^2;
//   k_lbfgs_finalize   one workgroup: per structure the longest row of p, the clip, the error verdict of a non-finite step, the cell rows
//                      moved and the cell written; writes the number of structures still relaxing to the caller's word;
//   k_lbfgs_apply      one workgroup per chunk: X_prev, grad_prev, X and the caller's positions of the structures that moved.
// The ring holds memory + 1 slots per vector: the spare one takes the candidate pair, so that a rejected pair evicts nothing.  No
// atomics: every sum runs over the structure's own rows, chunks and slots in a fixed order (chunks never straddle structures), so results
// are bitwise reproducible and independent of the rest of the batch.  No allocation, copy or wait in m3g_lbfgs_step (capture-safe).
#include <cmath>

#include "m3g_cell_filter.h"
#include "m3g_chunks.h"
#include "m3g_internal.h"

namespace m3g {
namespace {
constexpr int kCoef = 16;            // per structure: move, c_g, step scale, p of the cell rows [9], (pad)
constexpr int kSlotDots = 5;         // per stored pair i: s_i.y_new, s_i.grad, y_i.s_new, y_i.y_new, y_i.grad
constexpr int kHeadDots = 5;         // s_new.y_new, y_new.y_new, s_new.grad, y_new.grad, max_i |g_i|^2
constexpr int kMaxMemory = 2047;     // the solve kernel keeps 2 (memory + 1) coefficients in LDS

// State buffer, in this order (every region rounded up to 256 bytes), with C = chunk_bound(N, S), R = N + 3 S rows, M = memory + 1:
//   the chunk table; head partials 8*5*C; slot partials 8*5*M*C; chunk maxima of |p_row|^2 8*C;
//   X, X_prev, grad, grad_prev, p: 8*3R each;  the rings of s and y: 8*3R*M each  (the dominant term: memory * 2 * 3(N+3S) * 8);
//   L0, F: 8*9*S each;  the Gram blocks s_i.y_j and y_i.y_j: 8*M*M*S each;  rho, s.grad, y.grad, c_s, c_y: 8*M*S each;
//   ring head, pair count, flags, step count: 4*S each;  coefficients 8*16*S.
struct LbfgsView {
  int64_t N, R;     // atoms; rows of a vector (N + 3 S)
  int M;            // ring slots: memory + 1
  ChunkView ch;
  double *head_part, *slot_part, *pmax, *x, *xprev, *grad, *gprev, *p, *ring_s, *ring_y, *l0, *f, *sy, *yy, *rho, *sg, *yg, *cs, *cy, *coef;
  int32_t *head, *count, *flags, *steps;
  // ring position j (0 = oldest of `count` pairs) -> slot, `head` being the spare slot
  __device__ int slot(int head, int count, int j) const { return (head + M - count + j) % M; }
  __device__ double* s_of(int slot) const { return ring_s + (size_t)slot * 3 * R; }
  __device__ double* y_of(int slot) const { return ring_y + (size_t)slot * 3 * R; }
};
Carved<LbfgsView> lbfgs_view(int64_t N, int64_t S, int64_t memory, void* state) {
  Carve c{state};
  const size_t C = (size_t)chunk_bound(N, S), R = (size_t)(N + 3 * S), M = (size_t)memory + 1, Ss = (size_t)S;
  LbfgsView st{N, N + 3 * S, (int)memory + 1};
  st.ch = chunk_view(N, S, c);
  st.head_part = c.take<double>(kHeadDots * C);
  st.slot_part = c.take<double>(kSlotDots * M * C);
  st.pmax = c.take<double>(C);
  st.x = c.take<double>(3 * R);                // rows: the N atoms, then 3 cell rows per structure
  st.xprev = c.take<double>(3 * R);
  st.grad = c.take<double>(3 * R);
  st.gprev = c.take<double>(3 * R);
  st.p = c.take<double>(3 * R);
  st.ring_s = c.take<double>(3 * R * M);
  st.ring_y = c.take<double>(3 * R * M);
  st.l0 = c.take<double>(9 * Ss);
  st.f = c.take<double>(9 * Ss);
  st.sy = c.take<double>(M * M * Ss);
  st.yy = c.take<double>(M * M * Ss);
  st.rho = c.take<double>(M * Ss);
  st.sg = c.take<double>(M * Ss);
  st.yg = c.take<double>(M * Ss);
  st.cs = c.take<double>(M * Ss);
  st.cy = c.take<double>(M * Ss);
  st.head = c.take<int32_t>(Ss);
  st.count = c.take<int32_t>(Ss);
  st.flags = c.take<int32_t>(Ss);
  st.steps = c.take<int32_t>(Ss);
  st.coef = c.take<double>(kCoef * Ss);
  return {st, c.off};
}

__device__ inline double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// a + b on both partners of every stage, so every lane ends with the same bits
template <int K>
__device__ inline void wave_butterfly_sum(double (&acc)[K]) {
#pragma unroll
  for (int w = kWave / 2; w > 0; w >>= 1)
    for (int j = 0; j < K; ++j) acc[j] += __shfl_xor(acc[j], w, kWave);
}

__global__ void __launch_bounds__(kChunkRows) k_lbfgs_init(LbfgsView st, const double* __restrict__ pos, const double* __restrict__ lattice) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < 3 * st.N) { st.x[i] = pos[i]; st.xprev[i] = pos[i]; st.grad[i] = 0.0; st.gprev[i] = 0.0; st.p[i] = 0.0; }
  if (i < st.ch.S) {
    const double cf = (double)(st.ch.offsets[i + 1] - st.ch.offsets[i]);
    for (int k = 0; k < 9; ++k) {
      const double id = (k % 4 == 0) ? 1.0 : 0.0;
      const int64_t at = 3 * st.N + 9 * i + k;
      st.l0[9 * i + k] = lattice ? lattice[9 * i + k] : 0.0;
      st.f[9 * i + k] = id;
      st.x[at] = cf * id;
      st.xprev[at] = cf * id;
      st.grad[at] = 0.0;
      st.gprev[at] = 0.0;
      st.p[at] = 0.0;
    }
    st.head[i] = 0;
    st.count[i] = 0;
    st.flags[i] = 0;
    st.steps[i] = 0;
    for (int k = 0; k < kCoef; ++k) st.coef[kCoef * i + k] = 0.0;
  }
}

__global__ void __launch_bounds__(kChunkRows) k_lbfgs_gather(LbfgsView st, int32_t relax_cell, const float* __restrict__ forces) {
  __shared__ double sh[kHeadDots][kChunkRows];
  __shared__ double nv[9][kChunkRows];   // s_new, y_new, grad of the chunk's rows (zero beyond the structure's end)
  const int c = blockIdx.x, t = threadIdx.x;
  if (c >= st.ch.n_chunks()) return;
  const int s = st.ch.structure(c);
  const int fl = st.flags[s];
  if (fl & (M3G_LBFGS_CONVERGED | M3G_LBFGS_ERROR)) return;   // frozen: solve reads nothing of it
  const bool started = (fl & M3G_LBFGS_STARTED) != 0;
  const int head = st.head[s], count = st.count[s];
  const int64_t i = st.ch.row(c, t);
  double sn[3] = {0.0, 0.0, 0.0}, yn[3] = {0.0, 0.0, 0.0}, gr[3] = {0.0, 0.0, 0.0};
  double val[kHeadDots] = {0.0, 0.0, 0.0, 0.0, 0.0};
  if (st.ch.holds(s, i)) {
    double g[3];
    gen_force(forces, i, st.f + 9 * s, relax_cell != 0, g);
    for (int k = 0; k < 3; ++k) {
      gr[k] = -g[k];
      st.grad[3 * i + k] = gr[k];
    }
    val[4] = dot3(g, g);
    if (started) {
      double* sr = st.s_of(head) + 3 * i;
      double* yr = st.y_of(head) + 3 * i;
      for (int k = 0; k < 3; ++k) {
        sn[k] = st.x[3 * i + k] - st.xprev[3 * i + k];
        yn[k] = gr[k] - st.gprev[3 * i + k];
        sr[k] = sn[k];
        yr[k] = yn[k];
      }
      val[0] = dot3(sn, yn);
      val[1] = dot3(yn, yn);
      val[2] = dot3(sn, gr);
      val[3] = dot3(yn, gr);
    }
  }
  for (int k = 0; k < 3; ++k) {
    nv[k][t] = sn[k];
    nv[3 + k][t] = yn[k];
    nv[6 + k][t] = gr[k];
  }
  chunk_tree_reduce<kHeadDots, 1>(sh, val, t);   // four sums and a maximum (its first barrier publishes nv as well)
  if (t < kHeadDots) st.head_part[kHeadDots * c + t] = sh[t][0];
  if (!started) return;
  // every stored pair against the new vectors: one wave per pair, a lane's rows in row order, then the butterfly
  const int wave = t / kWave, lane = t % kWave;
  for (int j = wave; j < count; j += kChunkRows / kWave) {
    const int a = st.slot(head, count, j);
    const double* sa = st.s_of(a);
    const double* ya = st.y_of(a);
    double acc[kSlotDots] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int r = lane; r < kChunkRows; r += kWave) {
      const int64_t row = st.ch.row(c, r);
      if (!st.ch.holds(s, row)) break;
      const double sv[3] = {sa[3 * row], sa[3 * row + 1], sa[3 * row + 2]};
      const double yv[3] = {ya[3 * row], ya[3 * row + 1], ya[3 * row + 2]};
      const double n_s[3] = {nv[0][r], nv[1][r], nv[2][r]}, n_y[3] = {nv[3][r], nv[4][r], nv[5][r]}, n_g[3] = {nv[6][r], nv[7][r], nv[8][r]};
      acc[0] += dot3(sv, n_y);
      acc[1] += dot3(sv, n_g);
      acc[2] += dot3(yv, n_s);
      acc[3] += dot3(yv, n_y);
      acc[4] += dot3(yv, n_g);
    }
    wave_butterfly_sum(acc);
    if (lane == 0)
      for (int q = 0; q < kSlotDots; ++q) st.slot_part[((size_t)c * st.M + a) * kSlotDots + q] = acc[q];
  }
}

__global__ void __launch_bounds__(kWave) k_lbfgs_solve(LbfgsView st, m3g_lbfgs_params p, int32_t check_only, const float* __restrict__ stresses,
                                                      const double* __restrict__ lattice) {
  extern __shared__ double lds[];
  double* alpha = lds;            // [M], by ring position
  double* cc = lds + st.M;        // [M]: a_i - b_i
  const int64_t s = blockIdx.x;
  const int lane = threadIdx.x;
  double* coef = st.coef + kCoef * s;
  const int fl = st.flags[s];
  if (lane == 0) coef[0] = 0.0;
  if (fl & (M3G_LBFGS_CONVERGED | M3G_LBFGS_ERROR)) return;
  const bool started = (fl & M3G_LBFGS_STARTED) != 0, cell = p.relax_cell != 0;
  const int M = st.M;
  int head = st.head[s], count = st.count[s];
  const int c0 = st.ch.chunks_begin(s), c1 = st.ch.chunks_end(s);
  // the head partials: lane-strided in chunk order, then the butterfly
  double hp[4] = {0.0, 0.0, 0.0, 0.0}, g2 = 0.0;
  for (int c = c0 + lane; c < c1; c += kWave) {
    for (int q = 0; q < 4; ++q) hp[q] += st.head_part[kHeadDots * c + q];
    g2 = max_nan(g2, st.head_part[kHeadDots * c + 4]);
  }
  wave_butterfly_sum(hp);
  for (int w = kWave / 2; w > 0; w >>= 1) g2 = max_nan(g2, __shfl_xor(g2, w, kWave));
  // the three cell rows, serially (every lane the same arithmetic)
  const int64_t cell_at = 3 * st.N + 9 * s;
  double grc[9], snc[9], ync[9];
  for (int k = 0; k < 9; ++k) grc[k] = snc[k] = ync[k] = 0.0;
  if (cell) {
    const double cf = (double)(st.ch.offsets[s + 1] - st.ch.offsets[s]);   // ASE's cell_factor: the structure's atom count
    double gc[9];
    cell_gen_force(st.f + 9 * s, lattice + 9 * s, stresses + 6 * s, cf, gc);
    for (int k = 0; k < 9; ++k) grc[k] = -gc[k];
    if (started)
      for (int k = 0; k < 9; ++k) {
        snc[k] = st.x[cell_at + k] - st.xprev[cell_at + k];
        ync[k] = grc[k] - st.gprev[cell_at + k];
      }
    for (int r = 0; r < 3; ++r) {
      g2 = max_nan(g2, dot3(gc + 3 * r, gc + 3 * r));
      hp[0] += dot3(snc + 3 * r, ync + 3 * r);
      hp[1] += dot3(ync + 3 * r, ync + 3 * r);
      hp[2] += dot3(snc + 3 * r, grc + 3 * r);
      hp[3] += dot3(ync + 3 * r, grc + 3 * r);
    }
  }
  if (!std::isfinite(g2)) {   // never move a structure onto non-finite positions
    if (lane == 0) st.flags[s] = fl | M3G_LBFGS_ERROR;
    return;
  }
  if (g2 < p.fmax * p.fmax) {   // ASE: (forces**2).sum(axis=1).max() < fmax**2 -> frozen from here on
    if (lane == 0) st.flags[s] = fl | M3G_LBFGS_CONVERGED;
    return;
  }
  if (check_only) return;
  double* sy = st.sy + (size_t)s * M * M;   // sy[a * M + b] = s_a . y_b
  double* yy = st.yy + (size_t)s * M * M;
  double* rho = st.rho + (size_t)s * M;
  double* sg = st.sg + (size_t)s * M;
  double* yg = st.yg + (size_t)s * M;
  if (lane == 0 && cell) {
    for (int k = 0; k < 9; ++k) {
      st.grad[cell_at + k] = grc[k];
      if (started) {
        st.s_of(head)[cell_at + k] = snc[k];
        st.y_of(head)[cell_at + k] = ync[k];
      }
    }
  }
  // every stored pair against the new vectors and grad: a lane per pair, its chunk partials in chunk order, then the cell rows
  for (int j = lane; j < count; j += kWave) {
    const int a = st.slot(head, count, j);
    double d[kSlotDots] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int c = c0; c < c1; ++c)
      for (int q = 0; q < kSlotDots; ++q) d[q] += st.slot_part[((size_t)c * M + a) * kSlotDots + q];
    if (cell) {
      const double* sa = st.s_of(a) + cell_at;
      const double* ya = st.y_of(a) + cell_at;
      for (int r = 0; r < 3; ++r) {
        d[0] += dot3(sa + 3 * r, ync + 3 * r);
        d[1] += dot3(sa + 3 * r, grc + 3 * r);
        d[2] += dot3(ya + 3 * r, snc + 3 * r);
        d[3] += dot3(ya + 3 * r, ync + 3 * r);
        d[4] += dot3(ya + 3 * r, grc + 3 * r);
      }
    }
    sy[a * M + head] = d[0];   // (the spare slot's row and column: read only once the pair is committed)
    sy[head * M + a] = d[2];
    yy[a * M + head] = d[3];
    yy[head * M + a] = d[3];
    sg[a] = d[1];
    yg[a] = d[4];
  }
  // commit the pair unless y.s is zero or not finite (ASE would divide by zero; equal fp32 forces twice give y = 0)
  if (started && hp[0] != 0.0 && std::isfinite(hp[0])) {
    if (lane == 0) {
      sy[head * M + head] = hp[0];
      yy[head * M + head] = hp[1];
      rho[head] = 1.0 / hp[0];
      sg[head] = hp[2];
      yg[head] = hp[3];
    }
    if (count < M - 1) ++count;   // else the oldest pair's slot becomes the spare one
    head = (head + 1) % M;
    if (lane == 0) {
      st.head[s] = head;
      st.count[s] = count;
    }
  }
  __threadfence_block();
  __syncthreads();
  // first loop, newest to oldest: a_i = rho_i s_i.q with q = grad - sum_{j newer} a_j y_j
  for (int j = count - 1; j >= 0; --j) {
    const int a = st.slot(head, count, j);
    double part[1] = {0.0};
    for (int jj = j + 1 + lane; jj < count; jj += kWave) part[0] += alpha[jj] * sy[a * M + st.slot(head, count, jj)];
    wave_butterfly_sum(part);
    const double al = rho[a] * (sg[a] - part[0]);
    if (lane == 0) alpha[j] = al;
    __syncthreads();
  }
  // second loop, oldest to newest: z = H0 q + sum_{j older} s_j (a_j - b_j), b_i = rho_i y_i.z
  const double h0 = 1.0 / p.alpha;
  for (int j = 0; j < count; ++j) {
    const int a = st.slot(head, count, j);
    double part[2] = {0.0, 0.0};
    for (int jj = lane; jj < count; jj += kWave) {
      const int b = st.slot(head, count, jj);
      part[0] += alpha[jj] * yy[a * M + b];
      if (jj < j) part[1] += cc[jj] * sy[b * M + a];
    }
    wave_butterfly_sum(part);
    const double yz = h0 * (yg[a] - part[0]) + part[1];
    if (lane == 0) cc[j] = alpha[j] - rho[a] * yz;
    __syncthreads();
  }
  // p = -z = -H0 grad + sum_i (H0 a_i y_i - (a_i - b_i) s_i)
  double* cs = st.cs + (size_t)s * M;
  double* cy = st.cy + (size_t)s * M;
  for (int j = lane; j < count; j += kWave) {
    const int a = st.slot(head, count, j);
    cs[a] = -cc[j];
    cy[a] = h0 * alpha[j];
  }
  if (lane == 0) {
    coef[0] = 1.0;
    coef[1] = -h0;
    if (cell) {
      double pc[9];
      for (int k = 0; k < 9; ++k) pc[k] = -h0 * grc[k];
      for (int j = 0; j < count; ++j) {
        const int a = st.slot(head, count, j);
        const double ca = h0 * alpha[j], cb = -cc[j];
        const double* sa = st.s_of(a) + cell_at;
        const double* ya = st.y_of(a) + cell_at;
        for (int k = 0; k < 9; ++k) {
          pc[k] += ca * ya[k];
          pc[k] += cb * sa[k];
        }
      }
      for (int k = 0; k < 9; ++k) coef[3 + k] = pc[k];
    }
  }
}

__global__ void __launch_bounds__(kChunkRows) k_lbfgs_direction(LbfgsView st) {
  __shared__ double sh[1][kChunkRows];
  const int c = blockIdx.x, t = threadIdx.x;
  if (c >= st.ch.n_chunks()) return;
  const int s = st.ch.structure(c);
  const double* coef = st.coef + kCoef * s;
  if (coef[0] == 0.0) return;   // converged, failed or checked only
  const int head = st.head[s], count = st.count[s];
  const double* cs = st.cs + (size_t)s * st.M;
  const double* cy = st.cy + (size_t)s * st.M;
  const int64_t i = st.ch.row(c, t);
  double val[1] = {0.0};
  if (st.ch.holds(s, i)) {
    const double cg = coef[1];
    double pr[3];
    for (int k = 0; k < 3; ++k) pr[k] = cg * st.grad[3 * i + k];
    for (int j = 0; j < count; ++j) {   // oldest to newest
      const int a = st.slot(head, count, j);
      const double ca = cy[a], cb = cs[a];
      const double* ya = st.y_of(a) + 3 * i;
      const double* sa = st.s_of(a) + 3 * i;
      for (int k = 0; k < 3; ++k) {
        pr[k] += ca * ya[k];
        pr[k] += cb * sa[k];
      }
    }
    for (int k = 0; k < 3; ++k) st.p[3 * i + k] = pr[k];
    val[0] = dot3(pr, pr);
  }
  chunk_tree_reduce<1, 1>(sh, val, t);
  if (t == 0) st.pmax[c] = sh[0][0];
}

__global__ void __launch_bounds__(kChunkRows) k_lbfgs_finalize(LbfgsView st, m3g_lbfgs_params p, int32_t check_only, double* __restrict__ lattice,
                                                              float* __restrict__ lattice32, int32_t* host_unconverged) {
  __shared__ int cnt_sh[1][kChunkRows];
  const int t = threadIdx.x;
  int cnt = 0;
  for (int64_t s = t; s < st.ch.S; s += kChunkRows) {
    double* coef = st.coef + kCoef * s;
    const int fl = st.flags[s];
    if (fl & (M3G_LBFGS_CONVERGED | M3G_LBFGS_ERROR)) continue;
    if (check_only) { ++cnt; continue; }
    const bool cell = p.relax_cell != 0;
    double p2 = 0.0;
    for (int c = st.ch.chunks_begin(s); c < st.ch.chunks_end(s); ++c) p2 = max_nan(p2, st.pmax[c]);   // serial, in chunk order
    if (cell)
      for (int r = 0; r < 3; ++r) p2 = max_nan(p2, dot3(coef + 3 + 3 * r, coef + 3 + 3 * r));
    if (!std::isfinite(p2)) {   // a non-finite step: flagged, not moved
      st.flags[s] = fl | M3G_LBFGS_ERROR;
      coef[0] = 0.0;
      continue;
    }
    ++cnt;
    const double longest = sqrt(p2);   // per ROW, cell rows included (not FIRE's norm over the whole structure)
    const double scale = longest >= p.maxstep ? p.maxstep / longest : 1.0;
    coef[2] = scale;
    st.flags[s] = fl | M3G_LBFGS_STARTED;
    st.steps[s] += 1;
    if (cell) {
      const double cf = (double)(st.ch.offsets[s + 1] - st.ch.offsets[s]);
      const int64_t cell_at = 3 * st.N + 9 * s;
      double Fn[9];
      for (int k = 0; k < 9; ++k) {
        const double xo = st.x[cell_at + k];
        const double xn = xo + p.damping * (coef[3 + k] * scale);
        st.xprev[cell_at + k] = xo;
        st.gprev[cell_at + k] = st.grad[cell_at + k];
        st.x[cell_at + k] = xn;
        Fn[k] = xn / cf;
        st.f[9 * s + k] = Fn[k];
      }
      deformed_lattice(st.l0 + 9 * s, Fn, lattice + 9 * s, lattice32 ? lattice32 + 9 * s : nullptr);
    }
  }
  const int val[1] = {cnt};
  chunk_tree_reduce<1>(cnt_sh, val, t);
  if (t == 0 && host_unconverged) *host_unconverged = cnt_sh[0][0];
}

__global__ void __launch_bounds__(kChunkRows) k_lbfgs_apply(LbfgsView st, int32_t relax_cell, double damping, double* __restrict__ pos) {
  const int c = blockIdx.x;
  if (c >= st.ch.n_chunks()) return;
  const int s = st.ch.structure(c);
  const double* coef = st.coef + kCoef * s;
  if (coef[0] == 0.0) return;   // converged, failed or checked only: bitwise untouched
  const int64_t i = st.ch.row(c, threadIdx.x);
  if (!st.ch.holds(s, i)) return;
  const double scale = coef[2];
  double xn[3];
  for (int k = 0; k < 3; ++k) {
    const double xo = st.x[3 * i + k];
    xn[k] = xo + damping * (st.p[3 * i + k] * scale);
    st.xprev[3 * i + k] = xo;
    st.gprev[3 * i + k] = st.grad[3 * i + k];
    st.x[3 * i + k] = xn[k];
  }
  deformed_pos(xn, st.f + 9 * s, relax_cell != 0, pos + 3 * i);   // (F': finalize has written it)
}

bool lbfgs_params_ok(const m3g_lbfgs_params* p) {
  return p && finite_positive(p->maxstep) && finite_positive(p->damping) && finite_positive(p->alpha) && finite_positive(p->fmax) &&
         p->memory >= 1 && p->memory <= kMaxMemory && (p->relax_cell == 0 || p->relax_cell == 1);
}
constexpr const char* kBadParams = "invalid L-BFGS parameters (maxstep, damping, alpha, fmax > 0; 1 <= memory <= 2047; relax_cell 0 or 1)";
}  // namespace
}  // namespace m3g

using namespace m3g;

extern "C" int m3g_lbfgs_state_bytes(int64_t n_atoms, int64_t n_structs, int32_t memory, size_t* bytes) {
  if (!bytes || !batch_sizes_ok(n_atoms, n_structs) || memory < 1 || memory > kMaxMemory) {
    set_error("m3g_lbfgs_state_bytes: bad sizes (1 <= memory <= %d)", kMaxMemory);
    return M3G_ERR_VALUE;
  }
  *bytes = lbfgs_view(n_atoms, n_structs, memory, nullptr).bytes;
  return M3G_OK;
}

extern "C" int m3g_lbfgs_init(const m3g_lbfgs_params* p, int64_t n_atoms, int64_t n_structs, const int64_t* host_offsets, const double* pos,
                              const double* lattice, void* state, size_t state_bytes, void* stream_) {
  if (!lbfgs_params_ok(p)) { set_error("m3g_lbfgs_init: %s", kBadParams); return M3G_ERR_VALUE; }
  const int64_t N = n_atoms, S = n_structs;
  if (!init_args_ok("m3g_lbfgs_init", N, S, host_offsets && pos && state && (lattice || !p->relax_cell))) return M3G_ERR_VALUE;
  if (!offsets_ok("m3g_lbfgs_init", host_offsets, N, S)) return M3G_ERR_VALUE;
  const auto [st, total] = lbfgs_view(N, S, p->memory, state);
  if (!state_fits("m3g_lbfgs_init", state_bytes, total, true)) return M3G_ERR_SIZE;
  const ChunkTable table(host_offsets, S);
  hipStream_t s = (hipStream_t)stream_;
  if (int rc = table.upload(st.ch, host_offsets, s)) return rc;
  const int64_t work = 3 * N > S ? 3 * N : S;
  hipLaunchKernelGGL(k_lbfgs_init, grid_for(work, kChunkRows), dim3(kChunkRows), 0, s, st, pos, lattice);
  return launched_and_synced(s);   // (the host tables above go out of scope)
}

extern "C" int m3g_lbfgs_step(const m3g_lbfgs_params* p, int64_t n_atoms, int64_t n_structs, void* state, size_t state_bytes, const float* forces,
                              const float* stresses, double* pos, double* lattice, float* lattice32, int32_t check_only, int32_t* unconverged,
                              void* stream_) {
  if (!lbfgs_params_ok(p)) { set_error("m3g_lbfgs_step: %s", kBadParams); return M3G_ERR_VALUE; }
  const int64_t N = n_atoms, S = n_structs;
  if (!batch_sizes_ok(N, S) || !state || !forces || !pos) { set_error("m3g_lbfgs_step: null argument or bad sizes"); return M3G_ERR_VALUE; }
  if (p->relax_cell && (!stresses || !lattice)) { set_error("m3g_lbfgs_step: a cell relaxation needs stresses and the fp64 lattice"); return M3G_ERR_VALUE; }
  const auto [st, total] = lbfgs_view(N, S, p->memory, state);
  if (!state_fits("m3g_lbfgs_step", state_bytes, total)) return M3G_ERR_SIZE;
  hipStream_t s = (hipStream_t)stream_;
  const dim3 grid((unsigned)chunk_bound(N, S));   // workgroups beyond the table's chunk count return at once
  const size_t lds = 2 * sizeof(double) * (size_t)st.M;
  hipLaunchKernelGGL(k_lbfgs_gather, grid, dim3(kChunkRows), 0, s, st, p->relax_cell, forces);
  hipLaunchKernelGGL(k_lbfgs_solve, dim3((unsigned)S), dim3(kWave), lds, s, st, *p, check_only, stresses, lattice);
  if (!check_only) hipLaunchKernelGGL(k_lbfgs_direction, grid, dim3(kChunkRows), 0, s, st);
  hipLaunchKernelGGL(k_lbfgs_finalize, dim3(1), dim3(kChunkRows), 0, s, st, *p, check_only, lattice, lattice32, unconverged);
  if (!check_only) hipLaunchKernelGGL(k_lbfgs_apply, grid, dim3(kChunkRows), 0, s, st, p->relax_cell, p->damping, pos);
  M3G_RETURN_LAUNCH_STATUS();
}

extern "C" int m3g_lbfgs_read(int64_t n_atoms, int64_t n_structs, int32_t memory, const void* state, size_t state_bytes, int32_t* host_flags,
                              int32_t* host_steps, int32_t* host_pairs, double* host_x, void* stream_) {
  const int64_t N = n_atoms, S = n_structs;
  if (!batch_sizes_ok(N, S) || !state || memory < 1 || memory > kMaxMemory) { set_error("m3g_lbfgs_read: null argument or bad sizes"); return M3G_ERR_VALUE; }
  const auto [st, total] = lbfgs_view(N, S, memory, (void*)state);
  if (!state_fits("m3g_lbfgs_read", state_bytes, total)) return M3G_ERR_SIZE;
  return read_all((hipStream_t)stream_,
                  {rb(host_flags, st.flags, S), rb(host_steps, st.steps, S), rb(host_pairs, st.count, S), rb(host_x, st.x, 3 * st.R)});
}
