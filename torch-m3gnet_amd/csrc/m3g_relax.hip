// Batched FIRE structure relaxation, fixed or variable cell (linear deformation gradient, as ASE's UnitCellFilter).  The reference's
// relaxation script (scripts/relax_org.py) hands one structure at a time to m3gnet's Relaxer: ASE's FIRE on the host, one optimiser per
// structure, several small array operations and host reductions per step.  Here one iteration of the whole batch is three launches:
//   k_fire_partials   one workgroup per chunk (<= kChunkRows atoms of ONE structure): generalized forces g of its rows and the partial
//                     sums g.v, g.g, v.v, max_i |g_i|^2, in a fixed tree order;
//   k_fire_finalize   one workgroup: per structure, the chunk partials in chunk order (+ the three cell rows), convergence / error
//                     verdict, the FIRE scalars (dt, a, n), the mixing coefficients of v' = c_v v + c_g g and the step scale -- |v'|^2
//                     in closed form from the three sums, so no second pass over the rows -- and the cell rows themselves; writes the
//                     number of structures still relaxing to the caller's word;
//   k_fire_apply      one workgroup per chunk: v, X and the caller's positions of the structures that moved.
// No atomics: every sum depends on the structure's own rows only (chunks never straddle structures), so results are bitwise
// reproducible and independent of the rest of the batch.  No allocation, copy or wait in m3g_fire_step (capture-safe).
#include <cmath>

#include "m3g_chunks.h"
#include "m3g_internal.h"

namespace m3g {
namespace {
constexpr int kCoef = 24;        // per structure: move, c_v, c_g, step scale, F before [9], F after [9], (pad)

struct FireView {
  int64_t N;
  ChunkView ch;
  double *partial, *x, *v, *l0, *f, *dt, *a, *coef;
  int32_t *n, *flags, *steps;
};
Carved<FireView> fire_view(int64_t N, int64_t S, void* state) {
  Carve c{state};
  const int64_t C = chunk_bound(N, S), R = N + 3 * S;
  FireView st{N};
  st.ch = chunk_view(N, S, c);
  st.partial = c.take<double>(4 * C);
  st.x = c.take<double>(3 * R);                // rows: the N atoms, then 3 cell rows per structure
  st.v = c.take<double>(3 * R);
  st.l0 = c.take<double>(9 * S);
  st.f = c.take<double>(9 * S);
  st.dt = c.take<double>(S);
  st.a = c.take<double>(S);
  st.n = c.take<int32_t>(S);
  st.flags = c.take<int32_t>(S);
  st.steps = c.take<int32_t>(S);
  st.coef = c.take<double>(kCoef * S);
  return {st, c.off};
}

// g = f F (row vector times the deformation gradient), or f itself with the cell fixed
__device__ inline void gen_force(const float* __restrict__ forces, int64_t i, const double* F, bool cell, double g[3]) {
  const double f0 = forces[3 * i], f1 = forces[3 * i + 1], f2 = forces[3 * i + 2];
  if (cell) {
    for (int k = 0; k < 3; ++k) g[k] = f0 * F[k] + f1 * F[3 + k] + f2 * F[6 + k];
  } else {
    g[0] = f0; g[1] = f1; g[2] = f2;
  }
}

__global__ void __launch_bounds__(kChunkRows) k_fire_init(FireView st, const double* __restrict__ pos, const double* __restrict__ lattice,
                                                         double dt0, double astart) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < 3 * st.N) { st.x[i] = pos[i]; st.v[i] = 0.0; }
  if (i < st.ch.S) {
    const double cf = (double)(st.ch.offsets[i + 1] - st.ch.offsets[i]);
    for (int k = 0; k < 9; ++k) {
      const double id = (k % 4 == 0) ? 1.0 : 0.0;
      st.l0[9 * i + k] = lattice ? lattice[9 * i + k] : 0.0;
      st.f[9 * i + k] = id;
      st.x[3 * st.N + 9 * i + k] = cf * id;
      st.v[3 * st.N + 9 * i + k] = 0.0;
    }
    st.dt[i] = dt0;
    st.a[i] = astart;
    st.n[i] = 0;
    st.flags[i] = 0;
    st.steps[i] = 0;
    st.coef[kCoef * i] = 0.0;
  }
}

__global__ void __launch_bounds__(kChunkRows) k_fire_partials(FireView st, int32_t relax_cell, const float* __restrict__ forces) {
  __shared__ double sh[4][kChunkRows];
  const int c = blockIdx.x, t = threadIdx.x;
  if (c >= st.ch.n_chunks()) return;
  const int s = st.ch.structure(c);
  if (st.flags[s] & (M3G_FIRE_CONVERGED | M3G_FIRE_ERROR)) return;   // frozen: finalize reads nothing of it
  const int64_t i = st.ch.row(c, t);
  double val[4] = {0.0, 0.0, 0.0, 0.0};   // g.v, g.g, v.v, max |g_i|^2
  if (st.ch.holds(s, i)) {
    double g[3];
    gen_force(forces, i, st.f + 9 * s, relax_cell != 0, g);
    const double* v = st.v + 3 * i;
    val[0] = g[0] * v[0] + g[1] * v[1] + g[2] * v[2];
    val[1] = g[0] * g[0] + g[1] * g[1] + g[2] * g[2];
    val[2] = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
    val[3] = val[1];
  }
  chunk_tree_reduce<4, 1>(sh, val, t);   // three sums and a maximum
  if (t < 4) st.partial[4 * c + t] = sh[t][0];
}

__global__ void __launch_bounds__(kChunkRows) k_fire_finalize(FireView st, m3g_fire_params p, int32_t check_only, const float* __restrict__ stresses,
                                                             double* __restrict__ lattice, float* __restrict__ lattice32, int32_t* host_unconverged) {
  __shared__ int cnt_sh[1][kChunkRows];
  const int t = threadIdx.x;
  int cnt = 0;
  for (int64_t s = t; s < st.ch.S; s += kChunkRows) {
    double* coef = st.coef + kCoef * s;
    int fl = st.flags[s];
    coef[0] = 0.0;
    if (fl & (M3G_FIRE_CONVERGED | M3G_FIRE_ERROR)) continue;
    double gv = 0.0, gg = 0.0, vv = 0.0, g2 = 0.0;
    for (int c = st.ch.chunks_begin(s); c < st.ch.chunks_end(s); ++c) {   // serial, in chunk order
      gv += st.partial[4 * c];
      gg += st.partial[4 * c + 1];
      vv += st.partial[4 * c + 2];
      g2 = max_nan(g2, st.partial[4 * c + 3]);
    }
    const double cf = (double)(st.ch.offsets[s + 1] - st.ch.offsets[s]);   // ASE's cell_factor: the structure's atom count
    double Fo[9], gc[9], vc[9], xc[9];
    const bool cell = p.relax_cell != 0;
    if (cell) {
      for (int k = 0; k < 9; ++k) {
        Fo[k] = st.f[9 * s + k];
        vc[k] = st.v[3 * st.N + 9 * s + k];
        xc[k] = st.x[3 * st.N + 9 * s + k];
      }
      const double* L = lattice + 9 * s;
      const double vol = fabs(L[0] * (L[4] * L[8] - L[5] * L[7]) - L[1] * (L[3] * L[8] - L[5] * L[6]) + L[2] * (L[3] * L[7] - L[4] * L[6]));
      // virial W = -dE/d eps = V * stresses (pair-virial convention), Voigt xx yy zz yz zx xy
      const float* sv = stresses + 6 * s;
      const double W[9] = {vol * sv[0], vol * sv[5], vol * sv[4], vol * sv[5], vol * sv[1], vol * sv[3], vol * sv[4], vol * sv[3], vol * sv[2]};
      // F^-1 from the adjugate
      const double det = Fo[0] * (Fo[4] * Fo[8] - Fo[5] * Fo[7]) - Fo[1] * (Fo[3] * Fo[8] - Fo[5] * Fo[6]) + Fo[2] * (Fo[3] * Fo[7] - Fo[4] * Fo[6]);
      const double Fi[9] = {(Fo[4] * Fo[8] - Fo[5] * Fo[7]) / det, (Fo[2] * Fo[7] - Fo[1] * Fo[8]) / det, (Fo[1] * Fo[5] - Fo[2] * Fo[4]) / det,
                            (Fo[5] * Fo[6] - Fo[3] * Fo[8]) / det, (Fo[0] * Fo[8] - Fo[2] * Fo[6]) / det, (Fo[2] * Fo[3] - Fo[0] * Fo[5]) / det,
                            (Fo[3] * Fo[7] - Fo[4] * Fo[6]) / det, (Fo[1] * Fo[6] - Fo[0] * Fo[7]) / det, (Fo[0] * Fo[4] - Fo[1] * Fo[3]) / det};
      // g_cell = solve(F, W^T)^T / cell_factor = W F^-T / cell_factor
      for (int r = 0; r < 3; ++r) {
        for (int k = 0; k < 3; ++k) gc[3 * r + k] = (W[3 * r] * Fi[3 * k] + W[3 * r + 1] * Fi[3 * k + 1] + W[3 * r + 2] * Fi[3 * k + 2]) / cf;
        const double* g = gc + 3 * r;
        const double* v = vc + 3 * r;
        const double rg = g[0] * g[0] + g[1] * g[1] + g[2] * g[2];
        gv += g[0] * v[0] + g[1] * v[1] + g[2] * v[2];
        gg += rg;
        vv += v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
        g2 = max_nan(g2, rg);
      }
    }
    if (!(std::isfinite(gg) && std::isfinite(g2) && std::isfinite(gv))) {   // never move a structure onto non-finite positions
      st.flags[s] = fl | M3G_FIRE_ERROR;
      continue;
    }
    if (g2 < p.fmax * p.fmax) {   // ASE: (forces**2).sum(axis=1).max() < fmax**2 -> frozen from here on
      st.flags[s] = fl | M3G_FIRE_CONVERGED;
      continue;
    }
    ++cnt;
    if (check_only) continue;
    double dt = st.dt[s], a = st.a[s], cv, cg;
    int n = st.n[s];
    if (!(fl & M3G_FIRE_STARTED)) {   // ASE's `self.v is None`: v = 0, no branch
      cv = 0.0;
      cg = dt;
    } else if (gv > 0.0) {   // v = (1-a) v + a |v| g/|g|, then v += dt g
      cv = 1.0 - a;
      const double mix = a * sqrt(vv) / sqrt(gg);
      if (n > p.nmin) {
        dt = fmin(dt * p.finc, p.dtmax);
        a *= p.fa;
      }
      n += 1;
      cg = mix + dt;
    } else {
      cv = 0.0;
      a = p.astart;
      dt *= p.fdec;
      n = 0;
      cg = dt;
    }
    // |v'|^2 = c_v^2 v.v + 2 c_v c_g g.v + c_g^2 g.g;  dr = dt v', clipped to maxstep over ALL rows of the structure
    const double vn2 = fmax(cv * cv * vv + 2.0 * cv * cg * gv + cg * cg * gg, 0.0);
    const double ndr = dt * sqrt(vn2);
    const double sdt = ndr > p.maxstep ? dt * (p.maxstep / ndr) : dt;
    st.dt[s] = dt;
    st.a[s] = a;
    st.n[s] = n;
    st.flags[s] = fl | M3G_FIRE_STARTED;
    st.steps[s] += 1;
    coef[0] = 1.0;
    coef[1] = cv;
    coef[2] = cg;
    coef[3] = sdt;
    if (cell) {
      double Fn[9];
      for (int k = 0; k < 9; ++k) {
        const double vn = cv * vc[k] + cg * gc[k];
        const double xn = xc[k] + sdt * vn;
        st.v[3 * st.N + 9 * s + k] = vn;
        st.x[3 * st.N + 9 * s + k] = xn;
        Fn[k] = xn / cf;
        coef[4 + k] = Fo[k];
        coef[13 + k] = Fn[k];
        st.f[9 * s + k] = Fn[k];
      }
      // L = L0 F'^T
      const double* L0 = st.l0 + 9 * s;
      for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k) {
          const double l = L0[3 * r] * Fn[3 * k] + L0[3 * r + 1] * Fn[3 * k + 1] + L0[3 * r + 2] * Fn[3 * k + 2];
          lattice[9 * s + 3 * r + k] = l;
          if (lattice32) lattice32[9 * s + 3 * r + k] = (float)l;
        }
    }
  }
  const int val[1] = {cnt};
  chunk_tree_reduce<1>(cnt_sh, val, t);
  if (t == 0 && host_unconverged) *host_unconverged = cnt_sh[0][0];
}

__global__ void __launch_bounds__(kChunkRows) k_fire_apply(FireView st, int32_t relax_cell, const float* __restrict__ forces, double* __restrict__ pos) {
  const int c = blockIdx.x;
  if (c >= st.ch.n_chunks()) return;
  const int s = st.ch.structure(c);
  const double* coef = st.coef + kCoef * s;
  if (coef[0] == 0.0) return;   // converged, failed or checked only: bitwise untouched
  const int64_t i = st.ch.row(c, threadIdx.x);
  if (!st.ch.holds(s, i)) return;
  const double cv = coef[1], cg = coef[2], sdt = coef[3];
  double g[3], xn[3];
  gen_force(forces, i, coef + 4, relax_cell != 0, g);
  for (int k = 0; k < 3; ++k) {
    const double vn = cv * st.v[3 * i + k] + cg * g[k];
    xn[k] = st.x[3 * i + k] + sdt * vn;
    st.v[3 * i + k] = vn;
    st.x[3 * i + k] = xn[k];
  }
  if (relax_cell) {   // pos = X F'^T
    const double* Fn = coef + 13;
    for (int k = 0; k < 3; ++k) pos[3 * i + k] = xn[0] * Fn[3 * k] + xn[1] * Fn[3 * k + 1] + xn[2] * Fn[3 * k + 2];
  } else {
    for (int k = 0; k < 3; ++k) pos[3 * i + k] = xn[k];
  }
}

bool fire_params_ok(const m3g_fire_params* p) {
  return p && finite_positive(p->dt) && finite_positive(p->maxstep) && finite_positive(p->dtmax) && finite_positive(p->finc) &&
         finite_positive(p->fdec) && finite_positive(p->fmax) && std::isfinite(p->astart) && p->astart >= 0.0 && p->astart <= 1.0 &&
         std::isfinite(p->fa) && p->fa >= 0.0 && p->fa <= 1.0 && p->nmin >= 0 && (p->relax_cell == 0 || p->relax_cell == 1);
}
}  // namespace
}  // namespace m3g

using namespace m3g;

extern "C" int m3g_fire_state_bytes(int64_t n_atoms, int64_t n_structs, size_t* bytes) {
  if (!bytes || !batch_sizes_ok(n_atoms, n_structs)) { set_error("m3g_fire_state_bytes: bad sizes"); return M3G_ERR_VALUE; }
  *bytes = fire_view(n_atoms, n_structs, nullptr).bytes;
  return M3G_OK;
}

extern "C" int m3g_fire_init(const m3g_fire_params* p, int64_t n_atoms, int64_t n_structs, const int64_t* host_offsets, const double* pos,
                             const double* lattice, void* state, size_t state_bytes, void* stream_) {
  if (!fire_params_ok(p)) { set_error("m3g_fire_init: invalid FIRE parameters (fmax, dt, maxstep, dtmax, finc, fdec > 0; astart, fa in [0, 1])"); return M3G_ERR_VALUE; }
  const int64_t N = n_atoms, S = n_structs;
  if (!init_args_ok("m3g_fire_init", N, S, host_offsets && pos && state && (lattice || !p->relax_cell))) return M3G_ERR_VALUE;
  if (!offsets_ok("m3g_fire_init", host_offsets, N, S)) return M3G_ERR_VALUE;
  const auto [st, total] = fire_view(N, S, state);
  if (!state_fits("m3g_fire_init", state_bytes, total, true)) return M3G_ERR_SIZE;
  const ChunkTable table(host_offsets, S);
  hipStream_t s = (hipStream_t)stream_;
  if (int rc = table.upload(st.ch, host_offsets, s)) return rc;
  const int64_t work = 3 * N > S ? 3 * N : S;
  hipLaunchKernelGGL(k_fire_init, grid_for(work, kChunkRows), dim3(kChunkRows), 0, s, st, pos, lattice, p->dt, p->astart);
  return launched_and_synced(s);   // (the host tables above go out of scope)
}

extern "C" int m3g_fire_step(const m3g_fire_params* p, int64_t n_atoms, int64_t n_structs, void* state, size_t state_bytes, const float* forces,
                             const float* stresses, double* pos, double* lattice, float* lattice32, int32_t check_only, int32_t* unconverged,
                             void* stream_) {
  if (!fire_params_ok(p)) { set_error("m3g_fire_step: invalid FIRE parameters (fmax, dt, maxstep, dtmax, finc, fdec > 0; astart, fa in [0, 1])"); return M3G_ERR_VALUE; }
  const int64_t N = n_atoms, S = n_structs;
  if (!batch_sizes_ok(N, S) || !state || !forces || !pos) { set_error("m3g_fire_step: null argument or bad sizes"); return M3G_ERR_VALUE; }
  if (p->relax_cell && (!stresses || !lattice)) { set_error("m3g_fire_step: a cell relaxation needs stresses and the fp64 lattice"); return M3G_ERR_VALUE; }
  const auto [st, total] = fire_view(N, S, state);
  if (!state_fits("m3g_fire_step", state_bytes, total)) return M3G_ERR_SIZE;
  hipStream_t s = (hipStream_t)stream_;
  const dim3 grid((unsigned)chunk_bound(N, S));   // workgroups beyond the table's chunk count return at once
  hipLaunchKernelGGL(k_fire_partials, grid, dim3(kChunkRows), 0, s, st, p->relax_cell, forces);
  hipLaunchKernelGGL(k_fire_finalize, dim3(1), dim3(kChunkRows), 0, s, st, *p, check_only, stresses, lattice, lattice32, unconverged);
  if (!check_only) hipLaunchKernelGGL(k_fire_apply, grid, dim3(kChunkRows), 0, s, st, p->relax_cell, forces, pos);
  M3G_RETURN_LAUNCH_STATUS();
}

extern "C" int m3g_fire_read(int64_t n_atoms, int64_t n_structs, const void* state, size_t state_bytes, int32_t* host_flags, int32_t* host_steps,
                             double* host_dt, double* host_a, int32_t* host_n, double* host_x, double* host_v, void* stream_) {
  const int64_t N = n_atoms, S = n_structs;
  if (!batch_sizes_ok(N, S) || !state) { set_error("m3g_fire_read: null argument or bad sizes"); return M3G_ERR_VALUE; }
  const auto [st, total] = fire_view(N, S, (void*)state);
  if (!state_fits("m3g_fire_read", state_bytes, total)) return M3G_ERR_SIZE;
  const int64_t R = N + 3 * S;
  return read_all((hipStream_t)stream_, {rb(host_flags, st.flags, S), rb(host_steps, st.steps, S), rb(host_dt, st.dt, S), rb(host_a, st.a, S),
                                         rb(host_n, st.n, S), rb(host_x, st.x, 3 * R), rb(host_v, st.v, 3 * R)});
}
