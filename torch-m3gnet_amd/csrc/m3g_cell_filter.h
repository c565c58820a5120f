// The cell filter of the batched optimisers (m3g_relax.hip: FIRE, m3g_lbfgs.hip: L-BFGS), ASE's UnitCellFilter with a linear
// deformation gradient F (row-major [9], identity at the start) and cell_factor cf = the structure's atom count:
//   X = [pos F^-T ; cf F],   g = [f F ; W F^-T / cf]  with the virial W = V * stresses,   after a step F' = X_cell / cf,
//   lattice = L0 F'^T,  pos = X_atoms F'^T.
// Inline device functions, so each kernel that calls them compiles them under its own floating-point contraction mode.
// m3g_relax.hip keeps its own text of this algebra, the one these functions were lifted from: calling them from k_fire_finalize and
// k_fire_apply changed those kernels' generated code (registers, branch layout and the order of the fp64 multiplies, compared as
// gfx950 assembly), and FIRE's arithmetic is pinned bitwise by its tests and by every driver built on it.  A new optimiser calls these.
#pragma once
#include <cmath>
#include <cstdint>

namespace m3g {
// g = f F (row vector times the deformation gradient), or f itself with the cell fixed
__device__ inline void gen_force(const float* __restrict__ forces, int64_t i, const double* F, bool cell, double g[3]) {
  const double f0 = forces[3 * i], f1 = forces[3 * i + 1], f2 = forces[3 * i + 2];
  if (cell) {
    for (int k = 0; k < 3; ++k) g[k] = f0 * F[k] + f1 * F[3 + k] + f2 * F[6 + k];
  } else {
    g[0] = f0; g[1] = f1; g[2] = f2;
  }
}

// the three cell rows of g: solve(F, W^T)^T / cf = W F^-T / cf, W = |det L| * stresses (f32 Voigt xx yy zz yz zx xy, pair-virial
// convention: W = -dE/d eps) at the current lattice L (rows = lattice vectors)
__device__ inline void cell_gen_force(const double* Fo, const double* L, const float* sv, double cf, double gc[9]) {
  const double vol = fabs(L[0] * (L[4] * L[8] - L[5] * L[7]) - L[1] * (L[3] * L[8] - L[5] * L[6]) + L[2] * (L[3] * L[7] - L[4] * L[6]));
  const double W[9] = {vol * sv[0], vol * sv[5], vol * sv[4], vol * sv[5], vol * sv[1], vol * sv[3], vol * sv[4], vol * sv[3], vol * sv[2]};
  // F^-1 from the adjugate
  const double det = Fo[0] * (Fo[4] * Fo[8] - Fo[5] * Fo[7]) - Fo[1] * (Fo[3] * Fo[8] - Fo[5] * Fo[6]) + Fo[2] * (Fo[3] * Fo[7] - Fo[4] * Fo[6]);
  const double Fi[9] = {(Fo[4] * Fo[8] - Fo[5] * Fo[7]) / det, (Fo[2] * Fo[7] - Fo[1] * Fo[8]) / det, (Fo[1] * Fo[5] - Fo[2] * Fo[4]) / det,
                        (Fo[5] * Fo[6] - Fo[3] * Fo[8]) / det, (Fo[0] * Fo[8] - Fo[2] * Fo[6]) / det, (Fo[2] * Fo[3] - Fo[0] * Fo[5]) / det,
                        (Fo[3] * Fo[7] - Fo[4] * Fo[6]) / det, (Fo[1] * Fo[6] - Fo[0] * Fo[7]) / det, (Fo[0] * Fo[4] - Fo[1] * Fo[3]) / det};
  for (int r = 0; r < 3; ++r)
    for (int k = 0; k < 3; ++k) gc[3 * r + k] = (W[3 * r] * Fi[3 * k] + W[3 * r + 1] * Fi[3 * k + 1] + W[3 * r + 2] * Fi[3 * k + 2]) / cf;
}

// lattice = L0 F'^T, to the caller's fp64 cell and (when given) its fp32 copy
__device__ inline void deformed_lattice(const double* L0, const double* Fn, double* lattice, float* lattice32) {
  for (int r = 0; r < 3; ++r)
    for (int k = 0; k < 3; ++k) {
      const double l = L0[3 * r] * Fn[3 * k] + L0[3 * r + 1] * Fn[3 * k + 1] + L0[3 * r + 2] * Fn[3 * k + 2];
      lattice[3 * r + k] = l;
      if (lattice32) lattice32[3 * r + k] = (float)l;
    }
}

// pos = x F'^T, or x itself with the cell fixed
__device__ inline void deformed_pos(const double xn[3], const double* Fn, bool cell, double* pos) {
  if (cell) {
    for (int k = 0; k < 3; ++k) pos[k] = xn[0] * Fn[3 * k] + xn[1] * Fn[3 * k + 1] + xn[2] * Fn[3 * k + 2];
  } else {
    for (int k = 0; k < 3; ++k) pos[k] = xn[k];
  }
}
}  // namespace m3g
