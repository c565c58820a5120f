// The Nose-Hoover chain half-step the deterministic MD families share: m3g_nhc.hip (chain NVT, isotropic MTK NPT) and m3g_mtk.hip
// (flexible-cell MTK NPT) drive their particle and barostat chains with it, one lane per structure.
#pragma once
#include <cmath>
#include <cstdint>

#include "m3gnet_hip.h"

namespace m3g {
constexpr int kMaxChain = M3G_NHC_MAX_CHAIN;
inline bool chain_ok(int32_t M) { return M >= 1 && M <= kMaxChain; }

// The chain half-step of length h in n_c equal parts (MTK 1996) on a chain of M thermostats of masses q0, qk, qk, ... driven by k2,
// twice the kinetic energy it thermostats, against gkt: returns the scale of the thermostatted velocities; k2 leaves scaled.
__device__ inline double chain_half_step(double q0, double qk, double* xi, double* vxi, int M, int n_c, double& k2, double gkt, double kt,
                                         double h) {
  const double d = h / n_c;
  double scale = 1.0;
  auto force = [&](int k) {
    if (k == 0) return (k2 - gkt) / q0;
    return ((k == 1 ? q0 : qk) * vxi[k - 1] * vxi[k - 1] - kt) / qk;
  };
  for (int part = 0; part < n_c; ++part) {
    vxi[M - 1] += 0.5 * d * force(M - 1);
    for (int k = M - 2; k >= 0; --k) {
      const double e = exp(-0.25 * d * vxi[k + 1]);
      vxi[k] = (vxi[k] * e + 0.5 * d * force(k)) * e;
    }
    const double s = exp(-d * vxi[0]);
    scale *= s;
    k2 = s * s * k2;
    for (int k = 0; k < M; ++k) xi[k] += d * vxi[k];
    for (int k = 0; k < M - 1; ++k) {
      const double e = exp(-0.25 * d * vxi[k + 1]);
      vxi[k] = (vxi[k] * e + 0.5 * d * force(k)) * e;
    }
    vxi[M - 1] += 0.5 * d * force(M - 1);
  }
  return scale;
}
}  // namespace m3g
