// The basis functions of the model as device functions, one copy each for the MFMA-tile kernels (compile-time orders, caps
// kLCap / kRCap; STATIC = true: the recurrences unroll) and the any-size path (run-time orders, the reference's table caps; STATIC =
// false: they loop).  The order of fp32 operations in every body is the reference's; parity rests on it.
// Reference: nn/featurizer.py:81-100 (radial basis), nn/interaction.py:268-281 (spherical Bessel), :353-382 (Legendre and its
// backward), :389-400 (three-body cutoff envelope).
#pragma once
#include <hip/hip_runtime.h>

namespace m3g {

// torch.sinc: sin(pi x)/(pi x), and cos(pi x) from the same argument reduction
__device__ __forceinline__ float sinc_cos_pi(float x, float& cos_px) {
  const float kPi = 3.14159265358979323846f;
  float px = kPi * x, sn;
  sincosf(px, &sn, &cos_px);
  return x == 0.f ? 1.f : sn / px;
}

// one term of the radial basis: h_m(d) and dh_m/dd from h_{m-1}, dh_{m-1}/dd, which arrive in f / df (unread for m = 0).
// C: Consts or the any-size path's GenConsts (a1, a2, coeff, rec_mul, rec_div), by value: through a reference the any-size kernel
// copies its by-value kernel argument first
template <class C>
__device__ __forceinline__ void radial_term(const C c, int m, float d, float& f, float& df) {
  float c1, c2;
  const float s1 = sinc_cos_pi(c.a1[m] * d, c1), s2 = sinc_cos_pi(c.a2[m] * d, c2);
  float t = c.coeff[m] * (s1 + s2);
  float dt = c.coeff[m] * ((c1 - s1) + (c2 - s2)) / d;
  if (m > 0) {
    t = (t + c.rec_mul[m] * f) / c.rec_div[m];
    dt = (dt + c.rec_mul[m] * df) / c.rec_div[m];
  }
  f = t;
  df = dt;
}

// three-body cutoff envelope fc(d) and its derivative; zero beyond rc3
struct Envelope { float f, fp; };
__device__ __forceinline__ Envelope envelope(float d, float rc3) {
  const float rho = d / rc3;
  Envelope v{0.f, 0.f};
  if (rho <= 1.f) {
    const float r2 = rho * rho, r3 = r2 * rho;
    v.f = 1.f - 6.f * r3 * r2 + 15.f * r2 * r2 - 10.f * r3;
    v.fp = (-30.f * r2 * r2 + 60.f * r3 - 30.f * r2) / rc3;
  }
  return v;
}

// for (i = begin; i < end; ++i) body(i).  STATIC: the bounds are constants at the call and the loop unrolls (the MFMA-tile kernels'
// compile-time orders); otherwise a plain run-time loop (the any-size path)
template <bool STATIC, class F>
__device__ __forceinline__ void orders(int begin, int end, F body) {
  if constexpr (STATIC) {
#pragma unroll
    for (int i = begin; i < end; ++i) body(i);
  } else {
    for (int i = begin; i < end; ++i) body(i);
  }
}

// j_l(x), j_l'(x) for l = 0..L-1 (L <= CAP), upward recurrence with the reference's x <= 1e-8 branch
template <int CAP, bool STATIC>
__device__ __forceinline__ void sph_bessel(int L, float x, float* j, float* dj) {
  float seq[CAP + 1];
  if (x > 1e-8f) {
    float sn, cx;
    sincosf(x, &sn, &cx);
    const float sx = sn / x;
    seq[0] = sx;
    seq[1] = (sx - cx) / x;
    orders<STATIC>(1, L, [&](int n) { seq[n + 1] = (float)(2 * n + 1) / x * seq[n] - seq[n - 1]; });
    orders<STATIC>(0, L, [&](int l) {
      j[l] = seq[l];
      dj[l] = l == 0 ? -seq[1] : seq[l - 1] - (float)(l + 1) / x * seq[l];
    });
  } else {
    float dfact = 1.f;
    orders<STATIC>(0, L, [&](int l) {
      if (l > 0) dfact *= (float)(2 * l + 1);
      j[l] = l == 0 ? 1.f : x / dfact;
      dj[l] = l == 1 ? 1.f / 3.f : 0.f;
    });
  }
}

// P_l(x), P_l'(x) for l = 0..L-1
template <bool STATIC>
__device__ __forceinline__ void legendre(int L, float x, float* P, float* dP) {
  P[0] = 1.f; dP[0] = 0.f;
  if (L > 1) { P[1] = x; dP[1] = 1.f; }
  orders<STATIC>(1, L - 1, [&](int n) {
    P[n + 1] = ((float)(2 * n + 1) * x * P[n] - (float)n * P[n - 1]) / (float)(n + 1);
    dP[n + 1] = ((float)(2 * n + 1) * (P[n] + x * dP[n]) - (float)n * dP[n - 1]) / (float)(n + 1);
  });
}

// LegendreCosPolynomial.backward (nn/interaction.py:373-382) multiplies grad_output in at EVERY level of its recurrence,
//   grad_n = (n P_{n-1} + x grad_{n-1}) go   =>   grad_n = go k_n,  k_1 = 1,  k_n = n P_{n-1} + x go k_{n-1},
// which is the derivative P_n' go only for n <= 1 (SURVEY finding 2).  The engine computes the true derivative; with the option
// "legendre_backward" set, the list kernels return this k_n instead of P_n' so that forces and stresses reproduce the reference's
// own numbers.  `go` is the gradient arriving at legendre_cos(cos, l)'s output for ONE triplet and ONE l (the reference calls it
// once per l).  STATIC: the loop runs to the constant l_max = L, the levels above l masked; otherwise to l (L is not read).
template <bool STATIC>
__device__ __forceinline__ float legendre_ref_k(int L, int l, float x, const float* P, float go) {
  if (l == 0) return 0.f;
  float k = 1.f;
  orders<STATIC>(2, STATIC ? L : l + 1, [&](int n) {
    if (!STATIC || n <= l) k = (float)n * P[n - 1] + x * go * k;
  });
  return k;
}

}  // namespace m3g
