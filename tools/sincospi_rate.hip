// Rate of the fp64 sincospi the scattering sampler calls (csrc/m3g_scattering.hip, k_sq_density), for profiles/scattering.txt.
//   hipcc -O3 --offload-arch=gfx950 tools/sincospi_rate.hip -o tools/bin/sincospi_rate
//   tools/bin/sincospi_rate WORKGROUPS THREADS EVALUATIONS_PER_THREAD
// Every thread evaluates sincospi of EVALUATIONS_PER_THREAD different reduced arguments in [-1, 1], one after the other as the sampler's
// row loop does, and adds the results up (one store per thread keeps the loop alive).  Prints the device time of the best of five
// launches after a warm-up and the evaluations per second.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

#define CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { std::printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)

__global__ void k_rate(double* out, int n, double step) {
  const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  double p = 1e-3 * (double)(gid % 977), re = 0.0, im = 0.0;
  for (int j = 0; j < n; ++j) {
    p += step;
    p -= rint(p);   // in [-1/2, 1/2], as the sampler's phase
    double sn, cs;
    sincospi(2.0 * p, &sn, &cs);
    re += cs;
    im -= sn;
  }
  out[gid] = re + im;
}

int main(int argc, char** argv) {
  if (argc != 4) { std::printf("usage: %s WORKGROUPS THREADS EVALUATIONS_PER_THREAD\n", argv[0]); return 2; }
  const int groups = std::atoi(argv[1]), threads = std::atoi(argv[2]), n = std::atoi(argv[3]);
  if (groups < 1 || groups > (1 << 20) || threads < 1 || threads > 1024 || n < 1) { std::printf("bad arguments\n"); return 2; }
  double* out = nullptr;
  CHECK(hipMalloc(&out, sizeof(double) * (size_t)groups * threads));
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  float best = 1e30f;
  for (int rep = 0; rep < 6; ++rep) {   // the first launch warms up
    CHECK(hipEventRecord(e0, nullptr));
    hipLaunchKernelGGL(k_rate, dim3(groups), dim3(threads), 0, nullptr, out, n, 0.0137);
    CHECK(hipEventRecord(e1, nullptr));
    CHECK(hipEventSynchronize(e1));
    CHECK(hipGetLastError());
    float ms = 0.f;
    CHECK(hipEventElapsedTime(&ms, e0, e1));
    if (rep > 0 && ms < best) best = ms;
  }
  const double evals = (double)groups * threads * n;
  std::printf("{\"workgroups\": %d, \"threads\": %d, \"per_thread\": %d, \"best_ms\": %.5f, \"evaluations_per_s\": %.4e}\n", groups, threads, n,
              best, evals / (best * 1e-3));
  CHECK(hipFree(out));
  return 0;
}
