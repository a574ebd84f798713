// probe: v_mfma_f64_16x16x4_f64 -- (1) its operand and result lane maps, checked with asymmetric integer data against a host product; (2) the
// sustained rate at one wave per SIMD (one 256-thread workgroup per CU, 100 KB of LDS asked for so no second one fits) with NACC independent
// accumulators per wave, and at two waves per SIMD (512 threads), timed by events.  Prints one JSON line.
// build: hipcc --offload-arch=gfx950 -O3 -o probe_f64_mfma tools/probes/probe_f64_mfma.hip
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
typedef double d4 __attribute__((ext_vector_type(4)));
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)

// C = A B, A 16 x 4 and B 4 x 16 row-major: lane l loads A[l & 15][l >> 4] and B[l >> 4][l & 15], writes C[(l >> 4) + 4 q][l & 15]
__global__ void k_map(const double* A, const double* B, double* Cm)
{
  const int l = threadIdx.x;
  d4 c = {0.0, 0.0, 0.0, 0.0};
  c = __builtin_amdgcn_mfma_f64_16x16x4f64(A[(l & 15) * 4 + (l >> 4)], B[(l >> 4) * 16 + (l & 15)], c, 0, 0, 0);
  for (int q = 0; q < 4; q++) Cm[((l >> 4) + 4 * q) * 16 + (l & 15)] = c[q];
}

template <int NACC>
__global__ __launch_bounds__(512, 1) void k_rate(double* out, int iters, double seed)
{
  extern __shared__ double lds[];
  d4 acc[NACC];
  for (int t = 0; t < NACC; t++) acc[t] = (d4){0.0, 0.0, 0.0, 0.0};
  const double a = seed + threadIdx.x, b = seed * 0.5;
  for (int it = 0; it < iters; it++)
#pragma unroll
    for (int t = 0; t < NACC; t++) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[t], 0, 0, 0);
  double s = 0.0;
  for (int t = 0; t < NACC; t++) s += acc[t][0] + acc[t][1] + acc[t][2] + acc[t][3];
  if (s == 123.456) out[threadIdx.x] = s + lds[threadIdx.x];
}

template <int NACC>
static double rate(int cus, double* dout, int threads = 256)
{
  const int iters = 20000;
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  hipLaunchKernelGGL(k_rate<NACC>, dim3(cus), dim3(threads), 100 * 1024, 0, dout, 100, 1.0);
  CK(hipDeviceSynchronize());
  CK(hipEventRecord(e0));
  hipLaunchKernelGGL(k_rate<NACC>, dim3(cus), dim3(threads), 100 * 1024, 0, dout, iters, 1.0);
  CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
  float ms = 0.f; CK(hipEventElapsedTime(&ms, e0, e1));
  const double flop = (double) cus * (threads / 64) * iters * NACC * 16.0 * 16.0 * 4.0 * 2.0;
  return flop / (ms * 1e-3) / 1e12;
}

int main()
{
  hipDeviceProp_t p; CK(hipGetDeviceProperties(&p, 0));
  double hA[64], hB[64], hC[256], ref[256];
  for (int i = 0; i < 16; i++) for (int k = 0; k < 4; k++) hA[i * 4 + k] = 3 * i + 17 * k + 1;
  for (int k = 0; k < 4; k++) for (int j = 0; j < 16; j++) hB[k * 16 + j] = 100 * k - 7 * j + 5;
  for (int i = 0; i < 16; i++) for (int j = 0; j < 16; j++) { double s = 0; for (int k = 0; k < 4; k++) s += hA[i * 4 + k] * hB[k * 16 + j]; ref[i * 16 + j] = s; }
  double *dA, *dB, *dC, *dout;
  CK(hipMalloc(&dA, sizeof hA)); CK(hipMalloc(&dB, sizeof hB)); CK(hipMalloc(&dC, sizeof hC)); CK(hipMalloc(&dout, 256 * sizeof(double)));
  CK(hipMemcpy(dA, hA, sizeof hA, hipMemcpyHostToDevice)); CK(hipMemcpy(dB, hB, sizeof hB, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_map, dim3(1), dim3(64), 0, 0, dA, dB, dC);
  CK(hipMemcpy(hC, dC, sizeof hC, hipMemcpyDeviceToHost));
  int bad = 0; for (int i = 0; i < 256; i++) bad += hC[i] != ref[i];
  CK(hipFuncSetAttribute((const void*) k_rate<1>, hipFuncAttributeMaxDynamicSharedMemorySize, 100 * 1024));
  CK(hipFuncSetAttribute((const void*) k_rate<4>, hipFuncAttributeMaxDynamicSharedMemorySize, 100 * 1024));
  CK(hipFuncSetAttribute((const void*) k_rate<8>, hipFuncAttributeMaxDynamicSharedMemorySize, 100 * 1024));
  const int cus = p.multiProcessorCount;
  const double r1 = rate<1>(cus, dout), r4 = rate<4>(cus, dout), r8 = rate<8>(cus, dout), r8w2 = rate<8>(cus, dout, 512);
  printf("{\"probe\": \"f64_mfma_16x16x4\", \"lane_map_mismatches\": %d, \"cus\": %d, \"clock_mhz\": %d, \"tflops_1acc\": %.2f, \"tflops_4acc\": %.2f, \"tflops_8acc\": %.2f, "
         "\"tflops_8acc_2waves_per_simd\": %.2f}\n", bad, cus, p.clockRate / 1000, r1, r4, r8, r8w2);
  return bad ? 1 : 0;
}
