// The float64 vector rate of the device, for tools/bootstrap_bench.py (which
// loads this as a shared library and calls it in its own process):
//
//   hipcc --offload-arch=gfx950 -O3 -shared -fPIC -o build/libf64_rate.so \
//       tools/f64_rate.hip
//
// As in tools/valu_rate.hip every wave runs `reps` x 16 independent
// instructions of one form (16 accumulator chains, so dependent-issue latency
// does not enter) and nothing touches memory; one workgroup of `threads`
// threads per CU.  Form 0 is v_fma_f64, form 1 the pair K23 runs for float64
// input, v_mul_f64 then v_add_f64 (counted as ONE operation: one term).
// f64_rate returns 0 and the operations per second over all lanes of the
// device (the median of 5 timed launches), or a HIP error code.
#include <hip/hip_runtime.h>

#include <algorithm>

#define REPEAT16(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15)

template <int FORM>
__global__ void __launch_bounds__(1024) rate_kernel(double* out, int reps,
                                                    double seed) {
  double d[16], t[16], e = seed * 0.5, f = seed + 0.25;
#pragma unroll
  for (int i = 0; i < 16; ++i) d[i] = seed + i;
  for (int r = 0; r < reps; ++r) {
    if constexpr (FORM == 0) {
#define X(i) asm volatile("v_fma_f64 %0, %1, %2, %0" : "+v"(d[i]) : "v"(e), "v"(f));
      REPEAT16(X)
#undef X
    } else {
#define X(i) asm volatile("v_mul_f64 %0, %1, %2" : "=v"(t[i]) : "v"(e), "v"(f));
      REPEAT16(X)
#undef X
#define X(i) asm volatile("v_add_f64 %0, %0, %1" : "+v"(d[i]) : "v"(t[i]));
      REPEAT16(X)
#undef X
    }
  }
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < 16; ++i) s += d[i];
  if (s == 1.2345) out[threadIdx.x] = s;
}

extern "C" int f64_rate(int form, int threads, int reps,
                        double* ops_per_second) {
  if (!ops_per_second || threads < 64 || threads > 1024 || threads % 64 ||
      reps < 1 || form < 0 || form > 1)
    return -1;
  double* out = nullptr;
  hipError_t err = hipMalloc(&out, 1024 * sizeof(double));
  if (err != hipSuccess) return (int)err;
  int cus = 256;
  hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0);
  hipEvent_t e0, e1;
  hipEventCreate(&e0);
  hipEventCreate(&e1);
  auto launch = [&]() {
    if (form == 0)
      hipLaunchKernelGGL(rate_kernel<0>, dim3(cus), dim3(threads), 0, 0, out,
                         reps, 1.0);
    else
      hipLaunchKernelGGL(rate_kernel<1>, dim3(cus), dim3(threads), 0, 0, out,
                         reps, 1.0);
  };
  launch();
  launch();
  float ms[5];
  for (int i = 0; i < 5; ++i) {
    hipEventRecord(e0, 0);
    launch();
    hipEventRecord(e1, 0);
    hipEventSynchronize(e1);
    hipEventElapsedTime(&ms[i], e0, e1);
  }
  err = hipGetLastError();
  hipEventDestroy(e0);
  hipEventDestroy(e1);
  hipFree(out);
  if (err != hipSuccess) return (int)err;
  std::sort(ms, ms + 5);
  const double ops = (double)cus * threads * (double)reps * 16.0;
  *ops_per_second = ops / (ms[2] * 1e-3);
  return 0;
}
