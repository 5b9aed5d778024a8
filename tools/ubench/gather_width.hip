// Micro-benchmark: does a 64-lane random gather of 16-byte-stride records cost the texture path less as dwordx3 than as
// dwordx4?  (gather_rate.hip answers it for a 2 KB array that lives in the L1: no.)  Here the array is the size of the
// headline box's position records — 98 304 x 16 B = 1.5 MB, resident in an XCD's 4 MB L2, far larger than the 32 KB L1 — and
// every lane draws a new record per gather (a multiplicative hash of its own state: the same VALU work at either width).
// Patterns: 64 random records per wave-gather, and runs of 8 consecutive records (what the pair kernel's lists look like:
// the lanes of an atom walk cell-sorted neighbours).
//   hipcc --offload-arch=gfx950 -O3 gather_width.hip -o gather_width
// Counters, in a run of their own:  rocprofv3 --pmc TA_BUFFER_WAVEFRONTS TA_BUFFER_TOTAL_CYCLES -- ./gather_width
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#define CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); exit(1); } } while (0)
typedef unsigned v4u __attribute__((ext_vector_type(4)));
typedef unsigned v3u __attribute__((ext_vector_type(3)));
constexpr int ITERS = 2048;
constexpr unsigned NREC = 98304;  // records of 16 bytes

template <int W, int RUN>
__global__ __launch_bounds__(256) void gather(const unsigned *data, unsigned *out) {
  const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned *>(data), 0, NREC * 16, 0x00020000);
  const unsigned lane = threadIdx.x & 63;
  // one state per run of RUN lanes: the run's first record; the lanes of a run read consecutive records
  unsigned state = (blockIdx.x * 256u + (threadIdx.x & ~(unsigned)(RUN - 1))) * 2654435761u + 12345u;
  unsigned acc = 0;
  for (int it = 0; it < ITERS; it += 4) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      state = state * 1664525u + 1013904223u;
      const unsigned rec = ((state >> 8) % (NREC - RUN)) + (lane & (RUN - 1));  // (in range by construction; the buffer checks it too)
      if (W == 3) { v3u v = __builtin_amdgcn_raw_buffer_load_b96(r, rec * 16u, 0, 0); acc += v.x ^ v.y ^ v.z; }
      if (W == 4) { v4u v = __builtin_amdgcn_raw_buffer_load_b128(r, rec * 16u, 0, 0); acc += v.x ^ v.y ^ v.z ^ v.w; }
    }
  }
  out[blockIdx.x * 256 + threadIdx.x] = acc;
}

template <int W, int RUN>
static double time_it(const unsigned *data, unsigned *out, int blocks, hipEvent_t e0, hipEvent_t e1) {
  hipLaunchKernelGGL((gather<W, RUN>), dim3(blocks), dim3(256), 0, 0, data, out);  // warm: the array into the L2s
  CHECK(hipDeviceSynchronize());
  float best = 1e30f;
  for (int rep = 0; rep < 5; ++rep) {
    CHECK(hipEventRecord(e0, 0));
    hipLaunchKernelGGL((gather<W, RUN>), dim3(blocks), dim3(256), 0, 0, data, out);
    CHECK(hipEventRecord(e1, 0));
    CHECK(hipEventSynchronize(e1));
    float ms;
    CHECK(hipEventElapsedTime(&ms, e0, e1));
    best = ms < best ? ms : best;
  }
  CHECK(hipGetLastError());
  return best;
}

int main() {
  hipDeviceProp_t prop;
  CHECK(hipGetDeviceProperties(&prop, 0));
  const int cus = prop.multiProcessorCount, blocks = cus * 5;  // 5 waves per SIMD, as the pair kernel
  unsigned *data, *out;
  CHECK(hipMalloc(&data, NREC * 16));
  CHECK(hipMemset(data, 1, NREC * 16));
  CHECK(hipMalloc(&out, (size_t)blocks * 256 * 4));
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  const double per_cu = (double)ITERS * 20;  // wave-gathers per CU (20 waves)
  const double ghz = prop.clockRate * 1e-6;  // (nominal: the cycles below are at this clock)
  printf("%d CUs, %d blocks of 4 waves, %d gathers per wave, array %u x 16 B, cycles at %.2f GHz per wave-gather per CU\n", cus, blocks,
         ITERS, NREC, ghz);
  const double r3 = time_it<3, 1>(data, out, blocks, e0, e1), r4 = time_it<4, 1>(data, out, blocks, e0, e1);
  printf("64 random records:        dwordx3 %7.1f cyc (%.3f ms)   dwordx4 %7.1f cyc (%.3f ms)   x3/x4 %.3f\n", r3 * 1e6 / per_cu * ghz, r3,
         r4 * 1e6 / per_cu * ghz, r4, r3 / r4);
  const double s3 = time_it<3, 8>(data, out, blocks, e0, e1), s4 = time_it<4, 8>(data, out, blocks, e0, e1);
  printf("8 runs of 8 consecutive:  dwordx3 %7.1f cyc (%.3f ms)   dwordx4 %7.1f cyc (%.3f ms)   x3/x4 %.3f\n", s3 * 1e6 / per_cu * ghz, s3,
         s4 * 1e6 / per_cu * ghz, s4, s3 / s4);
  return 0;
}
