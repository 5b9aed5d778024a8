// The fixed-order sum (DESIGN, "The fixed-order sum"): how every kernel that reports a per-replica number without
// floating-point atomics adds it up, so that two runs give the same bits.  Device only.
//   block stage  every lane accumulates in double; the 64-lane xor butterfly; the four wave results of a block meet in LDS; the
//                block's K results are stored to one row of a workspace, rows[replica][row][K]            (block_sums, block_sum)
//   fold stage   ONE WAVE takes the rows: lane l takes rows l, l + 64, ... into an accumulator that starts at 0.0; the butterfly;
//                every lane holds the K results                                                                     (fold_rows)
// Additions (or fmax) only: contraction cannot change them.  tests/_reduce.py is the same arithmetic in numpy.
#pragma once

#include <hip/hip_runtime.h>

namespace tmd {

// wave-wide sum / maximum (64 lanes, xor butterfly), result valid in every lane
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// what is folded: a sum, or a maximum of values >= 0 (an accumulator starts at 0.0 either way)
struct Sum {
  static __device__ __forceinline__ double wave(double v) { return wave_sum(v); }
  static __device__ __forceinline__ double two(double a, double b) { return a + b; }
};
struct Max {
  static __device__ __forceinline__ double wave(double v) { return wave_max(v); }
  static __device__ __forceinline__ double two(double a, double b) { return fmax(a, b); }
};

// The order in which the four wave results p0 .. p3 of a block meet: p0 + p1 + p2 + p3, or (p0 + p1) + (p2 + p3).  Both are
// fixed; they give different bits from each other, and a site that changed its order would change the bits of every trajectory
// behind it.  A NEW SITE TAKES Pairwise.  Sequential is what thermostat.hip, exchange.hip, fire.hip, integrator.hip and
// pme.hip have had from their start (tests/test_gpu_*.py::test_partial_rows_* pin it).
enum class Meet { Sequential, Pairwise };

// The meet of a block of four waves: s[k] is the calling wave's result of column k (the same in its 64 lanes); thread k < K
// returns the block's result of column k, every other thread 0.0.  The LDS belongs to the instance: a second call with the
// same template arguments in one kernel needs a __syncthreads() in between.
template <Meet ORDER, int K, typename Op>
__device__ __forceinline__ double meet_in_lds(const double (&s)[K]) {
  __shared__ double part[4][K];
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) part[threadIdx.x >> 6][k] = s[k];
  }
  __syncthreads();
  if (threadIdx.x >= K) return 0.0;
  const double p0 = part[0][threadIdx.x], p1 = part[1][threadIdx.x], p2 = part[2][threadIdx.x], p3 = part[3][threadIdx.x];
  // (no start from 0.0: a sum of -0.0 keeps its sign)
  return ORDER == Meet::Sequential ? Op::two(Op::two(Op::two(p0, p1), p2), p3) : Op::two(Op::two(p0, p1), Op::two(p2, p3));
}

// Block stage: v[k] is the lane's value of column k; dst[0 .. K) receive the results of the block of WAVES waves (1: no meet
// and no LDS; 4: see meet_in_lds).  Every thread of the block must arrive.
template <int WAVES, Meet ORDER, int K, typename Op = Sum>
__device__ __forceinline__ void block_sums(const double (&v)[K], double *__restrict__ dst) {
  static_assert(WAVES == 1 || WAVES == 4, "one wave, or four that meet");
  double s[K];
#pragma unroll
  for (int k = 0; k < K; ++k) s[k] = Op::wave(v[k]);
  if (WAVES == 1) {
    if (threadIdx.x == 0) {
#pragma unroll
      for (int k = 0; k < K; ++k) dst[k] = s[k];
    }
  } else {
    const double r = meet_in_lds<ORDER, K, Op>(s);
    if (threadIdx.x < K) dst[threadIdx.x] = r;
  }
}

// the same for one column of a block of four waves, handed back: thread 0 returns the block's sum
template <Meet ORDER>
__device__ __forceinline__ double block_sum(double v) {
  const double s[1] = {wave_sum(v)};
  return meet_in_lds<ORDER, 1, Sum>(s);
}

// Fold stage, run by one wave: acc[k] takes rows[b * STRIDE + k] for b = lane, lane + 64, ... < nrows, in that order.  A caller
// with several row sets (or one accumulator that continues over several) calls this once per set and butterflies (wave_sum)
// at the end: all loops first, then all butterflies, is what the hand-written folds did, and costs fewer registers.
template <int K, int STRIDE = K, typename Op = Sum>
__device__ __forceinline__ void fold_into(double (&acc)[K], const double *__restrict__ rows, int nrows) {
  for (int b = threadIdx.x & 63; b < nrows; b += 64) {
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = Op::two(acc[k], rows[(size_t)b * STRIDE + k]);
  }
}

// two column sets of the same rows in one pass (a serial wave pays every row's load latency once per pass)
template <int STRIDE, typename OpA, typename OpB, int KA, int KB>
__device__ __forceinline__ void fold_into(double (&a)[KA], const double *__restrict__ rows_a, double (&b)[KB],
                                          const double *__restrict__ rows_b, int nrows) {
  for (int r = threadIdx.x & 63; r < nrows; r += 64) {
#pragma unroll
    for (int k = 0; k < KA; ++k) a[k] = OpA::two(a[k], rows_a[(size_t)r * STRIDE + k]);
#pragma unroll
    for (int k = 0; k < KB; ++k) b[k] = OpB::two(b[k], rows_b[(size_t)r * STRIDE + k]);
  }
}

// the whole fold of one row set: from 0.0, fold_into, the butterfly; every lane holds out[0 .. K)
template <int K, int STRIDE = K, typename Op = Sum>
__device__ __forceinline__ void fold_rows(const double *__restrict__ rows, int nrows, double (&out)[K]) {
#pragma unroll
  for (int k = 0; k < K; ++k) out[k] = 0.0;
  fold_into<K, STRIDE, Op>(out, rows, nrows);
#pragma unroll
  for (int k = 0; k < K; ++k) out[k] = Op::wave(out[k]);
}

}  // namespace tmd
