// Deterministic reduction of per-block partials, shared by the Jacobi sweep
// (jacobi5.hip) and the read-only residual (jacobi5_resid.hip): level 1
// reduces contiguous chunks with up to kL2 blocks, level 2 (one block)
// reduces those.  The order depends only on n, so results are run-to-run
// identical.  OP: 0 = sum, 1 = max.
#pragma once
#include "common.hpp"

namespace gmt {

constexpr int64_t kL2 = 1024;

template <int OP>
__device__ __forceinline__ double partial_op(double a, double b) {
  return OP == 0 ? a + b : fmax(a, b);
}
template <int OP>
__device__ __forceinline__ double block_op(double v) {
  return OP == 0 ? block_sum(v) : block_max(v);
}

template <int OP>
__global__ __launch_bounds__(kBlock) void reduce_chunks(const double* __restrict__ partial, int64_t n,
                                                        int64_t chunk, double* __restrict__ out) {
  const int64_t lo = blockIdx.x * chunk, hi = (lo + chunk) < n ? (lo + chunk) : n;
  double acc = 0.0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += kBlock) acc = partial_op<OP>(acc, partial[i]);
  acc = block_op<OP>(acc);
  if (threadIdx.x == 0) out[blockIdx.x] = acc;
}

template <int OP>
__global__ __launch_bounds__(kBlock) void reduce_all(const double* __restrict__ partial, int64_t n,
                                                     double* __restrict__ out) {
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += kBlock) acc = partial_op<OP>(acc, partial[i]);
  acc = block_op<OP>(acc);
  if (threadIdx.x == 0) out[0] = acc;
}

// partial[0, nb) -> out[0]; partial[nb, nb + kL2) is the level-2 scratch.
// (The max form starts from 0: its inputs are magnitudes.)
template <int OP>
static void reduce_partials(const double* partial, int64_t nb, double* out, hipStream_t s) {
  if (nb <= 4 * kBlock) {
    reduce_all<OP><<<1, kBlock, 0, s>>>(partial, nb, out);
    return;
  }
  const int64_t nb2 = nb < kL2 ? nb : kL2;
  const int64_t chunk = (nb + nb2 - 1) / nb2;
  const int64_t used = (nb + chunk - 1) / chunk;
  double* l2 = const_cast<double*>(partial) + nb;
  reduce_chunks<OP><<<grid_1d(used), kBlock, 0, s>>>(partial, nb, chunk, l2);
  reduce_all<OP><<<1, kBlock, 0, s>>>(l2, used, out);
}

// the block partials of write_block_partials (row_walk.hpp) -> out[0] = sum, out[1] = max
static void reduce_sum_max(const double* psum, const double* pmax, int64_t nb, double* out, hipStream_t s) {
  reduce_partials<0>(psum, nb, out, s);
  reduce_partials<1>(pmax, nb, out + 1, s);
}

}  // namespace gmt
