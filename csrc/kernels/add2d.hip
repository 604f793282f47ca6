// u[y][x] += g[y][x] over an nx x ny region (fp64), hand-written for gfx950.
//
// The streaming add that ends a Poisson block of the Jacobi engine
// (gmt/jacobi.hpp JacobiConfig::source): u(t+n) = L^n(u(t)) + g_n, the fused
// Laplace passes followed by one add of the fixed block field g_n.
//
// HBM-bound like DAXPY: 24 B per point (g read, u read, u written), every
// byte touched once, so the same shape as daxpy_stream (daxpy.hip): 128-thread
// blocks, ONE 16-B chunk of g and u per lane, nontemporal loads AND stores.
// A block covers 256 contiguous columns (2 KiB) of one row, as a DAXPY block
// covers 2 KiB of its vector; its row and segment come from one 32-bit scalar
// division of the block index, no per-lane division.
// add2d_scalar: one element per lane, for odd alignment or odd pitches.
// One IEEE addition per cell on both paths: bitwise u + g.
#include "common.hpp"
#include "gmt/kernels.h"

namespace gmt {

template <int B>
__global__ __launch_bounds__(B) void add2d_pt(int64_t nx, int64_t ny, const double* __restrict__ g, int64_t ldg,
                                              double* __restrict__ u, int64_t ld, unsigned nbx) {
  const unsigned bx = blockIdx.x % nbx, by = blockIdx.x / nbx;  // 32-bit: fewer than 2^31 blocks
  const int64_t xr = (static_cast<int64_t>(bx) * B + threadIdx.x) * 2;
  const int64_t yr = by;
  if (xr >= nx) return;
  const double* pg = g + yr * ldg + xr;
  double* pu = u + yr * ld + xr;
  if (xr + 1 < nx)
    st2_nt(pu, ld2_nt(pu) + ld2_nt(pg));
  else  // odd last column of the region
    pu[0] += pg[0];
}

__global__ __launch_bounds__(kBlock) void add2d_scalar(int64_t nx, int64_t ny, const double* __restrict__ g,
                                                       int64_t ldg, double* __restrict__ u, int64_t ld,
                                                       unsigned nbx) {
  const unsigned bx = blockIdx.x % nbx, by = blockIdx.x / nbx;
  const int64_t xr = static_cast<int64_t>(bx) * kBlock + threadIdx.x;
  const int64_t yr = by;
  if (xr >= nx) return;
  u[yr * ld + xr] += g[yr * ldg + xr];
}

// The one dispatch decision of gmt_add2d (and the answer of gmt_add2d_path)
static int add2d_path(const double* g, int64_t ldg, const double* u, int64_t ld) {
  return aligned16(g) && aligned16(u) && ldg % 2 == 0 && ld % 2 == 0 ? GMT_PATH_PT : GMT_PATH_SCALAR;
}

}  // namespace gmt

extern "C" int gmt_add2d_path(int64_t, const double* g, int64_t ldg, const double* u, int64_t ld) {
  return gmt::add2d_path(g, ldg, u, ld);
}

extern "C" int gmt_add2d(int64_t nx, int64_t ny, const double* g, int64_t ldg, double* u, int64_t ld,
                         void* stream) {
  using namespace gmt;
  if (nx < 0 || ny < 0) return static_cast<int>(hipErrorInvalidValue);
  if (nx == 0 || ny == 0) return 0;
  if (!g || !u || ldg < nx || ld < nx) return static_cast<int>(hipErrorInvalidValue);
  hipStream_t s = static_cast<hipStream_t>(stream);
  constexpr int B = 128;
  const bool pt = add2d_path(g, ldg, u, ld) == GMT_PATH_PT;
  const int64_t cols = pt ? 2 * B : kBlock;  // a block: one row segment
  const int64_t nbx = (nx + cols - 1) / cols, nb = nbx * ny;
  if (nb > INT32_MAX) return static_cast<int>(hipErrorInvalidValue);  // the grid's x extent
  if (pt)
    add2d_pt<B><<<grid_1d(nb), B, 0, s>>>(nx, ny, g, ldg, u, ld, static_cast<unsigned>(nbx));
  else
    add2d_scalar<<<grid_1d(nb), kBlock, 0, s>>>(nx, ny, g, ldg, u, ld, static_cast<unsigned>(nbx));
  GMT_RET_LAUNCH();
}
