// Read-only residual of the 2-D 5-point Jacobi update (fp64), for gfx950.
//
//   d[y][x] = c0*((u[y][x-1] + u[y][x+1]) + (u[y-1][x] + u[y+1][x])) [+ c1*f[y][x]] - u[y][x]
//   out[0]  = sum d^2 (not square-rooted: partial results can be all-reduced)
//   out[1]  = max |d| (a NaN d counts as +inf)
//
// u is never written: one HBM read pass, 8 B/pt, where the residual of
// gmt_jacobi5 moves 16 B/pt and advances the field.
//
// jacobi5_resid_walk: without a store a tile kernel (jacobi5_pt) would read
// every point three times from L2 for each 8 B of HBM, so this one walks
// (row_walk.hpp): a row is loaded once per segment and only accumulated.
// jacobi5_resid_scalar: one cell per lane, for odd alignment.
//
// The cell is evaluated without contraction (as the CPU backend's), so the
// result does not depend on how the compiler fuses c0*(...) - u.
#include "common.hpp"
#include "reduce_partials.hpp"
#include "row_walk.hpp"
#include "gmt/kernels.h"

namespace gmt {

// row loads in flight per lane (with f, two: its pairs double the registers
// of a row, and four would cost the eighth wave per SIMD)
constexpr int kResidUnrollU = 4, kResidUnrollF = 2;

template <bool HAS_F>
__device__ __forceinline__ double resid_cell(double w, double e, double n, double s, double c, double c0,
                                             double c1, double fv) {
#pragma clang fp contract(off)
  double o = c0 * ((w + e) + (n + s));
  if (HAS_F) o = o + c1 * fv;
  return o - c;
}

__device__ __forceinline__ void resid_acc(double d, bool on, double& acc, double& m) {
  const double ad = fabs(d);
  acc += on ? d * d : 0.0;
  m = fmax(m, on ? (d != d ? __builtin_inf() : ad) : 0.0);
}

// the walk's op: nothing of its own to load or store, a row is accumulated
template <bool HAS_F>
struct ResidOp {
  double c0, c1;
  double acc = 0.0, m = 0.0;
  __device__ __forceinline__ void begin(int64_t, int64_t, int64_t) {}
  __device__ __forceinline__ void load(int, int64_t) {}
  __device__ __forceinline__ void row(int, double w, double e, d2 a, d2 b, d2 c, d2 f, bool live, bool pair) {
    const double dx = resid_cell<HAS_F>(w, b.y, a.x, c.x, b.x, c0, c1, f.x);
    const double dy = resid_cell<HAS_F>(b.x, e, a.y, c.y, b.y, c0, c1, f.y);
    resid_acc(dx, live, acc, m);
    resid_acc(dy, pair, acc, m);
  }
  __device__ __forceinline__ void advance(int) {}
};

template <bool HAS_F>
__global__ __launch_bounds__(kBlock) void jacobi5_resid_walk(int64_t x0, int64_t nx, int64_t y0, int64_t ny,
                                                             const double* __restrict__ u, int64_t ld,
                                                             const double* __restrict__ f, int64_t ldf,
                                                             double c0, double c1, double* __restrict__ psum,
                                                             double* __restrict__ pmax, int64_t nseg,
                                                             int64_t seg_rows, int64_t nblocks) {
  ResidOp<HAS_F> op{c0, c1};
  row_walk<HAS_F ? kResidUnrollF : kResidUnrollU, HAS_F>(x0, nx, y0, ny, u, ld, f, ldf, nseg, seg_rows, nblocks, op);
  write_block_partials(op.acc, op.m, psum, pmax);
}

template <bool HAS_F>
__global__ __launch_bounds__(kBlock) void jacobi5_resid_scalar(int64_t x0, int64_t nx, int64_t y0, int64_t ny,
                                                               const double* __restrict__ u, int64_t ld,
                                                               const double* __restrict__ f, int64_t ldf,
                                                               double c0, double c1, double* __restrict__ psum,
                                                               double* __restrict__ pmax) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  double acc = 0.0, m = 0.0;
  if (i < nx * ny) {
    const int64_t x = x0 + i % nx, y = y0 + i / nx;
    const double* pc = u + y * ld + x;
    const double d = resid_cell<HAS_F>(pc[-1], pc[1], pc[-ld], pc[ld], pc[0], c0, c1, HAS_F ? f[y * ldf + x] : 0.0);
    resid_acc(d, true, acc, m);
  }
  write_block_partials(acc, m, psum, pmax);
}

static int64_t resid_max_blocks(int64_t nx, int64_t ny) {
  int64_t nseg, L;
  const int64_t a = walk_blocks(nx, ny, &nseg, &L), b = (nx * ny + kBlock - 1) / kBlock;
  return a > b ? a : b;
}
// pairs per lane need 16-B aligned rows and an even first column
static int resid_path(int64_t x0, const double* u, int64_t ld, const double* f, int64_t ldf) {
  return x0 % 2 == 0 && walk_vec_ok(u, ld) && (!f || walk_vec_ok(f, ldf)) ? GMT_PATH_ROW_WALK : GMT_PATH_SCALAR;
}

}  // namespace gmt

// workspace layout: sum partials [nbmax] | level-2 slots [kL2] | max partials [nbmax] | level-2 slots [kL2]
extern "C" int64_t gmt_jacobi5_resid_workspace(int64_t nx, int64_t ny) {
  using namespace gmt;
  if (nx <= 0 || ny <= 0) return 2;
  return 2 * (resid_max_blocks(nx, ny) + kL2);
}

extern "C" int gmt_jacobi5_resid_path(int64_t x0, int64_t nx, int64_t ny, const double* u, int64_t ld,
                                      const double* f, int64_t ldf, int64_t* seg_rows) {
  using namespace gmt;
  const int path = resid_path(x0, u, ld, f, ldf);
  if (seg_rows) *seg_rows = path == GMT_PATH_ROW_WALK && nx > 0 && ny > 0 ? walk_seg_rows(nx, ny) : 0;
  return path;
}

extern "C" int gmt_jacobi5_resid(int64_t x0, int64_t nx, int64_t y0, int64_t ny, const double* u, int64_t ld,
                                 const double* f, int64_t ldf, double c0, double c1, double* out,
                                 double* workspace, void* stream) {
  using namespace gmt;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (!out) return static_cast<int>(hipErrorInvalidValue);
  if (nx <= 0 || ny <= 0) return static_cast<int>(hipMemsetAsync(out, 0, 2 * sizeof(double), s));
  if (!u || !workspace || x0 < 1 || y0 < 1 || ld < x0 + nx + 1) return static_cast<int>(hipErrorInvalidValue);
  const int64_t half = resid_max_blocks(nx, ny) + kL2;
  double* psum = workspace;
  double* pmax = workspace + half;
  int64_t nb;
  if (resid_path(x0, u, ld, f, ldf) == GMT_PATH_ROW_WALK) {
    int64_t nseg, L;
    nb = walk_blocks(nx, ny, &nseg, &L);
    if (f)
      jacobi5_resid_walk<true><<<grid_1d(nb), kBlock, 0, s>>>(x0, nx, y0, ny, u, ld, f, ldf, c0, c1, psum, pmax,
                                                              nseg, L, nb);
    else
      jacobi5_resid_walk<false><<<grid_1d(nb), kBlock, 0, s>>>(x0, nx, y0, ny, u, ld, f, ldf, c0, c1, psum, pmax,
                                                               nseg, L, nb);
  } else {
    nb = (nx * ny + kBlock - 1) / kBlock;
    if (f)
      jacobi5_resid_scalar<true><<<grid_1d(nb), kBlock, 0, s>>>(x0, nx, y0, ny, u, ld, f, ldf, c0, c1, psum, pmax);
    else
      jacobi5_resid_scalar<false><<<grid_1d(nb), kBlock, 0, s>>>(x0, nx, y0, ny, u, ld, f, ldf, c0, c1, psum, pmax);
  }
  reduce_sum_max(psum, pmax, nb, out, s);
  GMT_RET_LAUNCH();
}
