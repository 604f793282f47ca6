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
// every point three times from L2 for each 8 B of HBM, so this one walks.
// A workgroup is four waves side by side (512 columns) on one row segment;
// each lane holds one column pair and each wave walks its 128 columns
// top-down with a three-row register window, so a row is loaded once per
// segment (plus the two rows around the segment).  The W/E neighbours of a
// pair come from the adjacent lanes through DPP; the two columns outside the
// wave come from one masked load each.  kRwUnroll rows are in flight per
// lane.  Vertically adjacent segments of a strip are consecutive tiles, so
// xcd_swizzle keeps the rows they share in one L2.
// jacobi5_resid_scalar: one cell per lane, for odd alignment.
//
// The cell is evaluated without contraction (as the CPU backend's), so the
// result does not depend on how the compiler fuses c0*(...) - u.
#include "common.hpp"
#include "reduce_partials.hpp"
#include "gmt/kernels.h"

namespace gmt {

constexpr int kRwWaveCols = 2 * kWave;                         // columns per wave
constexpr int kRwBlockCols = kRwWaveCols * (kBlock / kWave);   // columns per workgroup
// row loads in flight per lane (with f, two: its pairs double the registers
// of a row, and four would cost the eighth wave per SIMD)
constexpr int kRwUnrollU = 4, kRwUnrollF = 2;
constexpr int64_t kRwMaxSeg = 256, kRwMinSeg = 8;

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

template <bool HAS_F>
__global__ __launch_bounds__(kBlock) void jacobi5_resid_walk(int64_t x0, int64_t nx, int64_t y0, int64_t ny,
                                                             const double* __restrict__ u, int64_t ld,
                                                             const double* __restrict__ f, int64_t ldf,
                                                             double c0, double c1, double* __restrict__ psum,
                                                             double* __restrict__ pmax, int64_t nseg,
                                                             int64_t seg_rows, int64_t nblocks) {
  const int64_t t = xcd_swizzle(blockIdx.x, nblocks);
  const int64_t seg = t % nseg, bx = t / nseg;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int64_t xw = bx * kRwBlockCols + wave * kRwWaveCols;  // the wave's first column
  constexpr int kRwUnroll = HAS_F ? kRwUnrollF : kRwUnrollU;
  double acc = 0.0, m = 0.0;
  if (xw < nx) {  // wave-uniform: every lane of a working wave stays active (DPP)
    const int64_t r0 = seg * seg_rows;
    const int64_t r1 = (r0 + seg_rows) < ny ? (r0 + seg_rows) : ny;
    const int64_t xr = xw + 2 * lane;
    const bool live = xr < nx, pair = xr + 1 < nx;
    // lanes past the region re-read its last pair (their cells are masked);
    // the lane of an odd last column loads the pair too: its second value is
    // the cell's E neighbour
    const int64_t xl = live ? xr : ((nx - 1) & ~int64_t(1));
    const bool west = lane == 0;
    const bool east = pair && (lane == kWave - 1 || xr + 2 >= nx);
    const double* p = u + (y0 + r0 - 1) * ld + x0 + xl;
    const double* pf = HAS_F ? f + (y0 + r0) * ldf + x0 + xl : nullptr;
    d2 a = ld2(p);  // row r - 1
    p += ld;
    d2 b = ld2(p);  // row r
    for (int64_t r = r0; r < r1; r += kRwUnroll) {
      const int64_t left = r1 - r;  // rows still to do, >= 1
      d2 c[kRwUnroll], fv[kRwUnroll];
      double ew[kRwUnroll], ee[kRwUnroll];
#pragma unroll
      for (int j = 0; j < kRwUnroll; ++j) {
        // rows past the segment are clamped to its last ones (loaded, not used)
        const int64_t oc = (j + 1 < left ? j + 1 : left) * ld;
        const int64_t jr = j < left - 1 ? j : left - 1;
        c[j] = ld2(p + oc);
        ew[j] = ee[j] = 0.0;
        if (west) ew[j] = p[jr * ld - 1];
        if (east) ee[j] = p[jr * ld + 2];
        if (HAS_F) fv[j] = ld2(pf + jr * ldf);
      }
#pragma unroll
      for (int j = 0; j < kRwUnroll; ++j) {
        if (j < left) {
          const double wl = dpp_from_lower(b.y), eu = dpp_from_upper(b.x);
          const double w = west ? ew[j] : wl, e = east ? ee[j] : eu;
          const double dx = resid_cell<HAS_F>(w, b.y, a.x, c[j].x, b.x, c0, c1, HAS_F ? fv[j].x : 0.0);
          const double dy = resid_cell<HAS_F>(b.x, e, a.y, c[j].y, b.y, c0, c1, HAS_F ? fv[j].y : 0.0);
          resid_acc(dx, live, acc, m);
          resid_acc(dy, pair, acc, m);
        }
        a = b;
        b = c[j];
      }
      p += kRwUnroll * ld;
      if (HAS_F) pf += kRwUnroll * ldf;
    }
  }
  acc = block_sum(acc);
  m = block_max(m);
  if (threadIdx.x == 0) {
    psum[blockIdx.x] = acc;
    pmax[blockIdx.x] = m;
  }
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
  acc = block_sum(acc);
  m = block_max(m);
  if (threadIdx.x == 0) {
    psum[blockIdx.x] = acc;
    pmax[blockIdx.x] = m;
  }
}

// Rows per segment of the row walk: as long as possible (two extra row loads
// per segment) while the launch still has 8 workgroups per compute unit, the
// most a CU holds.  A function of the region and the device only.
static int64_t walk_seg_rows(int64_t nx, int64_t ny) {
  static const int cus = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
    return n;
  }();
  const int64_t nbx = (nx + kRwBlockCols - 1) / kRwBlockCols;
  int64_t L = kRwMaxSeg;
  while (L > kRwMinSeg && nbx * ((ny + L - 1) / L) < 8 * static_cast<int64_t>(cus)) L /= 2;
  return L;
}
static int64_t walk_blocks(int64_t nx, int64_t ny, int64_t* nseg, int64_t* seg_rows) {
  *seg_rows = walk_seg_rows(nx, ny);
  *nseg = (ny + *seg_rows - 1) / *seg_rows;
  return ((nx + kRwBlockCols - 1) / kRwBlockCols) * *nseg;
}
static int64_t resid_max_blocks(int64_t nx, int64_t ny) {
  int64_t nseg, L;
  const int64_t a = walk_blocks(nx, ny, &nseg, &L), b = (nx * ny + kBlock - 1) / kBlock;
  return a > b ? a : b;
}
// pairs per lane need 16-B aligned rows and an even first column
static int resid_path(int64_t x0, const double* u, int64_t ld, const double* f, int64_t ldf) {
  const bool vec_ok = aligned16(u) && (ld % 2 == 0) && (x0 % 2 == 0) && (!f || (aligned16(f) && ldf % 2 == 0));
  return vec_ok ? GMT_PATH_ROW_WALK : GMT_PATH_SCALAR;
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
  reduce_partials<0>(psum, nb, out, s);
  reduce_partials<1>(pmax, nb, out + 1, s);
  GMT_RET_LAUNCH();
}
