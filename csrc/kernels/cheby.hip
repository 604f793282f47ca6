// One Chebyshev semi-iteration over the Jacobi sweep (Golub-Varga), fp64,
// hand-written for gfx950: the single launch of an iteration of
// JacobiSolver::cheby (gmt/kernels.h).
//
//   v' = v + w*(G(u) - v),   G(u) = c0*((W+E)+(S+N)) [+ c1*f]
//
// u is the current iterate, v the previous one, overwritten in place by the
// next; w is the iteration's weight, passed by value.
//
//   cheby_step_walk    the row walk of cg_apply_walk / jacobi5_resid_walk: four
//                      waves side by side on one row segment, one column pair
//                      per lane, a three-row register window of u walked
//                      top-down, W/E neighbours through DPP, one masked load
//                      for each column outside the wave, xcd_swizzle so the
//                      rows two segments share stay in one L2.  Each row adds
//                      one 16-B load of v (and of f), issued with that row's u
//                      loads, and one 16-B store of v': 24 B/pt (32 with f).
//                      No reductions, no workspace.
//   cheby_step_scalar  one cell per lane, for odd alignment or pitches.
//
// The cell expression is evaluated without contraction, as the CPU backend's.
//
// Stores: v' is the next iteration's stencil operand and uses plain stores.
// GMT_CHEBY_NT (bit 0: nontemporal load of v, bit 1: nontemporal store of v')
// rebuilds the file with another policy for the A/B recorded in
// profiles/cheby/README.md.
#include "common.hpp"
#include "gmt/kernels.h"

#ifndef GMT_CHEBY_NT
#define GMT_CHEBY_NT 0
#endif

namespace gmt {

constexpr int kChWaveCols = 2 * kWave;                        // columns per wave
constexpr int kChBlockCols = kChWaveCols * (kBlock / kWave);  // columns per workgroup
// row loads in flight per lane (with f, two: its pairs add a third of the registers of a row)
constexpr int kChUnrollP = 4, kChUnrollF = 2;
constexpr int64_t kChMaxSeg = 256, kChMinSeg = 8;

template <bool HAS_F>
__device__ __forceinline__ double cheby_cell(double w, double e, double n, double s, double v, double c0, double c1,
                                             double fv, double om) {
#pragma clang fp contract(off)
  double o = c0 * ((w + e) + (n + s));
  if (HAS_F) o = o + c1 * fv;
  const double t = o - v;
  const double wt = om * t;
  return v + wt;
}

__device__ __forceinline__ d2 cheby_ldv(const double* p) { return (GMT_CHEBY_NT & 1) ? ld2_nt(p) : ld2(p); }
__device__ __forceinline__ void cheby_stv(double* p, d2 v) {
  if (GMT_CHEBY_NT & 2)
    st2_nt(p, v);
  else
    st2(p, v);
}

template <bool HAS_F>
__global__ __launch_bounds__(kBlock) void cheby_step_walk(int64_t x0, int64_t nx, int64_t y0, int64_t ny,
                                                          const double* __restrict__ u, int64_t ld,
                                                          const double* __restrict__ f, int64_t ldf, double c0,
                                                          double c1, double om, double* __restrict__ v,
                                                          int64_t ldv, int64_t nseg, int64_t seg_rows,
                                                          int64_t nblocks) {
  const int64_t t = xcd_swizzle(blockIdx.x, nblocks);
  const int64_t seg = t % nseg, bx = t / nseg;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int64_t xw = bx * kChBlockCols + wave * kChWaveCols;  // the wave's first column
  constexpr int kUnroll = HAS_F ? kChUnrollF : kChUnrollP;
  if (xw >= nx) return;  // wave-uniform: every lane of a working wave stays active (DPP)
  const int64_t r0 = seg * seg_rows;
  const int64_t r1 = (r0 + seg_rows) < ny ? (r0 + seg_rows) : ny;
  const int64_t xr = xw + 2 * lane;
  const bool live = xr < nx, pair = xr + 1 < nx;
  // lanes past the region re-read its last pair (their cells are masked and
  // never stored); the lane of an odd last column loads the pair too: its
  // second value of u is the cell's E neighbour, that of v and f is unused
  const int64_t xl = live ? xr : ((nx - 1) & ~int64_t(1));
  const bool west = lane == 0;
  const bool east = pair && (lane == kWave - 1 || xr + 2 >= nx);
  const double* p = u + (y0 + r0 - 1) * ld + x0 + xl;
  const double* pf = HAS_F ? f + (y0 + r0) * ldf + x0 + xl : nullptr;
  const double* pv = v + (y0 + r0) * ldv + x0 + xl;
  double* po = v + (y0 + r0) * ldv + x0 + xr;  // dereferenced by live lanes only
  d2 a = ld2(p);  // row r - 1
  p += ld;
  d2 b = ld2(p);  // row r
  for (int64_t r = r0; r < r1; r += kUnroll) {
    const int64_t left = r1 - r;  // rows still to do, >= 1
    d2 c[kUnroll], vv[kUnroll], fv[kUnroll];
    double ew[kUnroll], ee[kUnroll];
#pragma unroll
    for (int j = 0; j < kUnroll; ++j) {
      // rows past the segment are clamped to its last ones (loaded, not used)
      const int64_t oc = (j + 1 < left ? j + 1 : left) * ld;
      const int64_t jr = j < left - 1 ? j : left - 1;
      c[j] = ld2(p + oc);
      ew[j] = ee[j] = 0.0;
      if (west) ew[j] = p[jr * ld - 1];
      if (east) ee[j] = p[jr * ld + 2];
      vv[j] = cheby_ldv(pv + jr * ldv);
      if (HAS_F) fv[j] = ld2(pf + jr * ldf);
    }
#pragma unroll
    for (int j = 0; j < kUnroll; ++j) {
      if (j < left) {
        const double wl = dpp_from_lower(b.y), eu = dpp_from_upper(b.x);
        const double w = west ? ew[j] : wl, e = east ? ee[j] : eu;
        d2 o;
        o.x = cheby_cell<HAS_F>(w, b.y, a.x, c[j].x, vv[j].x, c0, c1, HAS_F ? fv[j].x : 0.0, om);
        o.y = cheby_cell<HAS_F>(b.x, e, a.y, c[j].y, vv[j].y, c0, c1, HAS_F ? fv[j].y : 0.0, om);
        if (pair)
          cheby_stv(po + j * ldv, o);
        else if (live)
          po[j * ldv] = o.x;
      }
      a = b;
      b = c[j];
    }
    p += kUnroll * ld;
    pv += kUnroll * ldv;
    po += kUnroll * ldv;
    if (HAS_F) pf += kUnroll * ldf;
  }
}

template <bool HAS_F>
__global__ __launch_bounds__(kBlock) void cheby_step_scalar(int64_t x0, int64_t nx, int64_t y0, int64_t ny,
                                                            const double* __restrict__ u, int64_t ld,
                                                            const double* __restrict__ f, int64_t ldf, double c0,
                                                            double c1, double om, double* __restrict__ v,
                                                            int64_t ldv) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= nx * ny) return;
  const int64_t x = x0 + i % nx, y = y0 + i / nx;
  const double* pc = u + y * ld + x;
  double* pv = v + y * ldv + x;
  *pv = cheby_cell<HAS_F>(pc[-1], pc[1], pc[-ld], pc[ld], *pv, c0, c1, HAS_F ? f[y * ldf + x] : 0.0, om);
}

// Rows per segment of the row walk: jacobi5_resid.hip's rule (as long as
// possible while the launch still has 8 workgroups per compute unit)
static int64_t cheby_seg_rows(int64_t nx, int64_t ny) {
  static const int cus = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
    return n;
  }();
  const int64_t nbx = (nx + kChBlockCols - 1) / kChBlockCols;
  int64_t L = kChMaxSeg;
  while (L > kChMinSeg && nbx * ((ny + L - 1) / L) < 8 * static_cast<int64_t>(cus)) L /= 2;
  return L;
}
static bool cheby_vec_ok(const double* a, int64_t ld) { return aligned16(a) && ld % 2 == 0; }

static int cheby_path(int64_t x0, const double* u, int64_t ld, const double* f, int64_t ldf, const double* v,
                      int64_t ldv) {
  return x0 % 2 == 0 && cheby_vec_ok(u, ld) && cheby_vec_ok(v, ldv) && (!f || cheby_vec_ok(f, ldf))
             ? GMT_PATH_ROW_WALK
             : GMT_PATH_SCALAR;
}

template <bool HAS_F>
static int cheby_launch(bool walk, int64_t x0, int64_t nx, int64_t y0, int64_t ny, const double* u, int64_t ld,
                        const double* f, int64_t ldf, double c0, double c1, double om, double* v, int64_t ldv,
                        hipStream_t s) {
  if (walk) {
    const int64_t L = cheby_seg_rows(nx, ny), nseg = (ny + L - 1) / L;
    const int64_t nb = ((nx + kChBlockCols - 1) / kChBlockCols) * nseg;
    if (nb > INT32_MAX) return static_cast<int>(hipErrorInvalidValue);  // the grid's x extent
    cheby_step_walk<HAS_F><<<grid_1d(nb), kBlock, 0, s>>>(x0, nx, y0, ny, u, ld, f, ldf, c0, c1, om, v, ldv, nseg, L,
                                                          nb);
  } else {
    const int64_t nb = (nx * ny + kBlock - 1) / kBlock;
    if (nb > INT32_MAX) return static_cast<int>(hipErrorInvalidValue);
    cheby_step_scalar<HAS_F><<<grid_1d(nb), kBlock, 0, s>>>(x0, nx, y0, ny, u, ld, f, ldf, c0, c1, om, v, ldv);
  }
  GMT_RET_LAUNCH();
}

}  // namespace gmt

extern "C" int gmt_cheby_step_path(int64_t x0, int64_t nx, int64_t ny, const double* u, int64_t ld, const double* f,
                                   int64_t ldf, const double* v, int64_t ldv, int64_t* seg_rows) {
  using namespace gmt;
  const int path = cheby_path(x0, u, ld, f, ldf, v, ldv);
  if (seg_rows) *seg_rows = path == GMT_PATH_ROW_WALK && nx > 0 && ny > 0 ? cheby_seg_rows(nx, ny) : 0;
  return path;
}

extern "C" int gmt_cheby_step(int64_t x0, int64_t nx, int64_t y0, int64_t ny, const double* u, int64_t ld,
                              const double* f, int64_t ldf, double c0, double c1, double w, double* v, int64_t ldv,
                              void* stream) {
  using namespace gmt;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (nx < 0 || ny < 0) return static_cast<int>(hipErrorInvalidValue);
  if (nx == 0 || ny == 0) return 0;
  if (!u || !v || x0 < 1 || y0 < 1 || ld < x0 + nx + 1 || ldv < x0 + nx || (f && ldf < x0 + nx))
    return static_cast<int>(hipErrorInvalidValue);
  const bool walk = cheby_path(x0, u, ld, f, ldf, v, ldv) == GMT_PATH_ROW_WALK;
  return f ? cheby_launch<true>(walk, x0, nx, y0, ny, u, ld, f, ldf, c0, c1, w, v, ldv, s)
           : cheby_launch<false>(walk, x0, nx, y0, ny, u, ld, f, ldf, c0, c1, w, v, ldv, s);
}
