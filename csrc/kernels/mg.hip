// The kernels of one geometric multigrid V-cycle over the Jacobi sweep
// (JacobiSolver::mg, gmt/kernels.h), fp64, hand-written for gfx950: the damped
// Jacobi smoother and the two grid transfers between a vertex-centred level
// and the next coarser one (coarse point (J, I) on fine point (2J+1, 2I+1)).
//
//   mg_smooth_walk      out = u + omega*(G(u) - u): the row walk of
//                       row_walk.hpp over u; the centre pair is the walk's own
//                       row b, so a row adds one 16-B store and nothing else:
//                       16 B/pt (24 with f).
//   mg_restrict_pt      full weighting: one lane per pair of coarse cells, the
//                       five fine columns of a row by two 16-B loads and one
//                       8-B load, one 16-B store.  Neighbouring lanes and rows
//                       re-read fine cells out of L2: the DPP row walk the
//                       smoother has is not built for it yet.
//   mg_prolong_pt       bilinear interpolation added in place: one lane per
//                       fine pair, a 16-B read-modify-write of u, the coarse
//                       cells by 8-B loads (L2 hits: four fine cells share them).
//   *_scalar            one cell per lane, for odd alignment or pitches.
//
// Every cell is evaluated without contraction, as the CPU backend's.
#include "common.hpp"
#include "row_walk.hpp"
#include "gmt/kernels.h"

namespace gmt {

// row loads in flight per lane (as the Chebyshev step's)
constexpr int kMgUnrollP = 4, kMgUnrollF = 2;

template <bool HAS_F>
__device__ __forceinline__ double mg_smooth_cell(double w, double e, double n, double s, double u, double c0,
                                                 double c1, double fv, double om) {
#pragma clang fp contract(off)
  double o = c0 * ((w + e) + (n + s));
  if (HAS_F) o = o + c1 * fv;
  const double t = o - u;
  const double wt = om * t;
  return u + wt;
}

// the walk's op: no loads of its own, one store of the damped pair
template <bool HAS_F>
struct MgSmoothOp {
  double c0, c1, om;
  double* __restrict__ out;
  int64_t ldo;
  double* po;  // stores: the lane's own column
  __device__ __forceinline__ void begin(int64_t row, int64_t, int64_t xr) { po = out + row * ldo + xr; }
  __device__ __forceinline__ void load(int, int64_t) {}
  __device__ __forceinline__ void row(int j, double w, double e, d2 a, d2 b, d2 c, d2 f, bool live, bool pair) {
    d2 o;
    o.x = mg_smooth_cell<HAS_F>(w, b.y, a.x, c.x, b.x, c0, c1, f.x, om);
    o.y = mg_smooth_cell<HAS_F>(b.x, e, a.y, c.y, b.y, c0, c1, f.y, om);
    if (pair)
      st2(po + j * ldo, o);
    else if (live)
      po[j * ldo] = o.x;
  }
  __device__ __forceinline__ void advance(int rows) { po += rows * ldo; }
};

template <bool HAS_F>
__global__ __launch_bounds__(kBlock) void mg_smooth_walk(int64_t x0, int64_t nx, int64_t y0, int64_t ny,
                                                         const double* __restrict__ u, int64_t ld,
                                                         const double* __restrict__ f, int64_t ldf, double c0,
                                                         double c1, double om, double* __restrict__ out,
                                                         int64_t ldo, int64_t nseg, int64_t seg_rows,
                                                         int64_t nblocks) {
  constexpr int kUnroll = HAS_F ? kMgUnrollF : kMgUnrollP;
  MgSmoothOp<HAS_F> op{c0, c1, om, out, ldo, nullptr};
  row_walk<kUnroll, HAS_F>(x0, nx, y0, ny, u, ld, f, ldf, nseg, seg_rows, nblocks, op);
}

template <bool HAS_F>
__global__ __launch_bounds__(kBlock) void mg_smooth_scalar(int64_t x0, int64_t nx, int64_t y0, int64_t ny,
                                                           const double* __restrict__ u, int64_t ld,
                                                           const double* __restrict__ f, int64_t ldf, double c0,
                                                           double c1, double om, double* __restrict__ out,
                                                           int64_t ldo) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= nx * ny) return;
  const int64_t x = x0 + i % nx, y = y0 + i / nx;
  const double* pc = u + y * ld + x;
  out[y * ldo + x] =
      mg_smooth_cell<HAS_F>(pc[-1], pc[1], pc[-ld], pc[ld], *pc, c0, c1, HAS_F ? f[y * ldf + x] : 0.0, om);
}

static int mg_smooth_path(int64_t x0, const double* u, int64_t ld, const double* f, int64_t ldf, const double* out,
                          int64_t ldo) {
  return x0 % 2 == 0 && walk_vec_ok(u, ld) && walk_vec_ok(out, ldo) && (!f || walk_vec_ok(f, ldf))
             ? GMT_PATH_ROW_WALK
             : GMT_PATH_SCALAR;
}

template <bool HAS_F>
static int mg_smooth_launch(bool walk, int64_t x0, int64_t nx, int64_t y0, int64_t ny, const double* u, int64_t ld,
                            const double* f, int64_t ldf, double c0, double c1, double om, double* out, int64_t ldo,
                            hipStream_t s) {
  if (walk) {
    int64_t nseg, L;
    const int64_t nb = walk_blocks(nx, ny, &nseg, &L);
    if (nb > INT32_MAX) return static_cast<int>(hipErrorInvalidValue);  // the grid's x extent
    mg_smooth_walk<HAS_F><<<grid_1d(nb), kBlock, 0, s>>>(x0, nx, y0, ny, u, ld, f, ldf, c0, c1, om, out, ldo, nseg, L,
                                                         nb);
  } else {
    const int64_t nb = (nx * ny + kBlock - 1) / kBlock;
    if (nb > INT32_MAX) return static_cast<int>(hipErrorInvalidValue);
    mg_smooth_scalar<HAS_F><<<grid_1d(nb), kBlock, 0, s>>>(x0, nx, y0, ny, u, ld, f, ldf, c0, c1, om, out, ldo);
  }
  GMT_RET_LAUNCH();
}

// ---- full weighting ----

// H(r) of one coarse column: (d[r][x-1] + d[r][x+1]) + 2*d[r][x]
__device__ __forceinline__ double mg_h(double w, double c, double e) {
#pragma clang fp contract(off)
  const double t = 2.0 * c;
  return (w + e) + t;
}
// cs*((H(y-1) + H(y+1)) + 2*H(y))
__device__ __forceinline__ double mg_full_weight(double hs, double hc, double hn, double cs) {
#pragma clang fp contract(off)
  const double t = 2.0 * hc;
  return cs * ((hs + hn) + t);
}

__global__ __launch_bounds__(kBlock) void mg_restrict_scalar(int64_t x0, int64_t y0, int px, int py, int64_t mx,
                                                             int64_t my, const double* __restrict__ d, int64_t ldd,
                                                             double cs, double* __restrict__ sc, int64_t cx0,
                                                             int64_t cy0, int64_t ldc) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= mx * my) return;
  const int64_t I = i % mx, J = i / mx;
  const double* p = d + (y0 + py + 2 * J) * ldd + x0 + px + 2 * I;  // the coarse point's fine cell
  const double hs = mg_h(p[-ldd - 1], p[-ldd], p[-ldd + 1]);
  const double hc = mg_h(p[-1], p[0], p[1]);
  const double hn = mg_h(p[ldd - 1], p[ldd], p[ldd + 1]);
  sc[(cy0 + J) * ldc + cx0 + I] = mg_full_weight(hs, hc, hn, cs);
}

// the five fine columns x-1 .. x+3 around a pair of coarse points at x, x+2
// (x0 even: x is odd with px = 1, even with px = 0; uniform over the launch)
__device__ __forceinline__ void mg_ld5(const double* p, int px, double v[5]) {
  if (px) {
    const d2 a = ld2(p - 1), b = ld2(p + 1);
    v[0] = a.x, v[1] = a.y, v[2] = b.x, v[3] = b.y, v[4] = p[3];
  } else {
    const d2 a = ld2(p), b = ld2(p + 2);
    v[0] = p[-1], v[1] = a.x, v[2] = a.y, v[3] = b.x, v[4] = b.y;
  }
}

__global__ __launch_bounds__(kBlock) void mg_restrict_pt(int64_t x0, int64_t y0, int px, int py, int64_t mx,
                                                         int64_t my, const double* __restrict__ d, int64_t ldd,
                                                         double cs, double* __restrict__ sc, int64_t cx0,
                                                         int64_t cy0, int64_t ldc) {
  const int64_t npx = (mx + 1) / 2;  // coarse pairs per coarse row
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= npx * my) return;
  const int64_t I = 2 * (i % npx), J = i / npx;
  const double* p = d + (y0 + py + 2 * J) * ldd + x0 + px + 2 * I;
  double* q = sc + (cy0 + J) * ldc + cx0 + I;
  if (I + 1 < mx) {
    double s[5], c[5], n[5];
    mg_ld5(p - ldd, px, s);
    mg_ld5(p, px, c);
    mg_ld5(p + ldd, px, n);
    d2 o;
    o.x = mg_full_weight(mg_h(s[0], s[1], s[2]), mg_h(c[0], c[1], c[2]), mg_h(n[0], n[1], n[2]), cs);
    o.y = mg_full_weight(mg_h(s[2], s[3], s[4]), mg_h(c[2], c[3], c[4]), mg_h(n[2], n[3], n[4]), cs);
    st2(q, o);
  } else {  // the single last coarse column of an odd mx: nothing east of its ring is read
    const double hs = mg_h(p[-ldd - 1], p[-ldd], p[-ldd + 1]);
    const double hc = mg_h(p[-1], p[0], p[1]);
    const double hn = mg_h(p[ldd - 1], p[ldd], p[ldd + 1]);
    *q = mg_full_weight(hs, hc, hn, cs);
  }
}

// ---- bilinear interpolation, added in place ----

// u' of region-relative fine cell (i, j); e points at coarse cell (cx0, cy0)
__device__ __forceinline__ double mg_prolong_cell(const double* __restrict__ e, int64_t lde, int64_t i, int64_t j,
                                                  int px, int py, double u) {
#pragma clang fp contract(off)
  const int64_t di = i - px, dj = j - py;  // >= -1
  const bool onx = (di & 1) == 0, ony = (dj & 1) == 0;
  // the coarse column / row the cell sits on, else the one west / south of it (-1: the ring)
  const int64_t I = onx ? di / 2 : (di + 1) / 2 - 1;
  const int64_t J = ony ? dj / 2 : (dj + 1) / 2 - 1;
  const double* p = e + J * lde + I;
  if (onx && ony) return u + p[0];
  if (ony) {
    const double t = 0.5 * (p[0] + p[1]);
    return u + t;
  }
  if (onx) {
    const double t = 0.5 * (p[0] + p[lde]);
    return u + t;
  }
  const double t = 0.25 * ((p[0] + p[1]) + (p[lde] + p[lde + 1]));
  return u + t;
}

__global__ __launch_bounds__(kBlock) void mg_prolong_scalar(int64_t x0, int64_t nx, int64_t y0, int64_t ny, int px,
                                                            int py, const double* __restrict__ e, int64_t lde,
                                                            double* __restrict__ u, int64_t ld) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (t >= nx * ny) return;
  const int64_t i = t % nx, j = t / nx;
  double* q = u + (y0 + j) * ld + x0 + i;
  *q = mg_prolong_cell(e, lde, i, j, px, py, *q);
}

__global__ __launch_bounds__(kBlock) void mg_prolong_pt(int64_t x0, int64_t nx, int64_t y0, int64_t ny, int px,
                                                        int py, const double* __restrict__ e, int64_t lde,
                                                        double* __restrict__ u, int64_t ld) {
  const int64_t npx = (nx + 1) / 2;  // fine pairs per row
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (t >= npx * ny) return;
  const int64_t i = 2 * (t % npx), j = t / npx;
  double* q = u + (y0 + j) * ld + x0 + i;
  if (i + 1 < nx) {
    d2 v = ld2(q);
    v.x = mg_prolong_cell(e, lde, i, j, px, py, v.x);
    v.y = mg_prolong_cell(e, lde, i + 1, j, px, py, v.y);
    st2(q, v);
  } else {
    *q = mg_prolong_cell(e, lde, i, j, px, py, *q);
  }
}

static int mg_restrict_path(int64_t x0, int64_t cx0, const double* d, int64_t ldd, const double* sc, int64_t ldc) {
  return x0 % 2 == 0 && cx0 % 2 == 0 && walk_vec_ok(d, ldd) && walk_vec_ok(sc, ldc) ? GMT_PATH_PT : GMT_PATH_SCALAR;
}
static int mg_prolong_path(int64_t x0, const double* e, int64_t lde, const double* u, int64_t ld) {
  return x0 % 2 == 0 && walk_vec_ok(e, lde) && walk_vec_ok(u, ld) ? GMT_PATH_PT : GMT_PATH_SCALAR;
}

}  // namespace gmt

extern "C" int gmt_mg_smooth_path(int64_t x0, int64_t nx, int64_t ny, const double* u, int64_t ld, const double* f,
                                  int64_t ldf, const double* out, int64_t ldo, int64_t* seg_rows) {
  using namespace gmt;
  const int path = mg_smooth_path(x0, u, ld, f, ldf, out, ldo);
  if (seg_rows) *seg_rows = path == GMT_PATH_ROW_WALK && nx > 0 && ny > 0 ? walk_seg_rows(nx, ny) : 0;
  return path;
}

extern "C" int gmt_mg_smooth(int64_t x0, int64_t nx, int64_t y0, int64_t ny, const double* u, int64_t ld,
                             const double* f, int64_t ldf, double c0, double c1, double omega, double* out,
                             int64_t ldo, void* stream) {
  using namespace gmt;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (nx < 0 || ny < 0) return static_cast<int>(hipErrorInvalidValue);
  if (nx == 0 || ny == 0) return 0;
  if (!u || !out || x0 < 1 || y0 < 1 || ld < x0 + nx + 1 || ldo < x0 + nx || (f && ldf < x0 + nx))
    return static_cast<int>(hipErrorInvalidValue);
  const bool walk = mg_smooth_path(x0, u, ld, f, ldf, out, ldo) == GMT_PATH_ROW_WALK;
  return f ? mg_smooth_launch<true>(walk, x0, nx, y0, ny, u, ld, f, ldf, c0, c1, omega, out, ldo, s)
           : mg_smooth_launch<false>(walk, x0, nx, y0, ny, u, ld, f, ldf, c0, c1, omega, out, ldo, s);
}

extern "C" int gmt_mg_restrict_path(int64_t x0, int64_t cx0, const double* d, int64_t ldd, const double* sc,
                                    int64_t ldc) {
  return gmt::mg_restrict_path(x0, cx0, d, ldd, sc, ldc);
}

extern "C" int gmt_mg_restrict(int64_t x0, int64_t nx, int64_t y0, int64_t ny, int px, int py, const double* d,
                               int64_t ldd, double cs, double* sc, int64_t cx0, int64_t cy0, int64_t ldc,
                               void* stream) {
  using namespace gmt;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (nx < 0 || ny < 0) return static_cast<int>(hipErrorInvalidValue);
  if (nx == 0 || ny == 0) return 0;
  if (px < 0 || px > 1 || py < 0 || py > 1) return static_cast<int>(hipErrorInvalidValue);
  const int64_t mx = (nx - px + 1) / 2, my = (ny - py + 1) / 2;
  if (!d || !sc || x0 < 1 || y0 < 1 || cx0 < 0 || cy0 < 0 || ldd < x0 + nx + 1 || ldc < cx0 + mx)
    return static_cast<int>(hipErrorInvalidValue);
  if (mx == 0 || my == 0) return 0;  // no coarse point on the region
  if (mg_restrict_path(x0, cx0, d, ldd, sc, ldc) == GMT_PATH_PT) {
    const int64_t nb = ((mx + 1) / 2 * my + kBlock - 1) / kBlock;
    if (nb > INT32_MAX) return static_cast<int>(hipErrorInvalidValue);
    mg_restrict_pt<<<grid_1d(nb), kBlock, 0, s>>>(x0, y0, px, py, mx, my, d, ldd, cs, sc, cx0, cy0, ldc);
  } else {
    const int64_t nb = (mx * my + kBlock - 1) / kBlock;
    if (nb > INT32_MAX) return static_cast<int>(hipErrorInvalidValue);
    mg_restrict_scalar<<<grid_1d(nb), kBlock, 0, s>>>(x0, y0, px, py, mx, my, d, ldd, cs, sc, cx0, cy0, ldc);
  }
  GMT_RET_LAUNCH();
}

extern "C" int gmt_mg_prolong_add_path(int64_t x0, const double* e, int64_t lde, const double* u, int64_t ld) {
  return gmt::mg_prolong_path(x0, e, lde, u, ld);
}

extern "C" int gmt_mg_prolong_add(int64_t x0, int64_t nx, int64_t y0, int64_t ny, int px, int py, const double* e,
                                  int64_t cx0, int64_t cy0, int64_t lde, double* u, int64_t ld, void* stream) {
  using namespace gmt;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (nx < 0 || ny < 0) return static_cast<int>(hipErrorInvalidValue);
  if (nx == 0 || ny == 0) return 0;
  if (px < 0 || px > 1 || py < 0 || py > 1) return static_cast<int>(hipErrorInvalidValue);
  const int64_t mx = (nx - px + 1) / 2;
  if (!e || !u || x0 < 1 || y0 < 1 || cx0 < 1 || cy0 < 1 || lde < cx0 + mx + 1 || ld < x0 + nx)
    return static_cast<int>(hipErrorInvalidValue);
  const double* e0 = e + cy0 * lde + cx0;
  if (mg_prolong_path(x0, e, lde, u, ld) == GMT_PATH_PT) {
    const int64_t nb = ((nx + 1) / 2 * ny + kBlock - 1) / kBlock;
    if (nb > INT32_MAX) return static_cast<int>(hipErrorInvalidValue);
    mg_prolong_pt<<<grid_1d(nb), kBlock, 0, s>>>(x0, nx, y0, ny, px, py, e0, lde, u, ld);
  } else {
    const int64_t nb = (nx * ny + kBlock - 1) / kBlock;
    if (nb > INT32_MAX) return static_cast<int>(hipErrorInvalidValue);
    mg_prolong_scalar<<<grid_1d(nb), kBlock, 0, s>>>(x0, nx, y0, ny, px, py, e0, lde, u, ld);
  }
  GMT_RET_LAUNCH();
}
