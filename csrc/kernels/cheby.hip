// One Chebyshev semi-iteration over the Jacobi sweep (Golub-Varga), fp64,
// hand-written for gfx950: the single launch of an iteration of
// JacobiSolver::cheby (gmt/kernels.h).
//
//   v' = v + w*(G(u) - v),   G(u) = c0*((W+E)+(S+N)) [+ c1*f]
//
// u is the current iterate, v the previous one, overwritten in place by the
// next; w is the iteration's weight, passed by value.
//
//   cheby_step_walk    the row walk of row_walk.hpp over u.  Each row adds one
//                      16-B load of v (and of f), issued with that row's u
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
#include "row_walk.hpp"
#include "gmt/kernels.h"

#ifndef GMT_CHEBY_NT
#define GMT_CHEBY_NT 0
#endif

namespace gmt {

// row loads in flight per lane (with f, two: its pairs add a third of the registers of a row)
constexpr int kChebyUnrollP = 4, kChebyUnrollF = 2;

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

// the walk's op: a row loads its pair of v with its loads of u and stores v'
// over it (the second value a lane of an odd last column loads is unused)
template <bool HAS_F, int UNROLL>
struct ChebyOp {
  double c0, c1, om;
  double* __restrict__ v;
  int64_t ldv;
  const double* pv;  // loads: the clamped column
  double* po;        // stores: the lane's own column
  d2 vv[UNROLL];
  __device__ __forceinline__ void begin(int64_t row, int64_t xl, int64_t xr) {
    pv = v + row * ldv + xl;
    po = v + row * ldv + xr;
  }
  __device__ __forceinline__ void load(int j, int64_t jr) { vv[j] = cheby_ldv(pv + jr * ldv); }
  __device__ __forceinline__ void row(int j, double w, double e, d2 a, d2 b, d2 c, d2 f, bool live, bool pair) {
    d2 o;
    o.x = cheby_cell<HAS_F>(w, b.y, a.x, c.x, vv[j].x, c0, c1, f.x, om);
    o.y = cheby_cell<HAS_F>(b.x, e, a.y, c.y, vv[j].y, c0, c1, f.y, om);
    if (pair)
      cheby_stv(po + j * ldv, o);
    else if (live)
      po[j * ldv] = o.x;
  }
  __device__ __forceinline__ void advance(int rows) {
    pv += rows * ldv;
    po += rows * ldv;
  }
};

template <bool HAS_F>
__global__ __launch_bounds__(kBlock) void cheby_step_walk(int64_t x0, int64_t nx, int64_t y0, int64_t ny,
                                                          const double* __restrict__ u, int64_t ld,
                                                          const double* __restrict__ f, int64_t ldf, double c0,
                                                          double c1, double om, double* __restrict__ v,
                                                          int64_t ldv, int64_t nseg, int64_t seg_rows,
                                                          int64_t nblocks) {
  constexpr int kUnroll = HAS_F ? kChebyUnrollF : kChebyUnrollP;
  ChebyOp<HAS_F, kUnroll> op{c0, c1, om, v, ldv};
  row_walk<kUnroll, HAS_F>(x0, nx, y0, ny, u, ld, f, ldf, nseg, seg_rows, nblocks, op);
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

static int cheby_path(int64_t x0, const double* u, int64_t ld, const double* f, int64_t ldf, const double* v,
                      int64_t ldv) {
  return x0 % 2 == 0 && walk_vec_ok(u, ld) && walk_vec_ok(v, ldv) && (!f || walk_vec_ok(f, ldf))
             ? GMT_PATH_ROW_WALK
             : GMT_PATH_SCALAR;
}

template <bool HAS_F>
static int cheby_launch(bool walk, int64_t x0, int64_t nx, int64_t y0, int64_t ny, const double* u, int64_t ld,
                        const double* f, int64_t ldf, double c0, double c1, double om, double* v, int64_t ldv,
                        hipStream_t s) {
  if (walk) {
    int64_t nseg, L;
    const int64_t nb = walk_blocks(nx, ny, &nseg, &L);
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
  if (seg_rows) *seg_rows = path == GMT_PATH_ROW_WALK && nx > 0 && ny > 0 ? walk_seg_rows(nx, ny) : 0;
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
