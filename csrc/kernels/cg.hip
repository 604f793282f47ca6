// Conjugate-gradient kernels for A = I - J (J: the 2-D 5-point Laplace sweep,
// fp64), hand-written for gfx950: the three launches of one CG iteration of
// JacobiSolver::cg (gmt/kernels.h).
//
//   cg_apply_walk    q = p - c0*((W+E)+(S+N))  (mode 0, + sum p*q)  or the
//                    residual d of jacobi5_resid.hip (mode 1, + sum d^2 and
//                    max |d|), 16 B/pt: the row walk of row_walk.hpp with one
//                    16-B store per row.
//   cg_update_k      x += a*p, r -= a*q, + sum r^2 and max |r|, 48 B/pt
//   cg_dir_k         p = r + b*p, 24 B/pt
//                    both streaming kernels in the shape of add2d_pt: one 16-B
//                    column pair per lane, a block covers 512 columns of
//                    kCgRows rows (so the update's block partials stay few).
//
// a and b are computed in the kernels from device scalars (num / den, 0 unless
// den > 0), so an iteration never waits for the host.  Every cell expression
// is evaluated without contraction, as the CPU backend's.  The *_scalar forms
// (one cell per lane) take odd alignment.
//
// Stores: x is touched once per iteration and goes around the caches
// (nontemporal load and store); q, r and p are read again by the next launch
// and use plain stores.  GMT_CG_NT (bit 0 q, 1 x, 2 r, 3 p: nontemporal pair
// stores) rebuilds the file with another policy for the A/B recorded in
// profiles/cg/README.md.
#include <algorithm>

#include "common.hpp"
#include "reduce_partials.hpp"
#include "row_walk.hpp"
#include "gmt/kernels.h"

#ifndef GMT_CG_NT
#define GMT_CG_NT 2
#endif

namespace gmt {

template <int BIT>
__device__ __forceinline__ void cg_st2(double* p, d2 v) {
  if ((GMT_CG_NT >> BIT) & 1)
    st2_nt(p, v);
  else
    st2(p, v);
}

// row loads in flight per lane of the walk (with f, two: its pairs double the registers of a row)
constexpr int kCgUnrollP = 4, kCgUnrollF = 2;
constexpr int kCgRows = 4;  // rows per block of the streaming kernels

template <int MODE, bool HAS_F>
__device__ __forceinline__ double cg_cell(double w, double e, double n, double s, double c, double c0, double c1,
                                          double fv) {
#pragma clang fp contract(off)
  double o = c0 * ((w + e) + (n + s));
  if (MODE == 0) return c - o;
  if (HAS_F) o = o + c1 * fv;
  return o - c;
}

// y + a*x and y - a*x with two roundings
__device__ __forceinline__ double cg_madd(double y, double a, double x) {
#pragma clang fp contract(off)
  const double t = a * x;
  return y + t;
}
__device__ __forceinline__ double cg_msub(double y, double a, double x) {
#pragma clang fp contract(off)
  const double t = a * x;
  return y - t;
}

__device__ __forceinline__ double cg_coef(const double* num, const double* den) {
  const double n = *num, d = *den;
  return d > 0.0 ? n / d : 0.0;  // a NaN denominator compares false
}

// mode 0: sum c*v; mode 1: sum v^2 and max |v| (NaN -> +inf)
template <int MODE>
__device__ __forceinline__ void cg_acc(double c, double v, bool on, double& acc, double& m) {
  if (MODE == 0) {
    acc += on ? c * v : 0.0;
  } else {
    const double av = fabs(v);
    acc += on ? v * v : 0.0;
    m = fmax(m, on ? (v != v ? __builtin_inf() : av) : 0.0);
  }
}

// the walk's op: a row is stored to q and accumulated
template <int MODE, bool HAS_F>
struct CgApplyOp {
  double c0, c1;
  double* __restrict__ q;
  int64_t ldq;
  double* pq = nullptr;
  double acc = 0.0, m = 0.0;
  __device__ __forceinline__ void begin(int64_t row, int64_t, int64_t xr) { pq = q + row * ldq + xr; }
  __device__ __forceinline__ void load(int, int64_t) {}
  __device__ __forceinline__ void row(int j, double w, double e, d2 a, d2 b, d2 c, d2 f, bool live, bool pair) {
    d2 v;
    v.x = cg_cell<MODE, HAS_F>(w, b.y, a.x, c.x, b.x, c0, c1, f.x);
    v.y = cg_cell<MODE, HAS_F>(b.x, e, a.y, c.y, b.y, c0, c1, f.y);
    if (pair)
      cg_st2<0>(pq + j * ldq, v);
    else if (live)
      pq[j * ldq] = v.x;
    cg_acc<MODE>(b.x, v.x, live, acc, m);
    cg_acc<MODE>(b.y, v.y, pair, acc, m);
  }
  __device__ __forceinline__ void advance(int rows) { pq += rows * ldq; }
};

template <int MODE, bool HAS_F>
__global__ __launch_bounds__(kBlock) void cg_apply_walk(int64_t x0, int64_t nx, int64_t y0, int64_t ny,
                                                        const double* __restrict__ u, int64_t ld,
                                                        const double* __restrict__ f, int64_t ldf, double c0,
                                                        double c1, double* __restrict__ q, int64_t ldq,
                                                        double* __restrict__ psum, double* __restrict__ pmax,
                                                        int64_t nseg, int64_t seg_rows, int64_t nblocks) {
  constexpr int kUnroll = HAS_F ? kCgUnrollF : kCgUnrollP;
  CgApplyOp<MODE, HAS_F> op{c0, c1, q, ldq};
  row_walk<kUnroll, HAS_F>(x0, nx, y0, ny, u, ld, f, ldf, nseg, seg_rows, nblocks, op);
  write_block_partials(op.acc, op.m, psum, pmax);
}

template <int MODE, bool HAS_F>
__global__ __launch_bounds__(kBlock) void cg_apply_scalar(int64_t x0, int64_t nx, int64_t y0, int64_t ny,
                                                          const double* __restrict__ u, int64_t ld,
                                                          const double* __restrict__ f, int64_t ldf, double c0,
                                                          double c1, double* __restrict__ q, int64_t ldq,
                                                          double* __restrict__ psum, double* __restrict__ pmax) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  double acc = 0.0, m = 0.0;
  if (i < nx * ny) {
    const int64_t x = x0 + i % nx, y = y0 + i / nx;
    const double* pc = u + y * ld + x;
    const double v = cg_cell<MODE, HAS_F>(pc[-1], pc[1], pc[-ld], pc[ld], pc[0], c0, c1,
                                          HAS_F ? f[y * ldf + x] : 0.0);
    q[y * ldq + x] = v;
    cg_acc<MODE>(pc[0], v, true, acc, m);
  }
  write_block_partials(acc, m, psum, pmax);
}

// PT: the lane's column pair (a scalar last column of an odd nx); else one column per lane
template <bool PT>
__global__ __launch_bounds__(kBlock) void cg_update_k(int64_t x0, int64_t nx, int64_t y0, int64_t ny,
                                                      const double* __restrict__ num,
                                                      const double* __restrict__ den,
                                                      const double* __restrict__ p, int64_t ldp,
                                                      const double* __restrict__ q, int64_t ldq,
                                                      double* __restrict__ x, int64_t ldx, double* __restrict__ r,
                                                      int64_t ldr, double* __restrict__ psum,
                                                      double* __restrict__ pmax, unsigned nbx) {
  const unsigned bx = blockIdx.x % nbx, by = blockIdx.x / nbx;  // 32-bit: fewer than 2^31 blocks
  const double a = cg_coef(num, den);
  const int64_t xr = (static_cast<int64_t>(bx) * kBlock + threadIdx.x) * (PT ? 2 : 1);
  double acc = 0.0, m = 0.0;
  if (xr < nx) {
    const bool pair = PT && xr + 1 < nx;
#pragma unroll
    for (int j = 0; j < kCgRows; ++j) {
      const int64_t y = static_cast<int64_t>(by) * kCgRows + j;
      if (y < ny) {
        const int64_t row = y0 + y, col = x0 + xr;
        const double* pp = p + row * ldp + col;
        const double* pq = q + row * ldq + col;
        double* px = x + row * ldx + col;
        double* pr = r + row * ldr + col;
        if (pair) {
          const d2 vp = ld2(pp), vq = ld2(pq), vx = (GMT_CG_NT & 2) ? ld2_nt(px) : ld2(px), vr = ld2(pr);
          d2 nx2, nr2;
          nx2.x = cg_madd(vx.x, a, vp.x);
          nx2.y = cg_madd(vx.y, a, vp.y);
          nr2.x = cg_msub(vr.x, a, vq.x);
          nr2.y = cg_msub(vr.y, a, vq.y);
          cg_st2<1>(px, nx2);
          cg_st2<2>(pr, nr2);
          cg_acc<1>(0.0, nr2.x, true, acc, m);
          cg_acc<1>(0.0, nr2.y, true, acc, m);
        } else {
          const double nxv = cg_madd(px[0], a, pp[0]);
          const double nrv = cg_msub(pr[0], a, pq[0]);
          px[0] = nxv;
          pr[0] = nrv;
          cg_acc<1>(0.0, nrv, true, acc, m);
        }
      }
    }
  }
  write_block_partials(acc, m, psum, pmax);
}

template <bool PT>
__global__ __launch_bounds__(kBlock) void cg_dir_k(int64_t x0, int64_t nx, int64_t y0, int64_t ny,
                                                   const double* __restrict__ num, const double* __restrict__ den,
                                                   const double* __restrict__ r, int64_t ldr,
                                                   double* __restrict__ p, int64_t ldp, unsigned nbx) {
  const unsigned bx = blockIdx.x % nbx, by = blockIdx.x / nbx;
  const double b = cg_coef(num, den);
  const int64_t xr = (static_cast<int64_t>(bx) * kBlock + threadIdx.x) * (PT ? 2 : 1);
  if (xr >= nx) return;
  const bool pair = PT && xr + 1 < nx;
#pragma unroll
  for (int j = 0; j < kCgRows; ++j) {
    const int64_t y = static_cast<int64_t>(by) * kCgRows + j;
    if (y < ny) {
      const int64_t row = y0 + y, col = x0 + xr;
      const double* pr = r + row * ldr + col;
      double* pp = p + row * ldp + col;
      if (pair) {
        const d2 vr = ld2(pr), vp = ld2(pp);
        d2 np2;
        np2.x = cg_madd(vr.x, b, vp.x);
        np2.y = cg_madd(vr.y, b, vp.y);
        cg_st2<3>(pp, np2);
      } else {
        pp[0] = cg_madd(pr[0], b, pp[0]);
      }
    }
  }
}

// blocks of the streaming kernels: nbx per row group
static int64_t cg_stream_blocks(bool pt, int64_t nx, int64_t ny, int64_t* nbx) {
  const int64_t cols = pt ? 2 * kBlock : kBlock;
  *nbx = (nx + cols - 1) / cols;
  return *nbx * ((ny + kCgRows - 1) / kCgRows);
}
// the most partials any of the kernels writes for this region
static int64_t cg_max_blocks(int64_t nx, int64_t ny) {
  int64_t nseg, L, nbx;
  int64_t n = walk_blocks(nx, ny, &nseg, &L);
  n = std::max(n, (nx * ny + kBlock - 1) / kBlock);
  n = std::max(n, cg_stream_blocks(true, nx, ny, &nbx));
  n = std::max(n, cg_stream_blocks(false, nx, ny, &nbx));
  return n;
}

static int cg_apply_path(int64_t x0, const double* p, int64_t ldp, const double* f, int64_t ldf, const double* q,
                         int64_t ldq) {
  return x0 % 2 == 0 && walk_vec_ok(p, ldp) && walk_vec_ok(q, ldq) && (!f || walk_vec_ok(f, ldf))
             ? GMT_PATH_ROW_WALK
             : GMT_PATH_SCALAR;
}
static int cg_update_path(int64_t x0, const double* p, int64_t ldp, const double* q, int64_t ldq, const double* x,
                          int64_t ldx, const double* r, int64_t ldr) {
  return x0 % 2 == 0 && walk_vec_ok(p, ldp) && walk_vec_ok(q, ldq) && walk_vec_ok(x, ldx) && walk_vec_ok(r, ldr)
             ? GMT_PATH_PT
             : GMT_PATH_SCALAR;
}
static int cg_dir_path(int64_t x0, const double* r, int64_t ldr, const double* p, int64_t ldp) {
  return x0 % 2 == 0 && walk_vec_ok(r, ldr) && walk_vec_ok(p, ldp) ? GMT_PATH_PT : GMT_PATH_SCALAR;
}

template <int MODE, bool HAS_F>
static void cg_apply_launch(bool walk, int64_t x0, int64_t nx, int64_t y0, int64_t ny, const double* p,
                            int64_t ldp, const double* f, int64_t ldf, double c0, double c1, double* q,
                            int64_t ldq, double* psum, double* pmax, int64_t* nb, hipStream_t s) {
  if (walk) {
    int64_t nseg, L;
    *nb = walk_blocks(nx, ny, &nseg, &L);
    cg_apply_walk<MODE, HAS_F><<<grid_1d(*nb), kBlock, 0, s>>>(x0, nx, y0, ny, p, ldp, f, ldf, c0, c1, q, ldq, psum,
                                                               pmax, nseg, L, *nb);
  } else {
    *nb = (nx * ny + kBlock - 1) / kBlock;
    cg_apply_scalar<MODE, HAS_F><<<grid_1d(*nb), kBlock, 0, s>>>(x0, nx, y0, ny, p, ldp, f, ldf, c0, c1, q, ldq,
                                                                 psum, pmax);
  }
}

}  // namespace gmt

// workspace layout: sum partials [nbmax] | level-2 slots [kL2] | max partials [nbmax] | level-2 slots [kL2]
extern "C" int64_t gmt_cg_workspace(int64_t nx, int64_t ny) {
  using namespace gmt;
  if (nx <= 0 || ny <= 0) return 2;
  return 2 * (cg_max_blocks(nx, ny) + kL2);
}

extern "C" int gmt_cg_apply_path(int64_t x0, int64_t nx, int64_t ny, const double* p, int64_t ldp,
                                 const double* f, int64_t ldf, const double* q, int64_t ldq, int64_t* seg_rows) {
  using namespace gmt;
  const int path = cg_apply_path(x0, p, ldp, f, ldf, q, ldq);
  if (seg_rows) *seg_rows = path == GMT_PATH_ROW_WALK && nx > 0 && ny > 0 ? walk_seg_rows(nx, ny) : 0;
  return path;
}
extern "C" int gmt_cg_update_path(int64_t x0, const double* p, int64_t ldp, const double* q, int64_t ldq,
                                  const double* x, int64_t ldx, const double* r, int64_t ldr) {
  return gmt::cg_update_path(x0, p, ldp, q, ldq, x, ldx, r, ldr);
}
extern "C" int gmt_cg_dir_path(int64_t x0, const double* r, int64_t ldr, const double* p, int64_t ldp) {
  return gmt::cg_dir_path(x0, r, ldr, p, ldp);
}

extern "C" int gmt_cg_apply(int mode, int64_t x0, int64_t nx, int64_t y0, int64_t ny, const double* p,
                            int64_t ldp, const double* f, int64_t ldf, double c0, double c1, double* q,
                            int64_t ldq, double* out, double* workspace, void* stream) {
  using namespace gmt;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (!out || mode < 0 || mode > 1) return static_cast<int>(hipErrorInvalidValue);
  if (nx <= 0 || ny <= 0) return static_cast<int>(hipMemsetAsync(out, 0, 2 * sizeof(double), s));
  if (!p || !q || !workspace || x0 < 1 || y0 < 1 || ldp < x0 + nx + 1 || ldq < x0 + nx)
    return static_cast<int>(hipErrorInvalidValue);
  if (mode == 0) f = nullptr;
  if (f && ldf < x0 + nx) return static_cast<int>(hipErrorInvalidValue);
  const int64_t nbmax = cg_max_blocks(nx, ny);
  if (nbmax > INT32_MAX) return static_cast<int>(hipErrorInvalidValue);  // the grid's x extent
  double* psum = workspace;
  double* pmax = workspace + nbmax + kL2;
  const bool walk = cg_apply_path(x0, p, ldp, f, ldf, q, ldq) == GMT_PATH_ROW_WALK;
  int64_t nb = 0;
  if (mode == 0)
    cg_apply_launch<0, false>(walk, x0, nx, y0, ny, p, ldp, f, ldf, c0, c1, q, ldq, psum, pmax, &nb, s);
  else if (f)
    cg_apply_launch<1, true>(walk, x0, nx, y0, ny, p, ldp, f, ldf, c0, c1, q, ldq, psum, pmax, &nb, s);
  else
    cg_apply_launch<1, false>(walk, x0, nx, y0, ny, p, ldp, f, ldf, c0, c1, q, ldq, psum, pmax, &nb, s);
  reduce_sum_max(psum, pmax, nb, out, s);
  GMT_RET_LAUNCH();
}

extern "C" int gmt_cg_update(int64_t x0, int64_t nx, int64_t y0, int64_t ny, const double* num, const double* den,
                             const double* p, int64_t ldp, const double* q, int64_t ldq, double* x, int64_t ldx,
                             double* r, int64_t ldr, double* out, double* workspace, void* stream) {
  using namespace gmt;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (!out) return static_cast<int>(hipErrorInvalidValue);
  if (nx <= 0 || ny <= 0) return static_cast<int>(hipMemsetAsync(out, 0, 2 * sizeof(double), s));
  if (!num || !den || !p || !q || !x || !r || !workspace || x0 < 0 || y0 < 0 || ldp < x0 + nx || ldq < x0 + nx ||
      ldx < x0 + nx || ldr < x0 + nx)
    return static_cast<int>(hipErrorInvalidValue);
  const int64_t nbmax = cg_max_blocks(nx, ny);
  if (nbmax > INT32_MAX) return static_cast<int>(hipErrorInvalidValue);
  double* psum = workspace;
  double* pmax = workspace + nbmax + kL2;
  const bool pt = cg_update_path(x0, p, ldp, q, ldq, x, ldx, r, ldr) == GMT_PATH_PT;
  int64_t nbx;
  const int64_t nb = cg_stream_blocks(pt, nx, ny, &nbx);
  if (pt)
    cg_update_k<true><<<grid_1d(nb), kBlock, 0, s>>>(x0, nx, y0, ny, num, den, p, ldp, q, ldq, x, ldx, r, ldr, psum,
                                                     pmax, static_cast<unsigned>(nbx));
  else
    cg_update_k<false><<<grid_1d(nb), kBlock, 0, s>>>(x0, nx, y0, ny, num, den, p, ldp, q, ldq, x, ldx, r, ldr, psum,
                                                      pmax, static_cast<unsigned>(nbx));
  reduce_sum_max(psum, pmax, nb, out, s);
  GMT_RET_LAUNCH();
}

extern "C" int gmt_cg_dir(int64_t x0, int64_t nx, int64_t y0, int64_t ny, const double* num, const double* den,
                          const double* r, int64_t ldr, double* p, int64_t ldp, void* stream) {
  using namespace gmt;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (nx <= 0 || ny <= 0) return 0;
  if (!num || !den || !r || !p || x0 < 0 || y0 < 0 || ldr < x0 + nx || ldp < x0 + nx)
    return static_cast<int>(hipErrorInvalidValue);
  const bool pt = cg_dir_path(x0, r, ldr, p, ldp) == GMT_PATH_PT;
  int64_t nbx;
  const int64_t nb = cg_stream_blocks(pt, nx, ny, &nbx);
  if (nb > INT32_MAX) return static_cast<int>(hipErrorInvalidValue);
  if (pt)
    cg_dir_k<true><<<grid_1d(nb), kBlock, 0, s>>>(x0, nx, y0, ny, num, den, r, ldr, p, ldp,
                                                  static_cast<unsigned>(nbx));
  else
    cg_dir_k<false><<<grid_1d(nb), kBlock, 0, s>>>(x0, nx, y0, ny, num, den, r, ldr, p, ldp,
                                                   static_cast<unsigned>(nbx));
  GMT_RET_LAUNCH();
}
