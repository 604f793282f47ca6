// The kernels of one geometric multigrid V-cycle over the Jacobi sweep
// (JacobiSolver::mg, gmt/kernels.h), fp64, hand-written for gfx950: the damped
// Jacobi smoother and the two grid transfers between a vertex-centred level
// and the next coarser one (coarse point (J, I) on fine point (2J+1, 2I+1)).
//
//   mg_smooth_walk      out = u + omega*(G(u) - u): the row walk of
//                       row_walk.hpp over u; the centre pair is the walk's own
//                       row b, so a row adds one 16-B store and nothing else:
//                       16 B/pt (24 with f).
//   mg_smooth_k_walk    k of those sweeps in one pass (gmt_mg_smooth_k): the walk
//                       with k levels in registers, described where it is
//                       defined below; still 16 B/pt (24 with f).
//   mg_restrict_pt      full weighting: one lane per pair of coarse cells, the
//                       five fine columns of a row by two 16-B loads and one
//                       8-B load, one 16-B store.  Neighbouring lanes and rows
//                       re-read fine cells out of L2: the DPP row walk the
//                       smoother has is not built for it yet.
//   mg_prolong_pt       bilinear interpolation added in place: one lane per
//                       fine pair, a 16-B read-modify-write of u, the coarse
//                       cells by 8-B loads (L2 hits: four fine cells share them).
//   mg_restrict_tab_pt  the transpose of linear interpolation between levels
//   mg_prolong_tab_pt   that are not nested (any point count on the same
//                       interval): the same 16-B stores and read-modify-write,
//                       with the coarse cell and weight of a fine column / row,
//                       and the 3 or 4 taps and weights of a coarse one, from
//                       device tables that the host built and checked
//                       (gmt/mg_tab.hpp); taps by 8-B loads out of L2.  The
//                       restriction computes one coarse cell per lane and pairs
//                       the lanes for the store.
//   mg_resid_restrict_* the residual and its full weighting in one pass
//                       (gmt_mg_resid_restrict), described where they are
//                       defined below: 8 + 2 B/pt (16 + 2 with f).
//   mg_smooth_k_* <PR>  the interpolation inside the fused smoother
//                       (gmt_mg_prolong_smooth): the same two kernels with a
//                       level-0 transform u + P e, described at MgProWalk
//                       below: 16 + 2 B/pt (24 + 2 with f).
//   *_scalar            one cell per lane, for odd alignment or pitches.
//
// Every cell is evaluated without contraction, as the CPU backend's.
#include <cstring>
#include <new>
#include <type_traits>
#include <vector>

#include "common.hpp"
#include "row_walk.hpp"
#include "gmt/kernels.h"
#include "gmt/mg_args.hpp"
#include "gmt/mg_tab.hpp"

namespace gmt {

// row loads in flight per lane (as the Chebyshev step's)
constexpr int kMgUnrollP = 4, kMgUnrollF = 2;

constexpr int kMgRefuse = static_cast<int>(hipErrorInvalidValue);  // what a refused check (gmt/mg_args.hpp) returns

// the grid of a kernel with one lane per cell or per pair; false past the grid's x extent
static bool mg_lane_grid(int64_t lanes, unsigned* grid) {
  const int64_t nb = (lanes + kBlock - 1) / kBlock;
  *grid = grid_1d(nb);
  return nb <= INT32_MAX;
}

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
    if (nb > INT32_MAX) return kMgRefuse;  // the grid's x extent
    mg_smooth_walk<HAS_F><<<grid_1d(nb), kBlock, 0, s>>>(x0, nx, y0, ny, u, ld, f, ldf, c0, c1, om, out, ldo, nseg, L,
                                                         nb);
  } else {
    unsigned grid;
    if (!mg_lane_grid(nx * ny, &grid)) return kMgRefuse;
    mg_smooth_scalar<HAS_F><<<grid, kBlock, 0, s>>>(x0, nx, y0, ny, u, ld, f, ldf, c0, c1, om, out, ldo);
  }
  GMT_RET_LAUNCH();
}

// ---- k fused sweeps of the smoother (gmt_mg_smooth_k, gmt/kernels.h) ----
//
//   mg_smooth_k_walk    the row walk with K levels in registers.  Level 0 is u;
//                       level l + 1 lags level l by one row and keeps the two
//                       last rows of level l as lane pairs (the third is the
//                       row that just arrived), so one new row of u pushes one
//                       row through every level and one row of level K to out.
//                       W/E neighbours of every level come through DPP, so a
//                       wave's valid columns shrink by one per level and side:
//                       a wave stores kWalkWaveCols - 2*SH columns, SH = K - 1
//                       rounded up to even (stores stay 16-B aligned), and
//                       loads SH columns around them; a segment runs K rows
//                       above and below its own.  Whether a cell is updated or
//                       kept at a level (the boxes B_j) is a scalar test on
//                       the row and a lane mask fixed for the walk: a select.
//                       The outermost column of u's read set, where it is half
//                       of a pair, comes by the walk's one-lane load, and is
//                       that lane's W or E neighbour at every level: the cell
//                       is never updated.
//   mg_smooth_k_scalar  one lane per output cell: the cells of its dependence
//                       cone (|dx| + |dy| <= K - j at level j) level by level
//                       in registers, with the same cell and keep rule.
//   red-black (gmt_mg_smooth_rb): the same two kernels with RB set and K = h
//                       half-sweeps, K = 1 included.  Level l + 1 updates only
//                       the cells that are due in half-sweep l + 1; in the walk
//                       that is one scalar per arriving row (see there), folded
//                       into the select, so the pass stays at 16 B/pt.  Both
//                       cells of a pair are evaluated and one is discarded:
//                       evaluating the due cell alone, operands by selects,
//                       measured the same (profiles/mg_rb).

// the shortest segment: 4k rows rounded up to a power of two, so the 2k warm-up
// rows stay at half the segment or below.  Small levels want short segments:
// a wave walks its rows one after another, and with 32-row segments the
// levels from 4095² down took longer fused than sweep by sweep.
constexpr int64_t mg_fuse_min_seg(int k) { return k <= 2 ? 8 : 16; }

// mg_fuse_shift and mg_fuse_wave_cols: gmt/mg_args.hpp, which the CPU backend reports the geometry from
static_assert(kMgWaveCols == kWalkWaveCols && kMgBlockWaves == kBlock / kWave, "gmt/mg_args.hpp: the walk's geometry");

struct MgFuseArgs {
  int64_t x0, nx, y0, ny;
  int mask;
  const double* u;
  int64_t ld;
  const double* f;
  int64_t ldf;
  double c0, c1, om;
  double* out;
  int64_t ldo;
  int64_t nseg, seg_rows, nblocks;
  int par;  // red-black only: the colour phase of cell (x0, y0)
};

// gmt_mg_prolong_smooth: the coarse field behind the level-0 transform u + P e
struct MgProArgs : MgFuseArgs {
  const double* e;  // at coarse cell (0, 0) of the region
  int64_t lde;
  int px, py;
  int64_t ilo, ihi, jlo, jhi;  // the coarse columns and rows that may be read, region-relative, inclusive
};
template <bool PR>
using MgWalkArgs = std::conditional_t<PR, MgProArgs, MgFuseArgs>;

__device__ __forceinline__ int64_t mg_clamp(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The level-0 transform of gmt_mg_prolong_smooth in the walk.  A lane loads coarse cell I = c >> 1 of a coarse
// row (8 B per lane, coalesced) and takes cells I - 1 and I + 1 from its neighbours through DPP; the first and
// last lane of the read set load theirs.  A new coarse row arrives with every second fine row: a fine row on a
// coarse row J uses q(J), the row between J and J + 1 uses q(J) + q(J + 1), in mg_prolong_cell's order.
template <bool PR>
struct MgProWalk {};
template <>
struct MgProWalk<true> {
  const double* eb;  // coarse row 0 at the lane's clamped column
  int64_t iw, ie;    // the offsets of columns I - 1 and I + 1 from it (clamped)
  bool west, east, px, py;
  bool m[4];      // fine columns c - 1, c, c + 1, c + 2: inside B0's columns
  double fc[4];   // 1 on a coarse column, 0.5 between two
  double q[4];    // of the coarse row at or below the fine row that arrives next
  __device__ __forceinline__ void rowq(double v, double vw, double ve, double o[4]) const {
#pragma clang fp contract(off)
    const double dl = dpp_from_lower(v), du = dpp_from_upper(v);  // by every lane, before the selects
    const double lw = west ? vw : dl, le = east ? ve : du;
    // px = 0: c - 1 between I - 1 and I, c on I, c + 1 between I and I + 1, c + 2 on I + 1
    // px = 1: c - 1 on I - 1, c between I - 1 and I, c + 1 on I, c + 2 between I and I + 1
    const double sw = lw + v, se = v + le;
    o[0] = px ? lw : sw;
    o[1] = px ? sw : v;
    o[2] = px ? v : se;
    o[3] = px ? se : le;
  }
  __device__ __forceinline__ void ldrow(const MgProArgs& a, int64_t J, double& v, double& vw, double& ve) const {
    const double* p = eb + mg_clamp(J, a.jlo, a.jhi) * a.lde;
    v = p[0];
    vw = ve = 0.0;
    if (west) vw = p[iw];
    if (east) ve = p[ie];
  }
  // c: the lane's pair; w, e: it takes its W / E operands by loads of its own; [bl, bh): B0's columns;
  // t0: the first fine row of the walk
  __device__ __forceinline__ void init(const MgProArgs& a, int64_t c, bool w, bool e, int64_t bl, int64_t bh,
                                       int64_t t0) {
    west = w, east = e, px = a.px != 0, py = a.py != 0;
    const int64_t I = c >> 1, Ic = mg_clamp(I, a.ilo, a.ihi);  // lanes outside re-read a cell inside (never used)
    eb = a.e + Ic;
    iw = mg_clamp(I - 1, a.ilo, a.ihi) - Ic;
    ie = mg_clamp(I + 1, a.ilo, a.ihi) - Ic;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int64_t x = c - 1 + k;
      m[k] = x >= bl && x < bh;
      fc[k] = ((x - a.px) & 1) == 0 ? 1.0 : 0.5;
    }
    double v, vw, ve;
    ldrow(a, (t0 - a.py) >> 1, v, vw, ve);  // the coarse row at or below the first fine row
    rowq(v, vw, ve, q);
  }
  // the coarse row above fine row t, when t lies between two
  __device__ __forceinline__ void load(const MgProArgs& a, int64_t t, double& v, double& vw, double& ve) const {
    v = vw = ve = 0.0;
    if ((t - a.py) & 1) ldrow(a, ((t - a.py) >> 1) + 1, v, vw, ve);
  }
  __device__ __forceinline__ void row(int64_t t, bool rok, double v, double vw, double ve, d2& C, double& wn,
                                      double& en) {
#pragma clang fp contract(off)
    const bool btw = ((t - py) & 1) != 0;  // wave-uniform
    double qn[4] = {0.0, 0.0, 0.0, 0.0}, tq[4];
    if (btw) rowq(v, vw, ve, qn);  // every lane of the wave or none: DPP
    const double fr = btw ? 0.5 : 1.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double s2 = q[k] + qn[k];
      const double s = btw ? s2 : q[k];
      const double fk = fc[k] * fr;  // 1, 0.5 or 0.25: exact
      tq[k] = fk * s;
      q[k] = btw ? qn[k] : q[k];
    }
    const double cw = wn + tq[0], cx = C.x + tq[1], cy = C.y + tq[2], ce = en + tq[3];
    wn = rok && m[0] ? cw : wn;
    C.x = rok && m[1] ? cx : C.x;
    C.y = rok && m[2] ? cy : C.y;
    en = rok && m[3] ? ce : en;
  }
};

template <int K, bool HAS_F, bool RB = false, bool PR = false>
__global__ __launch_bounds__(kBlock) void mg_smooth_k_walk(const MgWalkArgs<PR> a) {
  constexpr int SH = mg_fuse_shift(K), OC = mg_fuse_wave_cols(K);
  constexpr int U = HAS_F ? kMgUnrollF : kMgUnrollP;
  const double* __restrict__ u = a.u;
  const double* __restrict__ f = a.f;
  double* __restrict__ out = a.out;
  const int64_t nx = a.nx, ny = a.ny, ld = a.ld, ldf = a.ldf;
  const int64_t t = xcd_swizzle(blockIdx.x, a.nblocks);
  const int64_t seg = t % a.nseg, bx = t / a.nseg;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int64_t xo = (bx * (kBlock / kWave) + wave) * OC;  // the wave's first output column
  if (xo >= nx) return;  // wave-uniform: every lane of a working wave stays active (DPP)
  const int64_t xe = xo + OC < nx ? xo + OC : nx;
  const bool hw = a.mask & GMT_MG_HALO_W, he = a.mask & GMT_MG_HALO_E, hs = a.mask & GMT_MG_HALO_S,
             hn = a.mask & GMT_MG_HALO_N;
  // region-relative columns: the lane's own pair, u's read set [lo, hi), its first and last whole pair
  const int64_t c = xo - SH + 2 * lane;
  const int64_t lo = hw ? -K : -1, hi = nx + (he ? K : 1);
  const int64_t lop = lo + (lo & 1), hip = (hi - 2) & ~int64_t(1);
  const int64_t cl = mg_clamp(c, lop, hip);  // lanes outside re-read a pair inside (never used)
  const bool west = lane == 0 || c == lop, east = lane == kWave - 1 || c == hip;
  const bool wld = west && c - 1 >= lo && c - 1 < hi, eld = east && c + 2 >= lo && c + 2 < hi;
  // updated at level l + 1 or kept: the column masks of the lane's two cells
  bool mx[K], my[K];
#pragma unroll
  for (int l = 0; l < K; ++l) {
    const int64_t bl = hw ? -(K - 1 - l) : 0, bh = nx + (he ? K - 1 - l : 0);
    mx[l] = c >= bl && c < bh;
    my[l] = c + 1 >= bl && c + 1 < bh;
  }
  // f's read set: a lane loads a whole pair, one cell of it, or nothing
  const int64_t flo = hw ? -(K - 1) : 0, fhi = nx + (he ? K - 1 : 0);
  const bool fxo = HAS_F && c >= flo && c < fhi, fyo = HAS_F && c + 1 >= flo && c + 1 < fhi;
  const bool sp = c >= xo && c + 1 < xe, s1 = c >= xo && c < xe && !sp;
  const int64_t r0 = seg * a.seg_rows;
  const int64_t r1 = r0 + a.seg_rows < ny ? r0 + a.seg_rows : ny;
  const int64_t rlo = hs ? -K : -1, rhi = ny - 1 + (hn ? K : 1);             // u's rows
  const int64_t frlo = hs ? -(K - 1) : 0, frhi = ny - 1 + (hn ? K - 1 : 0);  // f's rows
  const double* ub = u + a.y0 * ld + a.x0;
  const double* fb = HAS_F ? f + a.y0 * ldf + a.x0 : nullptr;
  double* ob = out + a.y0 * a.ldo + a.x0 + c;
  d2 A[K], B[K], fh[K];
  double wh[K], eh[K];
#pragma unroll
  for (int l = 0; l < K; ++l) {
    A[l] = B[l] = fh[l] = d2{0.0, 0.0};
    wh[l] = eh[l] = 0.0;
  }
  // PR: the lane's coarse column sits on fine column c + px of its pair, the other cell of the pair lies between
  // it and the column of the W (px = 1) or E (px = 0) lane.  The four fine columns c - 1 .. c + 2 (the pair and the
  // two one-lane loads): corrected or not, and q = what a coarse row gives them (its cell, or the sum of two).
  MgProWalk<PR> pw;
  if constexpr (PR) pw.init(a, c, west, east, hw ? -int64_t(K) : 0, nx + (he ? K : 0), r0 - K);
  for (int64_t tt = r0 - K; tt < r1 + K; tt += U) {
    d2 cn[U], fn[U];
    double wn[U], en[U];
    [[maybe_unused]] double ec[U], ew[U], ee[U];
#pragma unroll
    for (int j = 0; j < U; ++j) {
      // rows past the read set are clamped to its last ones (loaded, not used)
      const double* p = ub + mg_clamp(tt + j, rlo, rhi) * ld;
      cn[j] = ld2(p + cl);
      wn[j] = en[j] = 0.0;
      if (wld) wn[j] = p[c - 1];
      if (eld) en[j] = p[c + 2];
      fn[j] = d2{0.0, 0.0};
      if (HAS_F) {  // the row level 1 computes when row tt + j arrives
        const double* pf = fb + mg_clamp(tt + j - 1, frlo, frhi) * ldf;
        if (fxo && fyo) {
          fn[j] = ld2(pf + c);
        } else {
          if (fxo) fn[j].x = pf[c];
          if (fyo) fn[j].y = pf[c + 1];
        }
      }
      if constexpr (PR) pw.load(a, tt + j, ec[j], ew[j], ee[j]);
    }
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const int64_t tr = tt + j;  // the row of u that arrives; level l + 1 computes row tr - 1 - l
      if (HAS_F) {
#pragma unroll
        for (int l = K - 1; l > 0; --l) fh[l] = fh[l - 1];
        fh[0] = fn[j];
      }
      d2 C = cn[j];
      if constexpr (PR)  // level 0 becomes u + P e on B0
        pw.row(tr, tr >= (hs ? -int64_t(K) : 0) && tr < ny + (hn ? K : 0), ec[j], ew[j], ee[j], C, wn[j], en[j]);
      // red-black: level l + 1 is half-sweep l + 1 on row tr - 1 - l, and the lane's pair starts on an even
      // column, so which cell of the pair is due is one scalar for the row that arrives, the same at every level
      const bool duex = !RB || ((tr - 1 + a.par) & 1) == 0, duey = !RB || !duex;
#pragma unroll
      for (int l = 0; l < K; ++l) {
        const int64_t y = tr - 1 - l;
        const bool rok = y >= (hs ? -(K - 1 - l) : 0) && y < ny + (hn ? K - 1 - l : 0);
        const d2 b = B[l];
        const double wl = dpp_from_lower(b.y), eu = dpp_from_upper(b.x);
        const double w = west ? wh[l] : wl, e = east ? eh[l] : eu;
        d2 n;
        n.x = mg_smooth_cell<HAS_F>(w, b.y, A[l].x, C.x, b.x, a.c0, a.c1, fh[l].x, a.om);
        n.y = mg_smooth_cell<HAS_F>(b.x, e, A[l].y, C.y, b.y, a.c0, a.c1, fh[l].y, a.om);
        n.x = rok && duex && mx[l] ? n.x : b.x;
        n.y = rok && duey && my[l] ? n.y : b.y;
        A[l] = b;
        B[l] = C;
        C = n;
      }
#pragma unroll
      for (int l = K - 1; l > 0; --l) wh[l] = wh[l - 1], eh[l] = eh[l - 1];
      wh[0] = wn[j], eh[0] = en[j];
      const int64_t yo = tr - K;  // the row of level K that came out
      if (yo >= r0 && yo < r1) {
        if (sp)
          st2(ob + yo * a.ldo, C);
        else if (s1)
          ob[yo * a.ldo] = C.x;
      }
    }
  }
}

__device__ __forceinline__ double mg_prolong_cell(const double* __restrict__ e, int64_t lde, int64_t i, int64_t j,
                                                  int px, int py, double u);

template <int K, bool HAS_F, bool RB = false, bool PR = false>
__global__ __launch_bounds__(kBlock) void mg_smooth_k_scalar(const MgWalkArgs<PR> a) {
  const double* __restrict__ u = a.u;
  const double* __restrict__ f = a.f;
  const int64_t nx = a.nx, ny = a.ny;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= nx * ny) return;
  const int64_t x = i % nx, y = i / nx;  // region-relative
  const bool hw = a.mask & GMT_MG_HALO_W, he = a.mask & GMT_MG_HALO_E, hs = a.mask & GMT_MG_HALO_S,
             hn = a.mask & GMT_MG_HALO_N;
  const double* ub = u + a.y0 * a.ld + a.x0;
  const double* fb = HAS_F ? f + a.y0 * a.ldf + a.x0 : nullptr;
  double v[2 * K + 1][2 * K + 1], n[2 * K + 1][2 * K + 1];  // indices are constants once unrolled: registers
  const int64_t lo = hw ? -K : -1, hi = nx + (he ? K : 1), rlo = hs ? -K : -1, rhi = ny + (hn ? K : 1);
#pragma unroll
  for (int dy = -K; dy <= K; ++dy)
#pragma unroll
    for (int dx = -K; dx <= K; ++dx)
      if ((dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy) <= K) {
        const int64_t X = x + dx, Y = y + dy;
        const bool in = X >= lo && X < hi && Y >= rlo && Y < rhi;
        double c = in ? ub[Y * a.ld + X] : 0.0;
        if constexpr (PR) {  // u + P e on B0
          if (X >= (hw ? -int64_t(K) : 0) && X < nx + (he ? K : 0) && Y >= (hs ? -int64_t(K) : 0) &&
              Y < ny + (hn ? K : 0))
            c = mg_prolong_cell(a.e, a.lde, X, Y, a.px, a.py, c);
        }
        v[dy + K][dx + K] = c;
      }
#pragma unroll
  for (int j = 1; j <= K; ++j) {
    const int64_t bxl = hw ? -(K - j) : 0, bxh = nx + (he ? K - j : 0);
    const int64_t byl = hs ? -(K - j) : 0, byh = ny + (hn ? K - j : 0);
#pragma unroll
    for (int dy = -K; dy <= K; ++dy)
#pragma unroll
      for (int dx = -K; dx <= K; ++dx)
        if ((dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy) <= K - j) {
          const int64_t X = x + dx, Y = y + dy;
          const double cv = v[dy + K][dx + K];
          double r = cv;
          const bool due = !RB || ((X + Y + a.par + (j - 1)) & 1) == 0;  // two's complement: the mathematical mod
          if (due && X >= bxl && X < bxh && Y >= byl && Y < byh)
            r = mg_smooth_cell<HAS_F>(v[dy + K][dx + K - 1], v[dy + K][dx + K + 1], v[dy + K - 1][dx + K],
                                      v[dy + K + 1][dx + K], cv, a.c0, a.c1, HAS_F ? fb[Y * a.ldf + X] : 0.0, a.om);
          n[dy + K][dx + K] = r;
        }
#pragma unroll
    for (int dy = -K; dy <= K; ++dy)
#pragma unroll
      for (int dx = -K; dx <= K; ++dx)
        if ((dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy) <= K - j) v[dy + K][dx + K] = n[dy + K][dx + K];
  }
  a.out[(a.y0 + y) * a.ldo + a.x0 + x] = v[K][K];
}

// rows per segment of the fused walk: the row walk's rule with its own floor
static int64_t mg_fuse_seg_rows(int k, int64_t nx, int64_t ny) {
  const int64_t nbx = (nx + mg_fuse_block_cols(k) - 1) / mg_fuse_block_cols(k);
  int64_t L = kWalkMaxSeg;
  while (L > mg_fuse_min_seg(k) && nbx * ((ny + L - 1) / L) < 8 * static_cast<int64_t>(walk_cus())) L /= 2;
  return L;
}

// the grid of a fused walk of depth k over a's region, into a; false past the grid's x extent
template <class Args>
static bool mg_fuse_grid(int k, Args* a) {
  a->seg_rows = mg_fuse_seg_rows(k, a->nx, a->ny);
  a->nseg = (a->ny + a->seg_rows - 1) / a->seg_rows;
  a->nblocks = (a->nx + mg_fuse_block_cols(k) - 1) / mg_fuse_block_cols(k) * a->nseg;
  return a->nblocks <= INT32_MAX;
}

// what a _path call reports once its path is decided: the segment rows of the walk of depth k, 0 off the walk
static int mg_fuse_path(int path, int k, int64_t nx, int64_t ny, int64_t* seg_rows) {
  if (seg_rows) *seg_rows = path == GMT_PATH_ROW_WALK && nx > 0 && ny > 0 ? mg_fuse_seg_rows(k, nx, ny) : 0;
  return path;
}

template <int K, bool HAS_F, bool RB, bool PR>
static int mg_smooth_k_launch(bool walk, MgWalkArgs<PR> a, hipStream_t s) {
  if (walk) {
    if (!mg_fuse_grid(K, &a)) return kMgRefuse;
    mg_smooth_k_walk<K, HAS_F, RB, PR><<<grid_1d(a.nblocks), kBlock, 0, s>>>(a);
  } else {
    unsigned grid;
    if (!mg_lane_grid(a.nx * a.ny, &grid)) return kMgRefuse;
    mg_smooth_k_scalar<K, HAS_F, RB, PR><<<grid, kBlock, 0, s>>>(a);
  }
  GMT_RET_LAUNCH();
}

template <int K, bool RB, bool PR>
static int mg_smooth_k_launch_f(bool walk, const MgWalkArgs<PR>& a, hipStream_t s) {
  return a.f ? mg_smooth_k_launch<K, true, RB, PR>(walk, a, s) : mg_smooth_k_launch<K, false, RB, PR>(walk, a, s);
}

// k sweeps (RB: half-sweeps; PR: behind the interpolation) on the walk or one lane per cell.  Plain k = 1 is
// gmt_mg_smooth's kernel and is not compiled here.
template <bool RB, bool PR>
static int mg_smooth_k_run(int k, const MgWalkArgs<PR>& a, hipStream_t s) {
  static_assert(GMT_MG_MAX_FUSE == 4, "one case per depth");
  const bool walk = mg_smooth_path(a.x0, a.u, a.ld, a.f, a.ldf, a.out, a.ldo) == GMT_PATH_ROW_WALK;
  switch (k) {
    case 1:
      if constexpr (RB || PR) return mg_smooth_k_launch_f<1, RB, PR>(walk, a, s);  // one level: 16 B per point
      return kMgRefuse;
    case 2: return mg_smooth_k_launch_f<2, RB, PR>(walk, a, s);
    case 3: return mg_smooth_k_launch_f<3, RB, PR>(walk, a, s);
    default: return mg_smooth_k_launch_f<4, RB, PR>(walk, a, s);
  }
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
  const int64_t di = i - px, dj = j - py;  // >= -1 on a region; below that on the halo cells of gmt_mg_prolong_smooth
  const bool onx = (di & 1) == 0, ony = (dj & 1) == 0;
  // the coarse column / row the cell sits on, else the one west / south of it (-1: the ring); both divisions are exact
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

// ---- the residual and its full weighting in one pass (gmt_mg_resid_restrict) ----
//
//   mg_resid_restrict_walk    the two-level walk of mg_smooth_k_walk<2> in its
//                       geometry (a wave stores the coarse cells of 124 fine
//                       columns and loads 2 columns around them; a segment
//                       runs 2 warm-up rows above and below its own).  Level 1
//                       is the residual cell d, +0.0 where the smoother would
//                       keep; level 2 is H of the lane's coarse column (fine
//                       column c + px of its pair at c), the third operand
//                       from the W or E lane by DPP.  The lane keeps H of the
//                       last two fine rows; every second row it stores one
//                       coarse cell, so a wave's store is 62 consecutive
//                       doubles.  8 B/pt (16 with f) read, 2 B/pt written.
//   mg_resid_restrict_scalar  one lane per coarse cell: its own 3 x 3 residuals
//                       from the 5 x 5 cells of u without the corners.

struct MgRrArgs {
  int64_t x0, nx, y0, ny;
  int px, py, mask;
  const double* u;
  int64_t ld;
  const double* f;
  int64_t ldf;
  double c0, c1, cs;
  double* sc;
  int64_t cx0, cy0, ldc, mx, my;
  int64_t nseg, seg_rows, nblocks;
};

template <bool HAS_F>
__device__ __forceinline__ double mg_resid_cell(double w, double e, double n, double s, double u, double c0,
                                                double c1, double fv) {
#pragma clang fp contract(off)
  double o = c0 * ((w + e) + (n + s));
  if (HAS_F) o = o + c1 * fv;
  return o - u;
}

template <bool HAS_F>
__global__ __launch_bounds__(kBlock) void mg_resid_restrict_walk(const MgRrArgs a) {
  constexpr int K = 2, SH = mg_fuse_shift(K), OC = mg_fuse_wave_cols(K);
  constexpr int U = HAS_F ? kMgUnrollF : kMgUnrollP;
  const double* __restrict__ u = a.u;
  const double* __restrict__ f = a.f;
  double* __restrict__ sc = a.sc;
  const int64_t nx = a.nx, ny = a.ny, ld = a.ld, ldf = a.ldf;
  const int64_t t = xcd_swizzle(blockIdx.x, a.nblocks);
  const int64_t seg = t % a.nseg, bx = t / a.nseg;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int64_t xo = (bx * (kBlock / kWave) + wave) * OC;  // the first fine column of the wave's coarse cells
  if (xo >= nx) return;  // wave-uniform: every lane of a working wave stays active (DPP)
  const bool hw = a.mask & GMT_MG_HALO_W, he = a.mask & GMT_MG_HALO_E, hs = a.mask & GMT_MG_HALO_S,
             hn = a.mask & GMT_MG_HALO_N;
  const bool px = a.px != 0;
  // region-relative columns, as mg_smooth_k_walk<2>: the lane's pair, u's read set [lo, hi), its whole pairs
  const int64_t c = xo - SH + 2 * lane;
  const int64_t lo = hw ? -K : -1, hi = nx + (he ? K : 1);
  const int64_t lop = lo + (lo & 1), hip = (hi - 2) & ~int64_t(1);
  const int64_t cl = mg_clamp(c, lop, hip);  // lanes outside re-read a pair inside (never used)
  const bool west = lane == 0 || c == lop, east = lane == kWave - 1 || c == hip;
  const bool wld = west && c - 1 >= lo && c - 1 < hi, eld = east && c + 2 >= lo && c + 2 < hi;
  // d is computed on the region grown by one cell on halo sides and is +0.0 on the rest of the ring
  const int64_t bl = hw ? -1 : 0, bh = nx + (he ? 1 : 0);
  const bool dx = c >= bl && c < bh, dy = c + 1 >= bl && c + 1 < bh;
  const bool fxo = HAS_F && dx, fyo = HAS_F && dy;  // f's read set is d's box
  // the lane's coarse column I sits on fine column c + px
  const int64_t I = c >> 1;
  const bool so = c >= xo && c < xo + OC && I < a.mx;
  const int64_t r0 = seg * a.seg_rows;
  const int64_t r1 = r0 + a.seg_rows < ny ? r0 + a.seg_rows : ny;
  const int64_t rlo = hs ? -K : -1, rhi = ny - 1 + (hn ? K : 1);  // u's rows
  const int64_t dlo = hs ? -1 : 0, dhi = ny + (hn ? 1 : 0);       // d's rows [dlo, dhi), f's too
  const double* ub = u + a.y0 * ld + a.x0;
  const double* fb = HAS_F ? f + a.y0 * ldf + a.x0 : nullptr;
  double* ob = sc + a.cy0 * a.ldc + a.cx0 + I;
  d2 A{0.0, 0.0}, B{0.0, 0.0};  // the two last rows of u
  double wB = 0.0, eB = 0.0;    // the columns beside B's pair that no lane of the wave holds
  double Hs = 0.0, Hc = 0.0;    // H of the two last rows of d
  for (int64_t tt = r0 - K; tt < r1 + K; tt += U) {
    d2 cn[U], fn[U];
    double wn[U], en[U];
#pragma unroll
    for (int j = 0; j < U; ++j) {
      // rows past the read set are clamped to its last ones (loaded, not used)
      const double* p = ub + mg_clamp(tt + j, rlo, rhi) * ld;
      cn[j] = ld2(p + cl);
      wn[j] = en[j] = 0.0;
      if (wld) wn[j] = p[c - 1];
      if (eld) en[j] = p[c + 2];
      fn[j] = d2{0.0, 0.0};
      if (HAS_F) {  // the row of d that is computed when row tt + j arrives
        const double* pf = fb + mg_clamp(tt + j - 1, dlo, dhi - 1) * ldf;
        if (fxo && fyo) {
          fn[j] = ld2(pf + c);
        } else {
          if (fxo) fn[j].x = pf[c];
          if (fyo) fn[j].y = pf[c + 1];
        }
      }
    }
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const int64_t y = tt + j - 1;  // row tt + j of u arrives: row y of d, then H(y)
      const bool rok = y >= dlo && y < dhi;
      const d2 C = cn[j];
      const double wl = dpp_from_lower(B.y), eu = dpp_from_upper(B.x);
      const double w = west ? wB : wl, e = east ? eB : eu;
      d2 d;
      d.x = mg_resid_cell<HAS_F>(w, B.y, A.x, C.x, B.x, a.c0, a.c1, fn[j].x);
      d.y = mg_resid_cell<HAS_F>(B.x, e, A.y, C.y, B.y, a.c0, a.c1, fn[j].y);
      d.x = rok && dx ? d.x : 0.0;
      d.y = rok && dy ? d.y : 0.0;
      A = B;
      B = C;
      wB = wn[j], eB = en[j];
      // beyond the read set's first and last pair lies the ring of a fixed side, or nothing that is needed
      const double dwl = dpp_from_lower(d.y), deu = dpp_from_upper(d.x);
      const double dw = west ? 0.0 : dwl, de = east ? 0.0 : deu;
      const double h = mg_h(px ? d.x : dw, px ? d.y : d.x, px ? de : d.y);
      const int64_t yc = y - 1;  // the coarse row centred here has all three rows of H now
      if (((yc - a.py) & 1) == 0 && yc >= r0 && yc < r1 && so)
        ob[((yc - a.py) >> 1) * a.ldc] = mg_full_weight(Hs, Hc, h, a.cs);
      Hs = Hc;
      Hc = h;
    }
  }
}

template <bool HAS_F>
__global__ __launch_bounds__(kBlock) void mg_resid_restrict_scalar(const MgRrArgs a) {
  const double* __restrict__ u = a.u;
  const double* __restrict__ f = a.f;
  const int64_t nx = a.nx, ny = a.ny;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= a.mx * a.my) return;
  const int64_t I = i % a.mx, J = i / a.mx;
  const int64_t x = a.px + 2 * I, y = a.py + 2 * J;  // region-relative centre
  const bool hw = a.mask & GMT_MG_HALO_W, he = a.mask & GMT_MG_HALO_E, hs = a.mask & GMT_MG_HALO_S,
             hn = a.mask & GMT_MG_HALO_N;
  const int64_t bxl = hw ? -1 : 0, bxh = nx + (he ? 1 : 0), byl = hs ? -1 : 0, byh = ny + (hn ? 1 : 0);  // d's box
  const double* ub = u + a.y0 * a.ld + a.x0;
  const double* fb = HAS_F ? f + a.y0 * a.ldf + a.x0 : nullptr;
  double v[5][5], d[3][3];  // indices are constants once unrolled: registers
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy)
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx)
      if ((dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy) <= 3) {
        // a cell of u is read iff a cell of d's box beside it needs it
        const int64_t X = x + dx, Y = y + dy;
        const bool colin = X >= bxl && X < bxh, rowin = Y >= byl && Y < byh;
        const bool need = (colin && Y >= byl - 1 && Y <= byh) || (rowin && X >= bxl - 1 && X <= bxh);
        v[dy + 2][dx + 2] = need ? ub[Y * a.ld + X] : 0.0;
      }
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      const int64_t X = x + dx, Y = y + dy;
      double r = 0.0;
      if (X >= bxl && X < bxh && Y >= byl && Y < byh)
        r = mg_resid_cell<HAS_F>(v[dy + 2][dx + 1], v[dy + 2][dx + 3], v[dy + 1][dx + 2], v[dy + 3][dx + 2],
                                 v[dy + 2][dx + 2], a.c0, a.c1, HAS_F ? fb[Y * a.ldf + X] : 0.0);
      d[dy + 1][dx + 1] = r;
    }
  const double h0 = mg_h(d[0][0], d[0][1], d[0][2]), h1 = mg_h(d[1][0], d[1][1], d[1][2]),
               h2 = mg_h(d[2][0], d[2][1], d[2][2]);
  a.sc[(a.cy0 + J) * a.ldc + a.cx0 + I] = mg_full_weight(h0, h1, h2, a.cs);
}

static int mg_resid_restrict_path(int64_t x0, int64_t cx0, const double* u, int64_t ld, const double* f, int64_t ldf,
                                  const double* sc, int64_t ldc) {
  return x0 % 2 == 0 && cx0 % 2 == 0 && walk_vec_ok(u, ld) && walk_vec_ok(sc, ldc) && (!f || walk_vec_ok(f, ldf))
             ? GMT_PATH_ROW_WALK
             : GMT_PATH_SCALAR;
}

static int mg_restrict_path(int64_t x0, int64_t cx0, const double* d, int64_t ldd, const double* sc, int64_t ldc) {
  return x0 % 2 == 0 && cx0 % 2 == 0 && walk_vec_ok(d, ldd) && walk_vec_ok(sc, ldc) ? GMT_PATH_PT : GMT_PATH_SCALAR;
}
static int mg_prolong_path(int64_t x0, const double* e, int64_t lde, const double* u, int64_t ld) {
  return x0 % 2 == 0 && walk_vec_ok(e, lde) && walk_vec_ok(u, ld) ? GMT_PATH_PT : GMT_PATH_SCALAR;
}

// ---- table-driven transfers between levels that are not nested (gmt/mg_tab.hpp) ----
//
// The tables of a plan: per fine column / row the coarse cell below it and t,
// per coarse column / row {first tap, tap count} and four weights.  Every
// index was checked on the host before the upload (gmt_mg_xfer_plan_create):
// the kernels add them to the region's origin without a second look.  Table
// bases are 16-B aligned and a lane's pair starts at an even entry, so the
// pair's entries of the prolongation come by one 8-B and one 16-B load, a
// coarse cell's by one 8-B and two 16-B loads, on any path; rows are uniform
// over most of a wave.
struct MgXferPlan {
  int64_t fn[2] = {0, 0}, cn[2] = {0, 0};  // fine and coarse extents of the region, x then y
  const int32_t* pq[2] = {nullptr, nullptr};
  const double* pt[2] = {nullptr, nullptr};
  const int2* rf[2] = {nullptr, nullptr};
  const double* rw[2] = {nullptr, nullptr};
  void* dev = nullptr;  // the one allocation behind them
};

// u' of one fine cell: p points at coarse cell (J, I) below / west of it
__device__ __forceinline__ double mg_tab_prolong_cell(const double* __restrict__ p, int64_t lde, double tx, double ty,
                                                      double u) {
#pragma clang fp contract(off)
  const double w0x = 1.0 - tx, w0y = 1.0 - ty;
  const double b0 = w0x * p[0], b1 = tx * p[1];
  const double bot = b0 + b1;
  const double t0 = w0x * p[lde], t1 = tx * p[lde + 1];
  const double top = t0 + t1;
  const double vb = w0y * bot, vt = ty * top;
  const double v = vb + vt;
  return u + v;
}

// e0 at coarse cell (0, 0) of the region, u0 at fine cell (0, 0)
__global__ __launch_bounds__(kBlock) void mg_prolong_tab_scalar(int64_t nx, int64_t ny,
                                                                const int32_t* __restrict__ qx,
                                                                const double* __restrict__ tx,
                                                                const int32_t* __restrict__ qy,
                                                                const double* __restrict__ ty,
                                                                const double* __restrict__ e0, int64_t lde,
                                                                double* __restrict__ u0, int64_t ld) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (t >= nx * ny) return;
  const int64_t i = t % nx, j = t / nx;
  double* q = u0 + j * ld + i;
  *q = mg_tab_prolong_cell(e0 + static_cast<int64_t>(qy[j]) * lde + qx[i], lde, tx[i], ty[j], *q);
}

__global__ __launch_bounds__(kBlock) void mg_prolong_tab_pt(int64_t nx, int64_t ny, const int32_t* __restrict__ qx,
                                                            const double* __restrict__ tx,
                                                            const int32_t* __restrict__ qy,
                                                            const double* __restrict__ ty,
                                                            const double* __restrict__ e0, int64_t lde,
                                                            double* __restrict__ u0, int64_t ld) {
  const int64_t npx = (nx + 1) / 2;  // fine pairs per row
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (t >= npx * ny) return;
  const int64_t i = 2 * (t % npx), j = t / npx;
  const double* er = e0 + static_cast<int64_t>(qy[j]) * lde;
  const double tyj = ty[j];
  double* q = u0 + j * ld + i;
  if (i + 1 < nx) {
    const int2 I = *reinterpret_cast<const int2*>(qx + i);
    const d2 tt = ld2(tx + i);
    d2 v = ld2(q);
    v.x = mg_tab_prolong_cell(er + I.x, lde, tt.x, tyj, v.x);
    v.y = mg_tab_prolong_cell(er + I.y, lde, tt.y, tyj, v.y);
    st2(q, v);
  } else {
    *q = mg_tab_prolong_cell(er + qx[i], lde, tx[i], tyj, *q);
  }
}

// the weighted taps of one coarse column in one fine row: p at the first tap.
// No branch: a column of three taps re-reads its third tap (a real one, so
// nothing outside the read set is touched) and the sum without it is selected,
// so every load of a lane can be in flight at once.
__device__ __forceinline__ double mg_tab_h(const double* __restrict__ p, d2 wa, d2 wb, int cnt) {
#pragma clang fp contract(off)
  const bool four = cnt == 4;
  const double d3 = p[four ? 3 : 2];
  const double a0 = wa.x * p[0], a1 = wa.y * p[1], a2 = wb.x * p[2], a3 = wb.y * d3;
  const double h = (a0 + a1) + a2;
  const double h4 = h + a3;
  return four ? h4 : h;
}

// one coarse cell: p at its first tap row and column; rows as columns
__device__ __forceinline__ double mg_tab_restrict_cell(const double* __restrict__ p, int64_t ldd, d2 wxa, d2 wxb,
                                                       int cx, d2 wya, d2 wyb, int cy) {
#pragma clang fp contract(off)
  const bool four = cy == 4;
  const double h0 = mg_tab_h(p, wxa, wxb, cx), h1 = mg_tab_h(p + ldd, wxa, wxb, cx),
               h2 = mg_tab_h(p + 2 * ldd, wxa, wxb, cx), h3 = mg_tab_h(p + (four ? 3 : 2) * ldd, wxa, wxb, cx);
  const double a0 = wya.x * h0, a1 = wya.y * h1, a2 = wyb.x * h2, a3 = wyb.y * h3;
  const double s = (a0 + a1) + a2;
  const double s4 = s + a3;
  return four ? s4 : s;
}

// d0 at fine cell (0, 0) of the region, s0 at coarse cell (0, 0)
__global__ __launch_bounds__(kBlock) void mg_restrict_tab_scalar(int64_t mx, int64_t my, const int2* __restrict__ fx,
                                                                 const double* __restrict__ wx,
                                                                 const int2* __restrict__ fy,
                                                                 const double* __restrict__ wy,
                                                                 const double* __restrict__ d0, int64_t ldd,
                                                                 double* __restrict__ s0, int64_t ldc) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= mx * my) return;
  const int64_t I = i % mx, J = i / mx;
  const int2 ax = fx[I], ay = fy[J];
  const double* p = d0 + static_cast<int64_t>(ay.x) * ldd + ax.x;
  s0[J * ldc + I] = mg_tab_restrict_cell(p, ldd, ld2(wx + 4 * I), ld2(wx + 4 * I + 2), ax.y, ld2(wy + 4 * J),
                                         ld2(wy + 4 * J + 2), ay.y);
}

// One lane per coarse cell, not per pair: neighbouring lanes then tap fine cells
// 16 B apart instead of 32, and a wave's 8-B loads touch half the cache lines
// per coarse cell (measured at 8192^2: 0.30 ms with a pair per lane, 0.20 ms so).
// The lanes of a coarse row are padded to an even count, so the two cells of a
// pair sit in one wave: the odd lane hands its value over and the even lane
// makes the pair's 16-B store.
__global__ __launch_bounds__(kBlock) void mg_restrict_tab_pt(int64_t mx, int64_t my, const int2* __restrict__ fx,
                                                             const double* __restrict__ wx,
                                                             const int2* __restrict__ fy,
                                                             const double* __restrict__ wy,
                                                             const double* __restrict__ d0, int64_t ldd,
                                                             double* __restrict__ s0, int64_t ldc) {
  const int64_t npl = (mx + 1) / 2 * 2;  // lanes per coarse row
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  const int64_t I = i % npl, J = i / npl;
  const bool live = J < my && I < mx;
  double v = 0.0;
  if (live) {
    const int2 ax = fx[I], ay = fy[J];
    const double* p = d0 + static_cast<int64_t>(ay.x) * ldd + ax.x;
    v = mg_tab_restrict_cell(p, ldd, ld2(wx + 4 * I), ld2(wx + 4 * I + 2), ax.y, ld2(wy + 4 * J), ld2(wy + 4 * J + 2),
                             ay.y);
  }
  const double east = __shfl_xor(v, 1);  // every lane of the wave is here: no lane left before
  if (live && (I & 1) == 0) {
    double* q = s0 + J * ldc + I;
    if (I + 1 < mx) {
      d2 o;
      o.x = v, o.y = east;
      st2(q, o);
    } else {  // the single last coarse column of an odd mx
      *q = v;
    }
  }
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
  const MgCheck c = mg_smooth_check(x0, nx, y0, ny, u, ld, f, ldf, out, ldo);
  if (c != MgCheck::kRun) return mg_check_code(c, kMgRefuse);
  const bool walk = mg_smooth_path(x0, u, ld, f, ldf, out, ldo) == GMT_PATH_ROW_WALK;
  return f ? mg_smooth_launch<true>(walk, x0, nx, y0, ny, u, ld, f, ldf, c0, c1, omega, out, ldo, s)
           : mg_smooth_launch<false>(walk, x0, nx, y0, ny, u, ld, f, ldf, c0, c1, omega, out, ldo, s);
}

extern "C" int gmt_mg_smooth_k_geom(int k, int64_t* wave_cols, int64_t* block_cols) {
  using namespace gmt;
  if (!mg_depth_ok(k)) return kMgRefuse;
  if (wave_cols) *wave_cols = mg_fuse_wave_cols(k);
  if (block_cols) *block_cols = mg_fuse_block_cols(k);
  return 0;
}

extern "C" int gmt_mg_smooth_k_path(int k, int64_t x0, int64_t nx, int64_t ny, int halo_mask, const double* u,
                                    int64_t ld, const double* f, int64_t ldf, const double* out, int64_t ldo,
                                    int64_t* seg_rows) {
  using namespace gmt;
  if (!mg_depth_ok(k) || !mg_mask_ok(halo_mask)) return mg_fuse_path(GMT_PATH_NONE, k, nx, ny, seg_rows);
  if (k == 1) return gmt_mg_smooth_path(x0, nx, ny, u, ld, f, ldf, out, ldo, seg_rows);
  return mg_fuse_path(mg_smooth_path(x0, u, ld, f, ldf, out, ldo), k, nx, ny, seg_rows);
}

extern "C" int gmt_mg_smooth_k(int k, int64_t x0, int64_t nx, int64_t y0, int64_t ny, int halo_mask, const double* u,
                               int64_t ld, const double* f, int64_t ldf, double c0, double c1, double omega,
                               double* out, int64_t ldo, void* stream) {
  using namespace gmt;
  const MgCheck c = mg_fuse_check(k, 0, x0, nx, y0, ny, halo_mask, u, ld, f, ldf, out, ldo);
  if (c != MgCheck::kRun) return mg_check_code(c, kMgRefuse);
  if (k == 1) return gmt_mg_smooth(x0, nx, y0, ny, u, ld, f, ldf, c0, c1, omega, out, ldo, stream);
  const MgFuseArgs a{x0, nx, y0, ny, halo_mask, u, ld, f, ldf, c0, c1, omega, out, ldo, 0, 0, 0, 0};
  return mg_smooth_k_run<false, false>(k, a, static_cast<hipStream_t>(stream));
}

extern "C" int gmt_mg_smooth_rb_path(int h, int par, int64_t x0, int64_t nx, int64_t ny, int halo_mask,
                                     const double* u, int64_t ld, const double* f, int64_t ldf, const double* out,
                                     int64_t ldo, int64_t* seg_rows) {
  using namespace gmt;
  const bool ok = mg_depth_ok(h) && mg_bit_ok(par) && mg_mask_ok(halo_mask);
  return mg_fuse_path(ok ? mg_smooth_path(x0, u, ld, f, ldf, out, ldo) : GMT_PATH_NONE, h, nx, ny, seg_rows);
}

extern "C" int gmt_mg_smooth_rb(int h, int par, int64_t x0, int64_t nx, int64_t y0, int64_t ny, int halo_mask,
                                const double* u, int64_t ld, const double* f, int64_t ldf, double c0, double c1,
                                double omega, double* out, int64_t ldo, void* stream) {
  using namespace gmt;
  const MgCheck c = mg_fuse_check(h, par, x0, nx, y0, ny, halo_mask, u, ld, f, ldf, out, ldo);
  if (c != MgCheck::kRun) return mg_check_code(c, kMgRefuse);
  const MgFuseArgs a{x0, nx, y0, ny, halo_mask, u, ld, f, ldf, c0, c1, omega, out, ldo, 0, 0, 0, par};
  return mg_smooth_k_run<true, false>(h, a, static_cast<hipStream_t>(stream));
}

// ---- the interpolation fused into h sweeps or half-sweeps (gmt_mg_prolong_smooth) ----

extern "C" int gmt_mg_prolong_smooth_geom(int h, int64_t* wave_cols, int64_t* block_cols) {
  return gmt_mg_smooth_k_geom(h, wave_cols, block_cols);
}

extern "C" int gmt_mg_prolong_smooth_path(int h, int rb, int par, int64_t x0, int64_t nx, int64_t y0, int64_t ny,
                                          int px, int py, int halo_mask, const double* e, int64_t cx0, int64_t cy0,
                                          int64_t lde, const double* u, int64_t ld, const double* f, int64_t ldf,
                                          const double* out, int64_t ldo, int64_t* seg_rows) {
  using namespace gmt;
  const bool ok = mg_prolong_smooth_check(h, rb, par, x0, nx, y0, ny, px, py, halo_mask, e, cx0, cy0, lde, u, ld, f,
                                          ldf, out, ldo, nullptr) != MgCheck::kRefuse;
  // e is read 8 B per lane: no rule of its own
  return mg_fuse_path(ok ? mg_smooth_path(x0, u, ld, f, ldf, out, ldo) : GMT_PATH_NONE, h, nx, ny, seg_rows);
}

extern "C" int gmt_mg_prolong_smooth(int h, int rb, int par, int64_t x0, int64_t nx, int64_t y0, int64_t ny, int px,
                                     int py, int halo_mask, const double* e, int64_t cx0, int64_t cy0, int64_t lde,
                                     const double* u, int64_t ld, const double* f, int64_t ldf, double c0, double c1,
                                     double omega, double* out, int64_t ldo, void* stream) {
  using namespace gmt;
  hipStream_t s = static_cast<hipStream_t>(stream);
  MgCoarseWin w;
  const MgCheck c = mg_prolong_smooth_check(h, rb, par, x0, nx, y0, ny, px, py, halo_mask, e, cx0, cy0, lde, u, ld, f,
                                            ldf, out, ldo, &w);
  if (c != MgCheck::kRun) return mg_check_code(c, kMgRefuse);
  const MgProArgs a{{x0, nx, y0, ny, halo_mask, u, ld, f, ldf, c0, c1, omega, out, ldo, 0, 0, 0, par},
                    e + cy0 * lde + cx0, lde, px, py, w.ilo, w.ihi, w.jlo, w.jhi};
  return rb ? mg_smooth_k_run<true, true>(h, a, s) : mg_smooth_k_run<false, true>(h, a, s);
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
  int64_t mx, my;
  const MgCheck c = mg_restrict_check(x0, nx, y0, ny, px, py, d, ldd, sc, cx0, cy0, ldc, &mx, &my);
  if (c != MgCheck::kRun) return mg_check_code(c, kMgRefuse);
  const bool pt = mg_restrict_path(x0, cx0, d, ldd, sc, ldc) == GMT_PATH_PT;
  unsigned grid;
  if (!mg_lane_grid((pt ? (mx + 1) / 2 : mx) * my, &grid)) return kMgRefuse;
  if (pt)
    mg_restrict_pt<<<grid, kBlock, 0, s>>>(x0, y0, px, py, mx, my, d, ldd, cs, sc, cx0, cy0, ldc);
  else
    mg_restrict_scalar<<<grid, kBlock, 0, s>>>(x0, y0, px, py, mx, my, d, ldd, cs, sc, cx0, cy0, ldc);
  GMT_RET_LAUNCH();
}

extern "C" int gmt_mg_resid_restrict_geom(int64_t* wave_cols, int64_t* block_cols) {
  return gmt_mg_smooth_k_geom(2, wave_cols, block_cols);
}

extern "C" int gmt_mg_resid_restrict_path(int64_t x0, int64_t nx, int64_t y0, int64_t ny, int px, int py,
                                          int halo_mask, const double* u, int64_t ld, const double* f, int64_t ldf,
                                          const double* sc, int64_t cx0, int64_t cy0, int64_t ldc,
                                          int64_t* seg_rows) {
  using namespace gmt;
  int64_t mx, my;
  // the parities count here on an empty region too
  const bool ok = mg_bit_ok(px) && mg_bit_ok(py) &&
                  mg_resid_restrict_check(x0, nx, y0, ny, px, py, halo_mask, u, ld, f, ldf, sc, cx0, cy0, ldc, &mx,
                                          &my) != MgCheck::kRefuse;
  return mg_fuse_path(ok ? mg_resid_restrict_path(x0, cx0, u, ld, f, ldf, sc, ldc) : GMT_PATH_NONE, 2, nx, ny,
                      seg_rows);
}

extern "C" int gmt_mg_resid_restrict(int64_t x0, int64_t nx, int64_t y0, int64_t ny, int px, int py, int halo_mask,
                                     const double* u, int64_t ld, const double* f, int64_t ldf, double c0, double c1,
                                     double cs, double* sc, int64_t cx0, int64_t cy0, int64_t ldc, void* stream) {
  using namespace gmt;
  hipStream_t s = static_cast<hipStream_t>(stream);
  int64_t mx, my;
  const MgCheck c = mg_resid_restrict_check(x0, nx, y0, ny, px, py, halo_mask, u, ld, f, ldf, sc, cx0, cy0, ldc, &mx,
                                            &my);
  if (c != MgCheck::kRun) return mg_check_code(c, kMgRefuse);
  MgRrArgs a{x0, nx, y0, ny, px, py, halo_mask, u, ld, f, ldf, c0, c1, cs, sc, cx0, cy0, ldc, mx, my, 0, 0, 0};
  if (mg_resid_restrict_path(x0, cx0, u, ld, f, ldf, sc, ldc) == GMT_PATH_ROW_WALK) {
    if (!mg_fuse_grid(2, &a)) return kMgRefuse;
    if (f)
      mg_resid_restrict_walk<true><<<grid_1d(a.nblocks), kBlock, 0, s>>>(a);
    else
      mg_resid_restrict_walk<false><<<grid_1d(a.nblocks), kBlock, 0, s>>>(a);
  } else {
    unsigned grid;
    if (!mg_lane_grid(mx * my, &grid)) return kMgRefuse;
    if (f)
      mg_resid_restrict_scalar<true><<<grid, kBlock, 0, s>>>(a);
    else
      mg_resid_restrict_scalar<false><<<grid, kBlock, 0, s>>>(a);
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
  const MgCheck c = mg_prolong_add_check(x0, nx, y0, ny, px, py, e, cx0, cy0, lde, u, ld);
  if (c != MgCheck::kRun) return mg_check_code(c, kMgRefuse);
  const double* e0 = e + cy0 * lde + cx0;
  const bool pt = mg_prolong_path(x0, e, lde, u, ld) == GMT_PATH_PT;
  unsigned grid;
  if (!mg_lane_grid((pt ? (nx + 1) / 2 : nx) * ny, &grid)) return kMgRefuse;
  if (pt)
    mg_prolong_pt<<<grid, kBlock, 0, s>>>(x0, nx, y0, ny, px, py, e0, lde, u, ld);
  else
    mg_prolong_scalar<<<grid, kBlock, 0, s>>>(x0, nx, y0, ny, px, py, e0, lde, u, ld);
  GMT_RET_LAUNCH();
}

// ---- the table-driven transfers ----

extern "C" int gmt_mg_xfer_plan_create(const gmt_mg_xfer_desc* desc, void** plan) {
  using namespace gmt;
  if (plan) *plan = nullptr;
  if (!desc || !plan) return static_cast<int>(hipErrorInvalidValue);
  // every table on the host first: an index that fails its check is never uploaded
  MgAxisTab tab[2];
  for (int a = 0; a < 2; ++a)
    if (mg_axis_tab_build(desc->n[a], desc->m[a], desc->fo[a], desc->fn[a], desc->co[a], desc->cn[a], &tab[a]) != 0)
      return static_cast<int>(hipErrorInvalidValue);
  // one allocation, every table on a 16-B boundary
  auto pad = [](size_t b) { return (b + 15) / 16 * 16; };
  size_t off[2][4], bytes = 0;
  for (int a = 0; a < 2; ++a) {
    const size_t sz[4] = {tab[a].pq.size() * sizeof(int32_t), tab[a].pt.size() * sizeof(double),
                          tab[a].rf.size() * sizeof(int32_t), tab[a].rw.size() * sizeof(double)};
    for (int k = 0; k < 4; ++k) {
      off[a][k] = bytes;
      bytes += pad(sz[k]);
    }
  }
  std::vector<char> host(bytes + 16, 0);
  for (int a = 0; a < 2; ++a) {
    std::memcpy(host.data() + off[a][0], tab[a].pq.data(), tab[a].pq.size() * sizeof(int32_t));
    std::memcpy(host.data() + off[a][1], tab[a].pt.data(), tab[a].pt.size() * sizeof(double));
    std::memcpy(host.data() + off[a][2], tab[a].rf.data(), tab[a].rf.size() * sizeof(int32_t));
    std::memcpy(host.data() + off[a][3], tab[a].rw.data(), tab[a].rw.size() * sizeof(double));
  }
  auto* p = new (std::nothrow) MgXferPlan();
  if (!p) return static_cast<int>(hipErrorOutOfMemory);
  hipError_t e = hipMalloc(&p->dev, host.size());
  if (e == hipSuccess) e = hipMemcpy(p->dev, host.data(), host.size(), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    if (p->dev) (void)hipFree(p->dev);
    delete p;
    return static_cast<int>(e);
  }
  const char* base = static_cast<const char*>(p->dev);
  for (int a = 0; a < 2; ++a) {
    p->fn[a] = desc->fn[a];
    p->cn[a] = desc->cn[a];
    p->pq[a] = reinterpret_cast<const int32_t*>(base + off[a][0]);
    p->pt[a] = reinterpret_cast<const double*>(base + off[a][1]);
    p->rf[a] = reinterpret_cast<const int2*>(base + off[a][2]);
    p->rw[a] = reinterpret_cast<const double*>(base + off[a][3]);
  }
  *plan = p;
  return 0;
}

extern "C" void gmt_mg_xfer_plan_destroy(void* plan) {
  auto* p = static_cast<gmt::MgXferPlan*>(plan);
  if (!p) return;
  if (p->dev) (void)hipFree(p->dev);
  delete p;
}

extern "C" int gmt_mg_restrict_tab_path(int64_t x0, int64_t cx0, const double* d, int64_t ldd, const double* sc,
                                        int64_t ldc) {
  return gmt::mg_restrict_path(x0, cx0, d, ldd, sc, ldc);
}

extern "C" int gmt_mg_restrict_tab(const void* plan, int64_t x0, int64_t y0, const double* d, int64_t ldd, double* sc,
                                   int64_t cx0, int64_t cy0, int64_t ldc, void* stream) {
  using namespace gmt;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const auto* p = static_cast<const MgXferPlan*>(plan);
  if (!p) return static_cast<int>(hipErrorInvalidValue);
  const int64_t nx = p->fn[0], ny = p->fn[1], mx = p->cn[0], my = p->cn[1];
  const MgCheck c = mg_restrict_tab_check(nx, ny, mx, my, x0, y0, d, ldd, sc, cx0, cy0, ldc);
  if (c != MgCheck::kRun) return mg_check_code(c, kMgRefuse);
  const double* d0 = d + y0 * ldd + x0;
  double* s0 = sc + cy0 * ldc + cx0;
  const bool pt = mg_restrict_path(x0, cx0, d, ldd, sc, ldc) == GMT_PATH_PT;
  unsigned grid;  // pt: a lane per coarse cell, rows padded to pairs
  if (!mg_lane_grid((pt ? (mx + 1) / 2 * 2 : mx) * my, &grid)) return kMgRefuse;
  if (pt)
    mg_restrict_tab_pt<<<grid, kBlock, 0, s>>>(mx, my, p->rf[0], p->rw[0], p->rf[1], p->rw[1], d0, ldd, s0, ldc);
  else
    mg_restrict_tab_scalar<<<grid, kBlock, 0, s>>>(mx, my, p->rf[0], p->rw[0], p->rf[1], p->rw[1], d0, ldd, s0, ldc);
  GMT_RET_LAUNCH();
}

extern "C" int gmt_mg_prolong_add_tab_path(int64_t x0, const double* e, int64_t lde, const double* u, int64_t ld) {
  return gmt::mg_prolong_path(x0, e, lde, u, ld);
}

extern "C" int gmt_mg_prolong_add_tab(const void* plan, int64_t x0, int64_t y0, const double* e, int64_t cx0,
                                      int64_t cy0, int64_t lde, double* u, int64_t ld, void* stream) {
  using namespace gmt;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const auto* p = static_cast<const MgXferPlan*>(plan);
  if (!p) return static_cast<int>(hipErrorInvalidValue);
  const int64_t nx = p->fn[0], ny = p->fn[1], mx = p->cn[0];
  const MgCheck c = mg_prolong_add_tab_check(nx, ny, mx, x0, y0, e, cx0, cy0, lde, u, ld);
  if (c != MgCheck::kRun) return mg_check_code(c, kMgRefuse);
  const double* e0 = e + cy0 * lde + cx0;
  double* u0 = u + y0 * ld + x0;
  const bool pt = mg_prolong_path(x0, e, lde, u, ld) == GMT_PATH_PT;
  unsigned grid;
  if (!mg_lane_grid((pt ? (nx + 1) / 2 : nx) * ny, &grid)) return kMgRefuse;
  if (pt)
    mg_prolong_tab_pt<<<grid, kBlock, 0, s>>>(nx, ny, p->pq[0], p->pt[0], p->pq[1], p->pt[1], e0, lde, u0, ld);
  else
    mg_prolong_tab_scalar<<<grid, kBlock, 0, s>>>(nx, ny, p->pq[0], p->pt[0], p->pq[1], p->pt[1], e0, lde, u0, ld);
  GMT_RET_LAUNCH();
}
