// The row walk shared by the read-only residual (jacobi5_resid.hip), CG's
// operator apply (cg.hip), the Chebyshev step (cheby.hip) and the multigrid
// smoother (mg.hip): one pass over
// the 5-point neighbourhood of u that loads every row once per segment.
//
// A workgroup is four waves side by side (512 columns) on one row segment;
// each lane holds one column pair and each wave walks its 128 columns
// top-down with a three-row register window, so a row is loaded once per
// segment (plus the two rows around the segment).  The W/E neighbours of a
// pair come from the adjacent lanes through DPP; the two columns outside the
// wave come from one masked load each.  UNROLL rows are in flight per lane.
// Vertically adjacent segments of a strip are consecutive tiles, so
// xcd_swizzle keeps the rows they share in one L2.
//
// What a row does with its neighbourhood is the kernel's op:
//   begin(row, xl, xr)   its row pointers at the segment's first row; xl is
//                        the column a lane loads from (clamped, below), xr the
//                        lane's own column, stored to by live lanes only
//   load(j, jr)          its loads for slot j of the load phase, from its row
//                        jr (clamped like u's): they go out with that row's
//                        loads of u and before any compute, which is what
//                        keeps UNROLL rows in flight
//   row(j, w, e, a, b, c, f, live, pair)
//                        the cells of the pair b (x: W = w, E = b.y; y: W =
//                        b.x, E = e; N = a, S = c), stored j rows below the
//                        op's pointers; live / pair mask the two cells
//   advance(rows)        its pointers move on by rows = UNROLL rows
#pragma once
#include "common.hpp"

namespace gmt {

constexpr int kWalkWaveCols = 2 * kWave;                           // columns per wave
constexpr int kWalkBlockCols = kWalkWaveCols * (kBlock / kWave);   // columns per workgroup
constexpr int64_t kWalkMaxSeg = 256, kWalkMinSeg = 8;              // rows per segment

template <int UNROLL, bool HAS_F, class Op>
__device__ __forceinline__ void row_walk(int64_t x0, int64_t nx, int64_t y0, int64_t ny,
                                         const double* __restrict__ u, int64_t ld,
                                         const double* __restrict__ f, int64_t ldf, int64_t nseg,
                                         int64_t seg_rows, int64_t nblocks, Op& op) {
  const int64_t t = xcd_swizzle(blockIdx.x, nblocks);
  const int64_t seg = t % nseg, bx = t / nseg;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int64_t xw = bx * kWalkBlockCols + wave * kWalkWaveCols;  // the wave's first column
  if (xw >= nx) return;  // wave-uniform: every lane of a working wave stays active (DPP)
  const int64_t r0 = seg * seg_rows;
  const int64_t r1 = (r0 + seg_rows) < ny ? (r0 + seg_rows) : ny;
  const int64_t xr = xw + 2 * lane;
  const bool live = xr < nx, pair = xr + 1 < nx;
  // lanes past the region re-read its last pair (their cells are masked and
  // never stored); the lane of an odd last column loads the pair too: its
  // second value of u is the cell's E neighbour
  const int64_t xl = live ? xr : ((nx - 1) & ~int64_t(1));
  const bool west = lane == 0;
  const bool east = pair && (lane == kWave - 1 || xr + 2 >= nx);
  const double* p = u + (y0 + r0 - 1) * ld + x0 + xl;
  const double* pf = HAS_F ? f + (y0 + r0) * ldf + x0 + xl : nullptr;
  op.begin(y0 + r0, x0 + xl, x0 + xr);
  d2 a = ld2(p);  // row r - 1
  p += ld;
  d2 b = ld2(p);  // row r
  for (int64_t r = r0; r < r1; r += UNROLL) {
    const int64_t left = r1 - r;  // rows still to do, >= 1
    d2 c[UNROLL], fv[UNROLL];
    double ew[UNROLL], ee[UNROLL];
#pragma unroll
    for (int j = 0; j < UNROLL; ++j) {
      // rows past the segment are clamped to its last ones (loaded, not used)
      const int64_t oc = (j + 1 < left ? j + 1 : left) * ld;
      const int64_t jr = j < left - 1 ? j : left - 1;
      c[j] = ld2(p + oc);
      ew[j] = ee[j] = 0.0;
      if (west) ew[j] = p[jr * ld - 1];
      if (east) ee[j] = p[jr * ld + 2];
      op.load(j, jr);
      if (HAS_F) fv[j] = ld2(pf + jr * ldf);
    }
#pragma unroll
    for (int j = 0; j < UNROLL; ++j) {
      if (j < left) {
        const double wl = dpp_from_lower(b.y), eu = dpp_from_upper(b.x);
        const double w = west ? ew[j] : wl, e = east ? ee[j] : eu;
        op.row(j, w, e, a, b, c[j], HAS_F ? fv[j] : d2{0.0, 0.0}, live, pair);
      }
      a = b;
      b = c[j];
    }
    p += UNROLL * ld;
    if (HAS_F) pf += UNROLL * ldf;
    op.advance(UNROLL);
  }
}

// The epilogue of a kernel that leaves one sum and one max per workgroup.
__device__ __forceinline__ void write_block_partials(double acc, double m, double* __restrict__ psum,
                                                     double* __restrict__ pmax) {
  acc = block_sum(acc);
  m = block_max(m);
  if (threadIdx.x == 0) {
    psum[blockIdx.x] = acc;
    pmax[blockIdx.x] = m;
  }
}

// Rows per segment: as long as possible (two extra row loads per segment)
// while the launch still has 8 workgroups per compute unit, the most a CU
// holds.  A function of the region and the device only.
inline int walk_cus() {
  static const int cus = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
    return n;
  }();
  return cus;
}
inline int64_t walk_seg_rows(int64_t nx, int64_t ny) {
  const int cus = walk_cus();
  const int64_t nbx = (nx + kWalkBlockCols - 1) / kWalkBlockCols;
  int64_t L = kWalkMaxSeg;
  while (L > kWalkMinSeg && nbx * ((ny + L - 1) / L) < 8 * static_cast<int64_t>(cus)) L /= 2;
  return L;
}
inline int64_t walk_blocks(int64_t nx, int64_t ny, int64_t* nseg, int64_t* seg_rows) {
  *seg_rows = walk_seg_rows(nx, ny);
  *nseg = (ny + *seg_rows - 1) / *seg_rows;
  return ((nx + kWalkBlockCols - 1) / kWalkBlockCols) * *nseg;
}
// pairs per lane need 16-B aligned rows (and an even first column)
inline bool walk_vec_ok(const double* a, int64_t ld) { return aligned16(a) && ld % 2 == 0; }

}  // namespace gmt
