/*
 * gmt/kernels.h — C ABI of the hand-written gfx950 kernels in libgmt.so.
 *
 * Every entry point is asynchronous on the given HIP stream (pass the raw
 * hipStream_t as `void*`; NULL = the legacy default stream) and returns a
 * hipError_t as int (0 = success). The same ABI is used by the native MPI
 * apps (csrc/apps) and by the Python package through ctypes
 * (gpu_mpi_tests_amd/_native.py), so there is exactly one kernel code path.
 *
 * Layout convention (matches the reference's column-major arrays, e.g.
 * /root/reference/mpi_stencil2d_sycl.cc:40-43 `idx2`): a 2-D field is stored
 * as `ny` rows of `ld` elements; x (the reference's "dim 0") is the contiguous
 * axis, y ("dim 1") is the strided axis. In torch terms that is a row-major
 * tensor of shape [ny, ld].
 */
#ifndef GMT_KERNELS_H
#define GMT_KERNELS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- K1/K2: y <- a*x + y (fp64).  reference: daxpy.cu:73, mpi_daxpy_gt.cc:81 */
int gmt_daxpy(int64_t n, double a, const double* x, double* y, void* stream);

/* ---- K3: 1-D 5-tap stencil, out[i] = scale * sum_k c[k]*in[i+k], k=0..4.
 *      `in` has n_out+4 elements.  reference: mpi_stencil_gt.cc:54-59 */
int gmt_stencil5_1d(int64_t n_out, const double* coef5, double scale,
                    const double* in, double* out, void* stream);

/* ---- K4/K5/K11: 2-D field, 5-tap stencil along `dim` (0 = contiguous x,
 *      1 = strided y).  `in` is (ny_out [+4 if dim==1]) rows of ld_in,
 *      holding nx_out [+4 if dim==0] valid columns.
 *      reference: mpi_stencil2d_gt.cc:84-110, mpi_stencil2d_sycl.cc:53-75 */
int gmt_stencil5_2d(int dim, int64_t nx_out, int64_t ny_out, const double* coef5,
                    double scale, const double* in, int64_t ld_in, double* out,
                    int64_t ld_out, void* stream);
/* Which kernel a launcher picks (tests assert the path a case ran): the
 * one-element-per-lane fallback, the pair-per-thread kernels (stencil5_pt,
 * jacobi5_pt), the dim-1 register-window walk, the dim-1 LDS-DMA pipeline,
 * the row walk of the read-only Jacobi residual.
 * The CPU backend has no kernels to pick from and answers GMT_PATH_NONE. */
enum { GMT_PATH_NONE = 0, GMT_PATH_SCALAR = 1, GMT_PATH_PT = 2, GMT_PATH_D1_WIN = 3, GMT_PATH_D1_DMA = 4,
       GMT_PATH_ROW_WALK = 5 };
/* the kernel gmt_stencil5_2d would launch for these arguments (no launch);
   *seg_rows (may be NULL) gets the rows per segment of the dim-1 kernels, 0 otherwise */
int gmt_stencil5_2d_path(int dim, int64_t nx_out, int64_t ny_out, const double* in, int64_t ld_in,
                         const double* out, int64_t ld_out, int64_t* seg_rows);

/* ---- The same stencil split for a step that overlaps the halo exchange with
 *      the derivative: the cells that read ghost cells (the edges) and the
 *      rest (the interior).
 *
 *      Band rule: n = the output extent along `dim`; `sides` bit 0 selects
 *      the low end, bit 1 the high end;
 *        lo_w = (sides & 1) ? min(2, n) : 0
 *        hi_w = (sides & 2) ? min(2, n - lo_w) : 0
 *      the edges are the indices [0, lo_w) and [n - hi_w, n) along `dim`, the
 *      interior is [lo_w, n - hi_w): disjoint, and together the whole output
 *      for every n >= 0 (2 = the ghost depth of a 5-tap stencil: an output
 *      further in reads no ghost cell).
 *
 *      gmt_stencil5_2d_edges takes gmt_stencil5_2d's arguments (`in` / `out`
 *      of the WHOLE output) and writes only the edge cells, both sides in one
 *      launch of a kernel shaped for narrow bands; sides == 0 or an empty
 *      band launches nothing.  gmt_stencil5_2d_interior runs gmt_stencil5_2d
 *      on the interior sub-rectangle (an empty one launches nothing). */
static inline void gmt_stencil5_bands(int64_t n, int sides, int64_t* lo_w, int64_t* hi_w) {
  if (n < 0) n = 0;
  *lo_w = (sides & 1) ? (n < 2 ? n : 2) : 0;
  *hi_w = (sides & 2) ? (n - *lo_w < 2 ? n - *lo_w : 2) : 0;
}
int gmt_stencil5_2d_edges(int dim, int64_t nx_out, int64_t ny_out, const double* coef5,
                          double scale, const double* in, int64_t ld_in, double* out,
                          int64_t ld_out, int sides, void* stream);
int gmt_stencil5_2d_interior(int dim, int64_t nx_out, int64_t ny_out, const double* coef5,
                             double scale, const double* in, int64_t ld_in, double* out,
                             int64_t ld_out, int sides, void* stream);

/* ---- K6/K7/K8: batched strided 2-D copy (halo pack / unpack, fused L+R).
 *      Each descriptor copies `height` rows of `width` elements of
 *      `elem_bytes` (4 or 8) from src (row pitch src_ld elements) to dst
 *      (row pitch dst_ld elements).  Up to GMT_MAX_COPY2D descriptors are
 *      fused into one launch.  reference: mpi_stencil2d_gt.cc:166-174,239,251 */
#define GMT_MAX_COPY2D 8
typedef struct gmt_copy2d_desc {
  const void* src;
  void* dst;
  int64_t src_ld;
  int64_t dst_ld;
  int64_t width;
  int64_t height;
} gmt_copy2d_desc;
int gmt_copy2d_batched(int n_desc, const gmt_copy2d_desc* descs, int elem_bytes,
                       void* stream);
// The same copy by at most max_wgs workgroups in a grid-stride loop (0: one
// element per thread, the full grid) — for exchanges that run beside a pass
// holding nearly every CU slot (profiles/r04_overlap.md).
int gmt_copy2d_batched_wgs(int n_desc, const gmt_copy2d_desc* descs, int elem_bytes, int max_wgs,
                           void* stream);

/* ---- K9: axis sums of a 2-D field of nx x ny (row pitch ld).
 *      keep_dim == 0: out[x] = sum_y z[y][x]   (length nx)
 *      keep_dim == 1: out[y] = sum_x z[y][x]   (length ny)
 *      `workspace` must hold gmt_sum_axis_workspace(...) doubles.
 *      reference: mpi_stencil2d_gt.cc:611,620 (gt::sum_axis_to) */
int64_t gmt_sum_axis_workspace(int keep_dim, int64_t nx, int64_t ny);
int gmt_sum_axis(int keep_dim, int64_t nx, int64_t ny, const double* z, int64_t ld,
                 double* out, double* workspace, void* stream);

/* ---- K10/K12: out[0] = sum over the nx x ny region of (a - b)^2
 *      (NOT square-rooted, so partial results can be all-reduced).
 *      `workspace` must hold gmt_diff_sq_workspace(...) doubles.
 *      reference: mpi_stencil2d_gt.cc:555, mpi_stencil2d_sycl.cc:165-181 */
int64_t gmt_diff_sq_workspace(int64_t nx, int64_t ny);
int gmt_diff_sq(int64_t nx, int64_t ny, const double* a, int64_t lda, const double* b,
                int64_t ldb, double* out, double* workspace, void* stream);

/* ---- out[0] = sum of x[0..n) (one HBM pass, deterministic order);
 *      workspace of gmt_sum_workspace(n) doubles.  The DAXPY partial sums
 *      (reference: host loops, mpi_daxpy_nvtx.cc:251-268) */
int64_t gmt_sum_workspace(int64_t n);
int gmt_sum(int64_t n, const double* x, double* out, double* workspace, void* stream);

/* ---- out[i] = sum (op 0) or max (op 1) over r = 0..nslices-1 of
 *      in[r*n + i], in rank order (an all-gather + this = a deterministic
 *      all-reduce; out may alias slice 0 of in only if it is in[0..n)).
 *      The sum is the IEEE additions acc = in[i]; acc += in[r*n + i] (inf and
 *      NaN propagate); the max is fmax in the same order on both backends: a
 *      NaN operand is ignored, out[i] is NaN only if every slice holds NaN.
 *      n == 0 does nothing; op > 1, n < 0 or nslices < 1 is refused. */
int gmt_slices_reduce(int op, int64_t n, int nslices, const double* in, double* out, void* stream);

/* ---- max over the nx x ny region of |z| -> out[0]; workspace of
 *      gmt_diff_sq_workspace(nx, ny) doubles */
int gmt_abs_max(int64_t nx, int64_t ny, const double* z, int64_t ld, double* out, double* workspace,
                void* stream);

/* ---- bitwise comparison of two nx x ny regions: out[0] = max |a - b|
 *      (NaN -> +inf), out[1] = number of elements whose 64 bits differ (as a
 *      double: exact to 2^53).  Deterministic two-pass; workspace of
 *      2 * gmt_diff_sq_workspace(nx, ny) doubles.  bench.py's check of the
 *      timed run (reference: the err_norm of the timed field,
 *      mpi_stencil2d_gt.cc:541-570) */
int gmt_diff_bits(int64_t nx, int64_t ny, const double* a, int64_t lda, const double* b, int64_t ldb,
                  double* out, double* workspace, void* stream);

/* ---- analytic fill z[y][x] = (x0+i*dx)^3 + (y0+j*dy)^2 over nx x ny (device
 *      side replacement of the reference's host init loops,
 *      mpi_stencil2d_gt.cc:439-497).  mode 0: x^3+y^2 (z), 1: 3x^2 (dz/dx),
 *      2: 2y (dz/dy), 3: x (linear ramp; DAXPY inputs), 4: x^3+y^2 on the
 *      integer lattice x = (x0 + i)*dx, y = (y0 + j)*dy with x0, y0 integer
 *      indices, no fma contraction (bitwise reproducible on the host),
 *      5: uniform [0, 1) random field, a counter-based hash (splitmix64) of
 *      the integer lattice point (x0 + i, y0 + j) with seed (uint64) dx —
 *      decomposition-independent random init.
 *      Jacobi source terms (JacobiConfig::source), both on the integer lattice:
 *      6: uniform [-dy, dy): dy * (2 r - 1) with r mode 5's hash of the same
 *      point and seed dx (no contraction: 2 r - 1 is exact, one rounding),
 *      7: -(1.5*x + 0.5)*dx*dx with x = (x0 + i)*dx, no contraction — the
 *      sweep source s = -h^2/4 (6x + 2) for which mode 4's x^3 + y^2
 *      (dx = dy = h) is the discrete fixed point of un = J(u) + s. */
int gmt_fill_poly(int mode, int64_t nx, int64_t ny, double x0, double dx, double y0,
                  double dy, double* z, int64_t ld, void* stream);
/* Per-exchange halo check (the apps' --check): counts the cells of the
 * nx x ny block z (pitch ld) that differ from x^3 + y^2 + offset at
 * x = x0 + i*dx, y = y0 + j*dy by more than rtol * (1 + |expected|), adding
 * the count to *bad (a device counter) — one small launch after each
 * exchange over the ghost rows it filled.  gmt_add_scalar adds v to every
 * cell of a block (the per-iteration offset that makes a stale ghost row
 * visible). */
int gmt_poly_check(int64_t nx, int64_t ny, double x0, double dx, double y0, double dy, double offset,
                   double rtol, const double* z, int64_t ld, unsigned* bad, void* stream);
int gmt_add_scalar(int64_t nx, int64_t ny, double v, double* z, int64_t ld, void* stream);

/* ---- u[y][x] += g[y][x] over nx x ny (pitches ld / ldg doubles), one
 *      rounding per cell; cells outside the region are untouched
 *      (csrc/kernels/add2d.hip).  The streaming add that ends a Poisson block
 *      of the Jacobi engine: u(t+n) = L^n(u(t)) + g_n (gmt/jacobi.hpp
 *      JacobiConfig::source).  24 B per point.  nx == 0 or ny == 0 launches
 *      nothing and returns 0; a negative extent, a NULL pointer or a pitch
 *      shorter than nx is refused (non-zero, the same on both backends). */
int gmt_add2d(int64_t nx, int64_t ny, const double* g, int64_t ldg, double* u, int64_t ld, void* stream);
/* GMT_PATH_PT (column pairs: both pointers 16-B aligned, both pitches even; an
 * odd nx keeps it with a scalar last column) or GMT_PATH_SCALAR */
int gmt_add2d_path(int64_t nx, const double* g, int64_t ldg, const double* u, int64_t ld);

/* ---- 2-D 5-point Jacobi sweep (the BASELINE "5-pt Jacobi" extension):
 *      for y in [y0, y0+ny), x in [x0, x0+nx) (absolute array coordinates):
 *        un[y][x] = c0*(u[y][x-1]+u[y][x+1]+u[y-1][x]+u[y+1][x]) + c1*f[y][x]
 *      f may be NULL (Laplace).  If resid_partial != NULL, the kernel also
 *      accumulates sum (un-u)^2 and leaves the total in resid_partial[0]
 *      (resid_partial must hold gmt_jacobi_resid_workspace(...) doubles). */
int64_t gmt_jacobi_resid_workspace(int64_t nx, int64_t ny);
int gmt_jacobi5(int64_t x0, int64_t nx, int64_t y0, int64_t ny, const double* u,
                double* un, int64_t ld, const double* f, int64_t ldf, double c0,
                double c1, double* resid_partial, void* stream);
/* GMT_PATH_PT or GMT_PATH_SCALAR for gmt_jacobi5 with these arguments */
int gmt_jacobi5_path(int64_t x0, const double* u, const double* un, int64_t ld, const double* f, int64_t ldf);
/* Same sweep for a list of rectangles in one launch (the boundary "frame" of
 * an overlapped step: up to 4 strips).  rect = {x0, nx, y0, ny}. */
int gmt_jacobi5_rects(int n_rect, const int64_t* rects, const double* u, double* un,
                      int64_t ld, const double* f, int64_t ldf, double c0, double c1,
                      void* stream);
/* ---- Read-only residual of that sweep (csrc/kernels/jacobi5_resid.hip), one
 *      HBM read pass, u is never written.  With
 *        d = c0*((u[y][x-1]+u[y][x+1]) + (u[y-1][x]+u[y+1][x])) [+ c1*f[y][x]] - u[y][x]
 *      over the region (evaluated without contraction): out[0] = sum d^2 (not
 *      square-rooted, so partial results can be all-reduced), out[1] = max |d|
 *      with a NaN d counted as +inf.  Deterministic summation order; an empty
 *      region gives {0, 0}.  `workspace` must hold
 *      gmt_jacobi5_resid_workspace(nx, ny) doubles. */
int64_t gmt_jacobi5_resid_workspace(int64_t nx, int64_t ny);
int gmt_jacobi5_resid(int64_t x0, int64_t nx, int64_t y0, int64_t ny, const double* u, int64_t ld,
                      const double* f, int64_t ldf, double c0, double c1,
                      double* out /* 2 doubles */, double* workspace, void* stream);
/* GMT_PATH_ROW_WALK or GMT_PATH_SCALAR: the kernel the call would launch, nothing launched;
 * *seg_rows (may be NULL) = rows per segment of the row walk, 0 otherwise */
int gmt_jacobi5_resid_path(int64_t x0, int64_t nx, int64_t ny, const double* u, int64_t ld, const double* f,
                           int64_t ldf, int64_t* seg_rows);
/* ---- Conjugate-gradient kernels (csrc/kernels/cg.hip) for A = I - J, J the
 *      Laplace sweep above: the three launches of one CG iteration
 *      (JacobiSolver::cg).  Conventions of gmt_jacobi5_resid: absolute x0, nx,
 *      y0, ny, every field with its own pitch, asynchronous on `stream`.  Every
 *      cell expression is evaluated without contraction, on both backends, so
 *      given the same coefficient bits the fields are bitwise NumPy's; the
 *      sums and maxima are deterministic (block partials, reduce_partials).
 *      An empty region touches no field and sets out to {0, 0}.  Refused
 *      (non-zero, the same on both backends): a NULL field, out, num, den or
 *      workspace, a negative x0 or y0, x0 < 1 or y0 < 1 for apply, a
 *      pitch shorter than the columns the call touches (x0 + nx, for apply's
 *      input x0 + nx + 1), mode outside 0..1.  No cell outside the region is
 *      written; apply reads only the region's plus-shaped set.
 *      `workspace` must hold gmt_cg_workspace(nx, ny) doubles. */
int64_t gmt_cg_workspace(int64_t nx, int64_t ny);
/* mode 0: q = p - c0*((W+E)+(S+N)) of p, out = {sum p*q, 0} (f, ldf, c1 ignored)
 * mode 1: q = c0*((W+E)+(S+N)) [+ c1*f] - p, bitwise gmt_jacobi5_resid's d,
 *         out = {sum q^2, max |q| (NaN -> +inf)}; f may be NULL
 * The row walk of the residual kernel with a store: 16 B per point. */
int gmt_cg_apply(int mode, int64_t x0, int64_t nx, int64_t y0, int64_t ny, const double* p, int64_t ldp,
                 const double* f, int64_t ldf, double c0, double c1, double* q, int64_t ldq,
                 double* out /* 2 doubles */, double* workspace, void* stream);
/* a = *den > 0 ? *num / *den : 0 (a NaN or non-positive denominator gives 0);
 * x += a*p; r -= a*q; out = {sum r^2, max |r| (NaN -> +inf)} of the new r.
 * num, den: device scalars.  48 B per point. */
int gmt_cg_update(int64_t x0, int64_t nx, int64_t y0, int64_t ny, const double* num, const double* den,
                  const double* p, int64_t ldp, const double* q, int64_t ldq, double* x, int64_t ldx, double* r,
                  int64_t ldr, double* out /* 2 doubles */, double* workspace, void* stream);
/* b = *den > 0 ? *num / *den : 0; p = r + b*p.  24 B per point. */
int gmt_cg_dir(int64_t x0, int64_t nx, int64_t y0, int64_t ny, const double* num, const double* den,
               const double* r, int64_t ldr, double* p, int64_t ldp, void* stream);
/* The kernel each call would launch, nothing launched.  apply: GMT_PATH_ROW_WALK
 * (x0 even, every pointer 16-B aligned, every pitch even; *seg_rows, may be
 * NULL, = rows per segment) or GMT_PATH_SCALAR (*seg_rows = 0); f counts only
 * when non-NULL.  update / dir: GMT_PATH_PT (column pairs under the same rule;
 * an odd nx keeps it with a scalar last column) or GMT_PATH_SCALAR. */
int gmt_cg_apply_path(int64_t x0, int64_t nx, int64_t ny, const double* p, int64_t ldp, const double* f,
                      int64_t ldf, const double* q, int64_t ldq, int64_t* seg_rows);
int gmt_cg_update_path(int64_t x0, const double* p, int64_t ldp, const double* q, int64_t ldq, const double* x,
                       int64_t ldx, const double* r, int64_t ldr);
int gmt_cg_dir_path(int64_t x0, const double* r, int64_t ldr, const double* p, int64_t ldp);

/* ---- Chebyshev semi-iteration over the Laplace sweep (csrc/kernels/cheby.hip):
 *      the one launch of an iteration of JacobiSolver::cheby,
 *        v' = v + w*(G(u) - v),  G(u) = c0*((W+E)+(S+N)) [+ c1*f],
 *      u the current iterate, v the previous one, overwritten in place by the
 *      next; w by value.  Conventions of gmt_cg_apply: absolute x0 >= 1, nx,
 *      y0 >= 1, ny, ld >= x0 + nx + 1, ldv and ldf >= x0 + nx, asynchronous on
 *      `stream`.  The cell is evaluated without contraction on both backends,
 *      in the order o = c0*((w+e)+(n+s)); o = o + c1*f (only with f);
 *      t = o - v; v' = v + (w*t), so v' is bitwise NumPy's.  f may be NULL.
 *      u and v must not overlap: v' of one cell would be another cell's
 *      neighbour.  No cell outside the region is written; u is read only on
 *      the region's plus-shaped set, v and f only on the region.  An empty
 *      region (nx or ny 0) launches nothing and returns 0.  Refused (non-zero,
 *      the same on both backends): a NULL u or v, a negative extent, x0 < 1 or
 *      y0 < 1, a short pitch.  24 B per point, 32 with f. */
int gmt_cheby_step(int64_t x0, int64_t nx, int64_t y0, int64_t ny, const double* u, int64_t ld, const double* f,
                   int64_t ldf, double c0, double c1, double w, double* v, int64_t ldv, void* stream);
/* The kernel the call would launch, nothing launched: GMT_PATH_ROW_WALK (x0
 * even, every pointer 16-B aligned, every pitch even; *seg_rows, may be NULL,
 * = rows per segment) or GMT_PATH_SCALAR (*seg_rows = 0); f counts only when
 * non-NULL.  GMT_PATH_NONE on the CPU backend. */
int gmt_cheby_step_path(int64_t x0, int64_t nx, int64_t ny, const double* u, int64_t ld, const double* f,
                        int64_t ldf, const double* v, int64_t ldv, int64_t* seg_rows);

/* ---- Geometric multigrid over the Laplace sweep (csrc/kernels/mg.hip): the
 *      smoother and the two grid transfers of a V-cycle of JacobiSolver::mg.
 *      Levels are vertex-centred: coarse point (J, I) sits on fine interior
 *      point (2J+1, 2I+1) of the global lattice.  Conventions of
 *      gmt_cheby_step: absolute x0 >= 1, y0 >= 1, every field with its own
 *      pitch, asynchronous on `stream`, every cell evaluated without
 *      contraction in exactly the order given, on both backends, so the fields
 *      are bitwise NumPy's.  An empty region (nx or ny 0) launches nothing and
 *      returns 0.  Refused (non-zero, the same on both backends): a NULL field,
 *      a negative extent, x0 < 1 or y0 < 1, a short pitch, px or py outside
 *      0..1.  No cell outside the output region is written.
 *
 * smooth: out = u + omega*(G(u) - u), damped Jacobi, in the order
 *   o = c0*((W+E)+(N+S)); o = o + c1*f (only with f); t = o - u; out = u + omega*t.
 *   u and out must not overlap; ld >= x0 + nx + 1, ldo and ldf >= x0 + nx; u
 *   is read on the region's plus-shaped set.  The row walk with a 16-B store:
 *   16 B per point, 24 with f. */
int gmt_mg_smooth(int64_t x0, int64_t nx, int64_t y0, int64_t ny, const double* u, int64_t ld, const double* f,
                  int64_t ldf, double c0, double c1, double omega, double* out, int64_t ldo, void* stream);
/* restrict: full weighting of the fine field d over the fine region nx x ny at
 *   (x0, y0) into the coarse field sc at (cx0, cy0).  px, py in {0, 1}: the
 *   region-relative fine index of the first coarse column / row (1 when the
 *   region's global offset is even, 0 when it is odd); mx = (nx - px + 1)/2 by
 *   my = (ny - py + 1)/2 coarse cells are written.  With the centre
 *   (x, y) = (x0+px+2I, y0+py+2J) and H(r) = (d[r][x-1] + d[r][x+1]) + 2*d[r][x]:
 *   sc[cy0+J][cx0+I] = cs*((H(y-1) + H(y+1)) + 2*H(y)).  The weights sum to
 *   16 cs (the engine's cs = 0.25 folds in the factor 4 between h^2 and (2h)^2).
 *   d is read on the region and its 1-wide ring, corners included;
 *   ldd >= x0 + nx + 1, ldc >= cx0 + mx, cx0 and cy0 >= 0. */
int gmt_mg_restrict(int64_t x0, int64_t nx, int64_t y0, int64_t ny, int px, int py, const double* d, int64_t ldd,
                    double cs, double* sc, int64_t cx0, int64_t cy0, int64_t ldc, void* stream);
/* prolong_add: u += P e on the fine region, P bilinear interpolation from the
 *   coarse field e whose cell (0, 0) of the region's mx x my is at (cx0, cy0);
 *   px, py as for restrict.  By how a fine cell sits relative to the coarse
 *   points: on one, u + e; between two in x, u + 0.5*(eW + eE); between two in
 *   y, u + 0.5*(eS + eN); between four, u + 0.25*((eSW + eSE) + (eNW + eNE))
 *   (S the lower row index).  e is read on its mx x my cells and their 1-wide
 *   ring, corners included; cx0 and cy0 >= 1, lde >= cx0 + mx + 1,
 *   ld >= x0 + nx.  e and u must not overlap. */
int gmt_mg_prolong_add(int64_t x0, int64_t nx, int64_t y0, int64_t ny, int px, int py, const double* e, int64_t cx0,
                       int64_t cy0, int64_t lde, double* u, int64_t ld, void* stream);
/* The kernel each call would launch, nothing launched.  smooth:
 * GMT_PATH_ROW_WALK (x0 even, every pointer 16-B aligned, every pitch even;
 * *seg_rows, may be NULL, = rows per segment) or GMT_PATH_SCALAR (*seg_rows =
 * 0); f counts only when non-NULL.  restrict / prolong_add: GMT_PATH_PT (pairs
 * of coarse cells / of fine cells per lane under the same rule, for restrict
 * with an even cx0 too; an odd count keeps it with a scalar last column) or
 * GMT_PATH_SCALAR.  GMT_PATH_NONE on the CPU backend. */
int gmt_mg_smooth_path(int64_t x0, int64_t nx, int64_t ny, const double* u, int64_t ld, const double* f, int64_t ldf,
                       const double* out, int64_t ldo, int64_t* seg_rows);
int gmt_mg_restrict_path(int64_t x0, int64_t cx0, const double* d, int64_t ldd, const double* sc, int64_t ldc);
int gmt_mg_prolong_add_path(int64_t x0, const double* e, int64_t lde, const double* u, int64_t ld);

/* ---- k smoothing sweeps in one memory pass: out[R] = the k-th of k
 *      applications of gmt_mg_smooth to u, R = nx x ny at (x0, y0), 16 B per
 *      point (24 with f) whatever k.  halo_mask has one bit per side of R:
 *      W = 1, E = 2, S = 4 (the lower row index), N = 8.
 *        set bit   halo side: the k cells beyond R hold a neighbour's current
 *                  cells; they are updatable
 *        clear bit ring side: the one cell beyond R is fixed
 *      B_j = R grown by k - j cells on each halo side (by 0 on a ring side);
 *      U_0 = u; for j = 1..k: U_j = smooth(U_{j-1}) on B_j (gmt_mg_smooth's
 *      cell, no contraction) and U_{j-1} everywhere else, so the ring cells
 *      along a grown edge stay fixed; out[R] = U_k.  No other cell of out is
 *      written (its ghost cells are stale afterwards).
 *      u is read on R grown by k on halo sides and by 1 on ring sides, corners
 *      included; f on R grown by k - 1 on halo sides and by 0 on ring sides;
 *      nothing else is read.  Refused (non-zero, nothing launched, the same on
 *      both backends): gmt_mg_smooth's refusals, k outside
 *      1..GMT_MG_MAX_FUSE, a mask outside 0..15, x0 or y0 smaller than the
 *      read set needs, a pitch shorter than the read set, u's read set
 *      overlapping out[R].  An empty region launches nothing and returns 0;
 *      k = 1 is gmt_mg_smooth.
 *      The fast path (the alignment rule of gmt_mg_smooth) is a row walk that
 *      carries k levels in registers, each level lagging the one below by a
 *      row; a wave's valid columns shrink by one per level and side, so
 *      neighbouring waves overlap by an even number of columns, and a row
 *      segment runs k warm-up rows above and below its own. */
#define GMT_MG_MAX_FUSE 4
enum { GMT_MG_HALO_W = 1, GMT_MG_HALO_E = 2, GMT_MG_HALO_S = 4, GMT_MG_HALO_N = 8 };
int gmt_mg_smooth_k(int k, int64_t x0, int64_t nx, int64_t y0, int64_t ny, int halo_mask, const double* u, int64_t ld,
                    const double* f, int64_t ldf, double c0, double c1, double omega, double* out, int64_t ldo,
                    void* stream);
/* GMT_PATH_ROW_WALK (*seg_rows, may be NULL, = the output rows per segment the
 * launch would use) or GMT_PATH_SCALAR (one lane per output cell, each
 * evaluating its own dependence cone; *seg_rows = 0); nothing launched.
 * GMT_PATH_NONE on the CPU backend and for arguments the call would refuse. */
int gmt_mg_smooth_k_path(int k, int64_t x0, int64_t nx, int64_t ny, int halo_mask, const double* u, int64_t ld,
                         const double* f, int64_t ldf, const double* out, int64_t ldo, int64_t* seg_rows);
/* Output columns per wave and per workgroup of the fast path for k sweeps
 * (either pointer may be NULL); non-zero for k outside 1..GMT_MG_MAX_FUSE. */
int gmt_mg_smooth_k_geom(int k, int64_t* wave_cols, int64_t* block_cols);

/* ---- h coloured half-sweeps of red-black Gauss-Seidel in one memory pass:
 *      gmt_mg_smooth_k with h for k and a colour rule on top.  par in {0, 1} is
 *      the colour phase of cell (x0, y0): in half-sweep j (1-based) cell (x, y)
 *      is due iff (x - x0) + (y - y0) + par + (j - 1) is even (a mathematical
 *      mod: the offsets are negative on halo sides).
 *      B_j = R grown by h - j on halo sides, by 0 on ring sides; U_0 = u;
 *      U_j = gmt_mg_smooth's cell of U_{j-1} (no contraction, the same order)
 *      on the due cells of B_j and U_{j-1} on every other cell; out[R] = U_h.
 *      Two consecutive half-sweeps are one red-black sweep, so h = 2 is one
 *      sweep and h = 4 two of them, still 16 B per point (24 with f).
 *      The read sets of u and f, the cells written, the empty region, the
 *      overlap rule and the refusals are gmt_mg_smooth_k's with h for k; par
 *      outside 0..1 is refused too.  The fast path (the alignment rule of
 *      gmt_mg_smooth) is the k-level row walk with k = h, h = 1 included, in
 *      the geometry of gmt_mg_smooth_k_geom(h): the lane's pair starts on an
 *      even region-relative column, so which cell of a pair is due is a scalar
 *      per row.  Other arguments take the one-lane-per-cell kernel.
 *      _path: as gmt_mg_smooth_k_path. */
int gmt_mg_smooth_rb(int h, int par, int64_t x0, int64_t nx, int64_t y0, int64_t ny, int halo_mask, const double* u,
                     int64_t ld, const double* f, int64_t ldf, double c0, double c1, double omega, double* out,
                     int64_t ldo, void* stream);
int gmt_mg_smooth_rb_path(int h, int par, int64_t x0, int64_t nx, int64_t ny, int halo_mask, const double* u,
                          int64_t ld, const double* f, int64_t ldf, const double* out, int64_t ldo,
                          int64_t* seg_rows);

/* ---- The residual and its full weighting in one memory pass: the composition
 *      of gmt_cg_apply mode 1 and gmt_mg_restrict without the field between
 *      them.  Let D be the field gmt_cg_apply mode 1 writes,
 *      q = c0*((W+E)+(S+N)) [+ c1*f] - u (the same order, no contraction), on
 *      the region R = nx x ny at (x0, y0) grown by one cell on every side
 *      whose halo_mask bit is set (W = 1, E = 2, S = 4, N = 8; corner cells
 *      where two set sides meet), and +0.0 on every other cell of R's 1-wide
 *      ring.  sc is then exactly gmt_mg_restrict(x0, nx, y0, ny, px, py, D, cs,
 *      sc, cx0, cy0): the same H and cs*((H(y-1) + H(y+1)) + 2*H(y)).  So sc is
 *      bitwise what the two calls give with the ring of d exchanged with a
 *      neighbour (set sides) or left zero (clear sides); D is never stored.
 *      u is read on R plus 2 cells beyond a set side and 1 beyond a clear
 *      side, without the outermost corner cell where two set sides meet (the
 *      cells gmt_mg_smooth_k(2, ...) reads); f on R plus 1 cell beyond set
 *      sides only; only sc's mx x my cells are written; 8 B per fine point read
 *      (16 with f), 2 written.
 *      Refused (non-zero, nothing launched, the same on both backends): every
 *      refusal of gmt_cg_apply and gmt_mg_restrict, a mask outside 0..15,
 *      x0 < 2 or y0 < 2 with that side's bit set, a pitch shorter than the
 *      read sets (ld >= x0 + nx + 2 with E set, else + 1; ldf >= x0 + nx + 1
 *      with E set, else + 0), sc's cells overlapping a read set.  An empty
 *      region launches nothing and returns 0.
 *      The fast path (GMT_PATH_ROW_WALK: x0 and cx0 even, every pointer 16-B
 *      aligned, every pitch even) is the two-level row walk of
 *      gmt_mg_smooth_k(2) in its geometry: level 1 is the residual cell, +0.0
 *      where the smoother would keep a cell; level 2 is H of the lane's coarse
 *      column with its W or E operand through DPP; a lane keeps H of the last
 *      two fine rows and stores one coarse cell every second row.  Everything
 *      else takes one lane per coarse cell (GMT_PATH_SCALAR), each with its own
 *      3 x 3 residuals.
 *      _path: the kernel the call would launch, nothing launched; *seg_rows
 *      (may be NULL) = the fine rows per segment of the walk, 0 otherwise;
 *      GMT_PATH_NONE on the CPU backend and for arguments the call would
 *      refuse.  _geom: the fine columns per wave and per workgroup of the walk
 *      (gmt_mg_smooth_k_geom(2)). */
int gmt_mg_resid_restrict(int64_t x0, int64_t nx, int64_t y0, int64_t ny, int px, int py, int halo_mask,
                          const double* u, int64_t ld, const double* f, int64_t ldf, double c0, double c1, double cs,
                          double* sc, int64_t cx0, int64_t cy0, int64_t ldc, void* stream);
int gmt_mg_resid_restrict_path(int64_t x0, int64_t nx, int64_t y0, int64_t ny, int px, int py, int halo_mask,
                               const double* u, int64_t ld, const double* f, int64_t ldf, const double* sc,
                               int64_t cx0, int64_t cy0, int64_t ldc, int64_t* seg_rows);
int gmt_mg_resid_restrict_geom(int64_t* wave_cols, int64_t* block_cols);

/* ---- The interpolation and the first h sweeps (rb = 0) or coloured
 *      half-sweeps (rb = 1) after it in one memory pass: the composition of
 *      gmt_mg_prolong_add and gmt_mg_smooth_k / gmt_mg_smooth_rb without the
 *      corrected field between them.  Let B0 be R = nx x ny at (x0, y0) grown
 *      by h cells on every side whose halo_mask bit is set and by nothing on
 *      the others: the cells gmt_mg_smooth_k(h) treats as current.  U' is u
 *      with gmt_mg_prolong_add's cell rule applied to every cell of B0, with
 *      the same px, py, cx0, cy0 and the same operation order; a halo cell has
 *      a negative region-relative index i and its coarse column follows from
 *      i - px as for any other cell.  out[R] = gmt_mg_smooth_k(h, ...)(U') for
 *      rb = 0 and gmt_mg_smooth_rb(h, par, ...)(U') for rb = 1.  The cells of
 *      u's read set outside B0 (the fixed ring) enter as they are, not even
 *      + 0.0 is added to them.  u, e and f are read only.
 *      u and f are read on the sets of gmt_mg_smooth_k(h); e on the coarse
 *      cells the rule names for B0, which lie within h/2 + 1 cells of the
 *      region's mx x my beyond a halo side and within 1 beyond a ring side.
 *      The fast path clamps its coarse loads to that box, so e must have every
 *      row of it: cy0 + my + h/2 + 1 rows with N set (else + 1).  Only the
 *      pitch can be checked from the arguments; the rows are the caller's.
 *      Refused (non-zero, nothing launched, the same on both backends): the
 *      refusals of gmt_mg_smooth_k / gmt_mg_smooth_rb and gmt_mg_prolong_add,
 *      rb outside 0..1, cx0 or cy0 smaller than h/2 + 1 on a halo side,
 *      lde < cx0 + mx + h/2 + 1 with E set (else + 1), out[R] overlapping the
 *      read set of u, e or f.  An empty region launches nothing and returns 0.
 *      The fast path (the alignment rule of gmt_mg_smooth for u, f and out) is
 *      the row walk of gmt_mg_smooth_k(h) / gmt_mg_smooth_rb(h) in its
 *      geometry: the row of u that arrives becomes U' before it enters level
 *      1.  A lane loads the coarse cell of its pair's coarse column, 8 B, once
 *      per coarse row and has its neighbour's through DPP; a fine row between
 *      two coarse rows uses the sums of both.  16 + 2 B per fine point (24 + 2
 *      with f) whatever h.  Other arguments take one lane per output cell
 *      (GMT_PATH_SCALAR), which corrects the cells of its cone as it loads
 *      them.  _path and _geom: as gmt_mg_smooth_k_path and
 *      gmt_mg_smooth_k_geom(h). */
int gmt_mg_prolong_smooth(int h, int rb, int par, int64_t x0, int64_t nx, int64_t y0, int64_t ny, int px, int py,
                          int halo_mask, const double* e, int64_t cx0, int64_t cy0, int64_t lde, const double* u,
                          int64_t ld, const double* f, int64_t ldf, double c0, double c1, double omega, double* out,
                          int64_t ldo, void* stream);
int gmt_mg_prolong_smooth_path(int h, int rb, int par, int64_t x0, int64_t nx, int64_t y0, int64_t ny, int px, int py,
                               int halo_mask, const double* e, int64_t cx0, int64_t cy0, int64_t lde, const double* u,
                               int64_t ld, const double* f, int64_t ldf, const double* out, int64_t ldo,
                               int64_t* seg_rows);
int gmt_mg_prolong_smooth_geom(int h, int64_t* wave_cols, int64_t* block_cols);

/* ---- Table-driven transfers between two levels that are not nested: n fine
 *      and m coarse interior points per axis on the same interval (any m with
 *      3 or 4 fine points between the neighbours of a coarse one), linear
 *      interpolation P with position-dependent weights and its exact transpose
 *      R = P^T.  gmt/mg_tab.hpp defines the tables: fine point i (1-based,
 *      global) lies between coarse points q and q + 1 with
 *      q, r = divmod(i*(m+1), n+1), t = r/(n+1), weights 1.0 - t and t.
 *
 *      The tables reach a kernel only through a plan.  plan_create builds them
 *      on the host from the description below, checks that every tap of the
 *      coarse region lies within 2 fine cells of the fine region, that every
 *      coarse cell the fine region interpolates from lies within 1 of the
 *      coarse region and that every coarse point has 3 or 4 taps per axis, and
 *      only then uploads them (a synchronous copy: not inside a capture).  A
 *      description that fails is refused (non-zero, *plan = NULL): nothing it
 *      describes is ever launched.  Index 0 of each pair is x, 1 is y. */
typedef struct gmt_mg_xfer_desc {
  int64_t n[2], m[2];   /* global fine and coarse interior points */
  int64_t fo[2], fn[2]; /* the fine region: global cells fo+1 .. fo+fn (1-based) */
  int64_t co[2], cn[2]; /* the coarse region: global cells co+1 .. co+cn */
} gmt_mg_xfer_desc;
int gmt_mg_xfer_plan_create(const gmt_mg_xfer_desc* desc, void** plan);
void gmt_mg_xfer_plan_destroy(void* plan); /* NULL is allowed; not while a launch that uses it is in flight */
/* restrict_tab: sc = P^T d.  d holds the plan's fine region at (x0, y0), sc its
 *   coarse region at (cx0, cy0).  Per coarse cell, with the taps and weights
 *   of its column (wx) and row (wy), per tapped fine row k
 *   h_k = ((wx0*d0 + wx1*d1) + wx2*d2) [+ wx3*d3], then
 *   s = ((wy0*h0 + wy1*h1) + wy2*h2) [+ wy3*h3]: the weights sum to about
 *   (n+1)/(m+1) per axis, there is no separate scale.  Only real taps are
 *   read: d on the region and up to 2 cells around it, corners included.
 *   x0 and y0 >= 2, ldd >= x0 + nx + 2, cx0 and cy0 >= 0, ldc >= cx0 + mx.
 * prolong_add_tab: u += P e on the plan's fine region at (x0, y0); e holds the
 *   coarse region at (cx0, cy0).  Per fine cell, with (I, tx) of its column
 *   and (J, ty) of its row, w0 = 1.0 - t:
 *   bot = w0x*e[J][I] + tx*e[J][I+1]; top = w0x*e[J+1][I] + tx*e[J+1][I+1];
 *   v = w0y*bot + ty*top; u = u + v.  All four coarse cells are always read:
 *   e on the coarse region and its 1-wide ring, corners included.  x0 and
 *   y0 >= 1, cx0 and cy0 >= 1, lde >= cx0 + mx + 1, ld >= x0 + nx.
 * Both: asynchronous on `stream`, no contraction, bitwise the same on both
 * backends; 0 with nothing launched for an empty region; refused (non-zero)
 * with a NULL plan or field, a small origin or a short pitch.  The path
 * queries follow gmt_mg_restrict_path / gmt_mg_prolong_add_path. */
int gmt_mg_restrict_tab(const void* plan, int64_t x0, int64_t y0, const double* d, int64_t ldd, double* sc,
                        int64_t cx0, int64_t cy0, int64_t ldc, void* stream);
int gmt_mg_prolong_add_tab(const void* plan, int64_t x0, int64_t y0, const double* e, int64_t cx0, int64_t cy0,
                           int64_t lde, double* u, int64_t ld, void* stream);
int gmt_mg_restrict_tab_path(int64_t x0, int64_t cx0, const double* d, int64_t ldd, const double* sc, int64_t ldc);
int gmt_mg_prolong_add_tab_path(int64_t x0, const double* e, int64_t lde, const double* u, int64_t ld);

/* ---- Temporal-blocking Jacobi (csrc/kernels/jacobi5tb.hip): `sweeps` fused
 *      Laplace sweeps per memory pass, un = J^sweeps(u), on up to 8 output
 *      rects {x0, nx, y0, ny} (absolute array coordinates, x0 >= sweeps,
 *      y0 >= sweeps, x0+nx+sweeps <= ld, y0+ny+sweeps <= nrows; u must hold
 *      each rect plus its sweeps-wide ring).  `dom` = the rank's interior
 *      {x0, nx, y0, ny}.  halo_mask bit0/1/2/3 = west/east/south/north ghost
 *      cells belong to a neighbour (they get the intermediate updates); a
 *      clear bit means a fixed Dirichlet ghost.  Cells of `un` outside the
 *      rects are never written.  Sweep counts: 1..10 (one wave per strip)
 *      and even 12..GMT_TB_MAX_SWEEPS (two waves per strip, levels split; K = 22
 *      and 24 exceed the register file at 2 waves per SIMD and are not built);
 *      gmt_jacobi5tb_supported() says which. */
#define GMT_TB_MAX_SWEEPS 20
typedef struct gmt_tb_opts {
  int sweeps;   /* K, see gmt_jacobi5tb_supported */
  int wg_waves; /* 256-column strips per workgroup, 1..8 (0 = default: four
                   one-stage strips for K <= 10; for K > 10 one two-stage
                   strip, two (stage-major waves) for a one-rect pass
                   larger than 2^28 points; at most 4 when K > 10) */
  int seg_rows; /* output rows per strip segment (0 = default: short edge
                   segments where a rect touches a Dirichlet row, interior
                   segments sized to fill the device's resident workgroups) */
  int exact;    /* 1: multiply by 1/4 per level (bitwise for any magnitude);
                   0: power-of-two scaled levels (bitwise unless a value is
                   subnormal or |u| * 4^K overflows) */
  /* Completion signal (0 = none): the workgroups of rects[0 .. signal_rects)
     — non-empty rects, given short segments — are dispatched first, and the
     last of them to finish adds 1 to *signal once their output is visible
     device-wide, while the rest of the launch still runs.  A stream can wait
     for it with gmt_signal_wait.  signal_count: a zeroed arrival counter
     (reset by the last arrival); both in GMT_SPACE_FLAGS memory. */
  int signal_rects;
  unsigned* signal_count;
  uint64_t* signal;
  /* Row bands (0 = none): rect signal_rects (the first rect after the
     signalling ones) keeps its S / N halo sides' segments separate, walks
     the N ones bottom-up, and dispatches all of them first; each of their
     output waves counts once toward the same signal after storing its
     first signal_rows output rows — the rect's signal_rows-deep row bands
     are ready long before the rect is.  No extra workgroups (the band
     rects of signal_rects each cost a pipeline warm-up and launch slots). */
  int signal_rows;
  /* Compute units the launch's stream may not use (a CU-masked stream, see
     gmt_rt_stream_create_cumask): the segment planner sizes the launch for
     the resident workgroups of the remaining ones (0 = every CU). */
  int reserved_cus;
  /* Column bands (0 = none; bit 0 W, bit 1 E): the first / last strip
     group of rect signal_rects — every one of its segments, full length —
     is dispatched before the rest of the launch and each of its workgroups
     counts toward the same signal when done: the rect's W / E halo columns
     are ready after the first round of workgroups, with no band rects of
     their own (no extra strips, segments or pipeline warm-ups). */
  int signal_cols;
  /* Inline halo exchange ("push", 0 = off): the pass stores its output's
     face cells a second time, straight into the ghost cells of the
     neighbours' NEXT input field — no pack, copy or exchange kernel.  For
     direction d (GMT_PUSH_S .. GMT_PUSH_NE), output cell (x, y) of a face
     goes to push[d] + (y * ld + x) doubles (the engine folds the
     neighbour's buffer and the translation into push[d]; IPC-mapped memory
     of another process or device, or this rank's own other buffer on a
     periodic axis); NULL = no neighbour that way.  Faces: rows [y0, y0 +
     push_w) to S, [y1 - push_w, y1) to N, columns [x0, x0 + push_w) to W,
     [x1 - push_w, x1) to E, their w x w intersections to the diagonals, of
     the one rect (which must be `dom`).  Needs: push_w even and <= 64;
     two strips or more when both W and E are pushed (a strip pushes one
     x face; a shared hand-off group always has two windows or more); the
     segment planner keeps every segment clear of one of the S / N faces;
     no completion signal options; rects of even width or wider than a
     strip (no odd-edge stores).  A push pass runs the per-strip kernel
     unless shared hand-off groups are asked for explicitly (`shared`).
     Every argument of a push pass is fixed per buffer parity, and so are
     those of the hand-over that follows it (gmt_push_sync_dev keeps its
     epoch in memory): pass + hand-over can be captured into a hipGraph. */
  const double* push[8];
  int push_w;
  /* Inline-halo passes only (push_w > 0): a device word (NULL = none) that a
     timed-out hand-over sets (gmt_push_sync / gmt_push_sync_dev `stop`); while it is non-zero
     every workgroup of the pass returns at entry — its ghost cells are
     stale and a late neighbour may still be writing them — and the job
     fails at its next synchronisation. */
  const unsigned* stop;
  /* Shader-clock record (NULL = none): one sampled wave per 256 workgroups
     adds its s_memtime delta (shader cycles) to clock[0], its
     s_memrealtime delta (the 100 MHz constant clock) to clock[1] and 1 to
     clock[2] (device memory, zeroed by the caller): the clock the pass ran
     at is clock[0] / clock[1] x 100 MHz. */
  uint64_t* clock;
  /* Shared hand-off groups (csrc/kernels/jacobi5tb.hpp Sh<K>): K = 12, 16,
     20 passes of one rect at least a group wide (920 columns at K = 20),
     with no signals or wg_waves, run as workgroups of four strips
     whose stage-1 waves read windows of one shared hand-off row — 6% fewer
     level updates per output at K = 20.  Bitwise the same field.
     -1 = off, 1 = on (four-strip groups), 2 / 4 = on with groups of that
     many strips (448 / 920 output columns at K = 20), 0 = default: four-
     strip groups where both x sides exchange halos, two-strip groups for
     other rects of 2^28 points or more (GMT_TB_SHARED=0 / 1 / 2 / 4 forces it).
     An inline-halo pass (push_w > 0) takes groups only when asked for
     explicitly (shared or GMT_TB_SHARED = 1 / 2 / 4): the first window of
     the first group then pushes the W face, the last window of the last
     group the E face.  With 0 (and GMT_TB_SHARED unset), for a rect
     narrower than a group, or where no push-group kernel is built
     (gmt_jacobi5tb_push_shared_supported) it runs the per-strip push kernel. */
  int shared;
} gmt_tb_opts;
enum { GMT_PUSH_S = 0, GMT_PUSH_N = 1, GMT_PUSH_W = 2, GMT_PUSH_E = 3,
       GMT_PUSH_SW = 4, GMT_PUSH_SE = 5, GMT_PUSH_NW = 6, GMT_PUSH_NE = 7 };
int gmt_jacobi5tb_supported(int sweeps);
/* gmt_jacobi5tb_supported and an inline-halo (gmt_tb_opts.push) kernel is built */
int gmt_jacobi5tb_push_supported(int sweeps);
/* Largest sweep count whose kernel runs without scratch: GMT_TB_MAX_SWEEPS
 * for the scaled form, 18 with exact = 1 (planners stay at or below it). */
int gmt_jacobi5tb_max_sweeps(int exact);
int gmt_jacobi5tb(const gmt_tb_opts* opts, int n_rect, const int64_t* rects, const int64_t* dom,
                  int halo_mask, const double* u, double* un, int64_t ld, int64_t nrows, void* stream);
/* The launch gmt_jacobi5tb would make, without launching: info = {workgroups,
 * resident workgroups on the device, threads per workgroup, rows per interior
 * segment and interior segments of rects[0], VGPRs per lane}. */
/* Output columns one workgroup of the fused kernel covers (strips per
 * workgroup x output columns per strip) for `sweeps` and wg_waves (0 = default). */
int64_t gmt_jacobi5tb_group_cols(int sweeps, int wg_waves);
int gmt_jacobi5tb_plan(const gmt_tb_opts* opts, int n_rect, const int64_t* rects, const int64_t* dom,
                       int halo_mask, int64_t ld, int64_t nrows, int64_t info[6]);
/* Column geometry of the shared hand-off group kernel for `sweeps` and
 * `strips` (2 or 4) per group: out = {GOUT output columns of a group, ML
 * columns from the group's first window to its first output column, NL levels
 * per stage, O first stage-1 window's offset, S0 / S1 stage-0 / stage-1 window
 * spacing, kJW / kJE lane slots of the two one-column Dirichlet keep bodies}.
 * Non-zero when no group kernel exists for (sweeps, strips). */
int gmt_jacobi5tb_shared_geom(int sweeps, int strips, int64_t out[8]);
/* An inline-halo (gmt_tb_opts.push) kernel in shared hand-off groups of
 * `strips` (2 or 4) strips is built for `sweeps`. */
int gmt_jacobi5tb_push_shared_supported(int sweeps, int strips);
/* The strips per shared hand-off group (2 or 4) gmt_jacobi5tb would launch
 * for these options and rects, or 0 for a per-strip launch: the launcher's own
 * decision, inline-halo passes included; nothing is launched.  (A workgroup
 * of 256 threads is a two-strip group or two plain strips: gmt_jacobi5tb_plan
 * cannot tell them apart.) */
int gmt_jacobi5tb_shared_path(const gmt_tb_opts* opts, int n_rect, const int64_t* rects, int halo_mask);

/* One-workgroup kernel on `stream`: waits until *signal > *seen (a
 * gmt_tb_opts completion signal), then advances *seen by one — a stream
 * ordered wait that replays correctly in a hipGraph.  Gives up after
 * GMT_WAIT_TIMEOUT_MS of device wall clock (default 10 s) and sets bit 2 of
 * *err.  All three in GMT_SPACE_FLAGS memory. */
int gmt_signal_wait(const uint64_t* signal, uint64_t* seen, unsigned* err, void* stream);

/* Hand-over between two inline-halo passes (gmt_tb_opts.push), one launch
 * on `stream` after the pushing pass: for every direction d set in `mask`,
 * stores `epoch` into *remote[d] (this rank's flag slot in the neighbour's
 * memory, IPC-mapped; system-scope release), then waits until local[d] >=
 * epoch (the neighbour's faces are in this rank's ghost cells) and acquires
 * on every XCD.  Each wait is bounded by GMT_WAIT_TIMEOUT_MS of device wall
 * clock (default 10 s); an expired one ORs 1 << d into *err (host-visible)
 * and into *stop (device memory, may be NULL: the gmt_tb_opts.stop word of
 * the following passes, which then return at once) and gives up.  While
 * *stop is non-zero the hand-over neither signals nor waits, so a stalled
 * neighbour stops the whole job within one wait instead of one per pass.
 * local / remote: GMT_SPACE_FLAGS memory.  The epoch is a launch argument:
 * the caller counts the hand-overs, and a captured launch would replay a
 * stale one (gmt_push_sync_dev is the form for hipGraphs). */
int gmt_push_sync(const uint64_t* local, uint64_t* const remote[8], int mask, uint64_t epoch, unsigned* err,
                  unsigned* stop, void* stream);

/* gmt_push_sync with the epoch in memory: the hand-over of epoch e = *epoch
 * + 1, read at entry by each of the launch's 8 workgroups; the last one to
 * finish (counted in *arrivals) stores e into *epoch and zeroes *arrivals.
 * The launch's arguments are then the same for every pass, so one captured
 * launch replays as the hand-over of every later pass, and eager and
 * replayed hand-overs mix freely (the engine uses this form for both).
 * epoch / arrivals: this rank's own words in device or GMT_SPACE_FLAGS
 * memory, zeroed before the first hand-over, touched by nothing else;
 * successive launches are ordered by the stream.  A launch that finds *stop
 * non-zero touches neither word.  mask == 0 launches nothing and leaves
 * *epoch alone.  err / stop / the wait bound: as gmt_push_sync. */
int gmt_push_sync_dev(const uint64_t* local, uint64_t* const remote[8], int mask, uint64_t* epoch,
                      unsigned* arrivals, unsigned* err, unsigned* stop, void* stream);

/* Test hook: the XCD (XCC_ID) each of n one-wave workgroups of a single
 * launch ran on, out[i] for workgroup i (device memory).  gmt_push_sync's
 * per-XCD acquire relies on workgroups i < 8 landing on 8 distinct XCDs. */
int gmt_xcd_of_workgroups(int n, unsigned* out, void* stream);

/* ---- Stream-ordered IPC exchange (csrc/kernels/ipc.hip), one launch per
 *      exchange of a persistent plan: e = *epoch + 1.  Send channel: wait
 *      until *wait >= e - 2 (receiver done with the slot), copy src -> dst +
 *      (e & 1) * dst_stride.  Receive channel: wait until *wait >= e
 *      (sender's slot ready), copy src + (e & 1) * src_stride -> dst.  When
 *      all send (receive) channels are copied, e is stored into each of their
 *      non-NULL *signal flags (system-scope release); when everything is
 *      done, *epoch = e.  Flags: GMT_SPACE_FLAGS memory; wait flags local,
 *      signal flags may be IPC-mapped memory of another process or device.
 *      Each wait is bounded by GMT_WAIT_TIMEOUT_MS of device wall clock
 *      (default 10 s); one that expires stores 1 + its channel index (sends
 *      first, then receives) into *err and gives up — the host must read
 *      *err after synchronising and treat non-zero as a failed exchange. */
typedef struct gmt_ipc_chan {
  const void* src;
  void* dst;
  int64_t bytes;
  int64_t src_stride; /* parity offsets (bytes): slot e & 1 */
  int64_t dst_stride;
  const uint64_t* wait;
  uint64_t* signal;
  /* strided side (a halo face moved in place, Transport::takes_blocks): the
     message is runs of src_run / dst_run bytes, src_ld / dst_ld bytes apart;
     run 0 = contiguous.  The staging slot side is always contiguous: a
     channel with src_run != 0 and dst_run != 0 is refused. */
  int64_t src_run, src_ld, dst_run, dst_ld;
} gmt_ipc_chan;
typedef struct gmt_ipc_plan {
  void* table;         /* device memory of gmt_ipc_table_bytes(n_send + n_recv) bytes */
  uint64_t* epoch;     /* device word, zero before the first exchange */
  unsigned* counters;  /* 3 device words, zero before the first exchange */
  unsigned* err;       /* host-visible (pinned) word, zero = no timeout */
  int n_send, n_recv;          /* filled by gmt_ipc_plan_init */
  int64_t send_chunks, recv_chunks;
} gmt_ipc_plan;
int64_t gmt_ipc_table_bytes(int n_chan);
/* Writes the channel table (synchronous copy) and the chunk counts; any
 * number of channels.  table/epoch/counters/err must be set by the caller.
 * Refused (non-zero, the same on both backends): a NULL table, n_send + n_recv == 0, a negative count, bytes or
 * run; for a strided side ld < run, bytes % run != 0 or bytes > 0xffffffff
 * (the kernel's 32-bit division); both sides strided. */
int gmt_ipc_plan_init(gmt_ipc_plan* plan, int n_send, const gmt_ipc_chan* sends, int n_recv,
                      const gmt_ipc_chan* recvs);
int gmt_ipc_exchange(const gmt_ipc_plan* plan, void* stream);

/* ---- Kernel-driven host staging (csrc/kernels/stage.hip): one launch copies
 *      every chunk src -> dst (device memory -> page-locked host memory the
 *      GPU maps; or the reverse): gmt_stage_copy's `wgs` workgroups each take
 *      their slice of chunk 0, then of chunk 1, ... (chunks complete in
 *      order); gmt_stage_scatter runs wgs_per_chunk per chunk.  Once chunk k is
 *      complete and visible system-wide, `value` is stored into flags[k]
 *      (GMT_SPACE_PINNED_COHERENT memory) so the host can hand chunk k to MPI
 *      while later chunks are still being copied.  The chunk table and the
 *      per-chunk arrival counters (zero between launches) are device memory.
 *      A chunk with rows > 0 is strided on its field side: it is the packed
 *      doubles [first, first + bytes/8) of a column-major block of `rows`
 *      doubles per column at pitch `ld` doubles starting at `block` (a halo
 *      face read straight out of the field: no separate pack launch, no
 *      device send buffer).  gmt_stage_copy gathers such a chunk from
 *      `block` into dst; gmt_stage_scatter writes src into `block` (a
 *      received chunk from page-locked memory straight into the ghost rows;
 *      rows == 0: a plain copy src -> dst). */
typedef struct gmt_stage_chunk {
  const void* src;
  void* dst;
  int64_t bytes;
  int64_t rows, ld, first; /* strided field side (rows == 0: contiguous) */
  double* block;
} gmt_stage_chunk;
int gmt_stage_copy(int n_chunks, const gmt_stage_chunk* chunks, unsigned* counters, uint64_t* flags,
                   uint64_t value, int wgs, void* stream);
int gmt_stage_scatter(int n_chunks, const gmt_stage_chunk* chunks, int wgs_per_chunk, void* stream);

/* One kernel per entry point: the variants the defaults were chosen against
 * are measured by csrc/bench/variant_bench.hip, not shipped in this ABI. */

/* ---- misc */
const char* gmt_error_string(int err);
int gmt_device_synchronize(void);
const char* gmt_build_info(void);

#ifdef __cplusplus
}
#endif
#endif /* GMT_KERNELS_H */
