// gmt/jacobi.hpp — distributed 2-D 5-point Jacobi solver (native engine).
//
// The BASELINE workload "mpi_stencil2d 32768² on 8 GPUs (2×4 decomp), halo
// exchange/interior overlap" and its single-GPU 8192² point.  The reference
// itself only times halo exchanges around a derivative stencil, serialised
// against compute (mpi_stencil2d_gt.cc:511-535); this engine is the
// MI355X-first version of that loop:
//
//   * 2-D Cartesian decomposition (py x px ranks), ghost width 1 (2 with
//     tblock), fp64;
//   * one step = halo exchange of u + one Jacobi sweep u -> un + swap;
//   * overlap: single sweeps — the interior "core" sweep runs on the compute
//     stream while the halo (fused pack kernel + RCCL/IPC/MPI transfer +
//     unpack) runs on a high-priority comm stream; the 1-2 cell boundary
//     frame is swept after the halo lands (gmt_jacobi5_rects).  Fused
//     passes run band-first: the boundary bands of the pass finish first
//     and signal, and the exchange of the pass's OUTPUT runs under the rest
//     of it (enqueue_block);
//   * graph: with a stream-ordered transport (rccl, ipc, local) both step
//     parities are captured into hipGraphs and replayed — one host call per
//     step, so small per-GPU domains (strong scaling at 8 GPUs) are not
//     launch-bound.  Fused passes are captured too, per parity: the serial
//     pass with its exchange, the band-first pass with its forked exchange,
//     and the inline-halo pass (push) with its hand-over, whose epoch lives
//     in device memory (gmt_push_sync_dev) so a replay hands over the right
//     one.  Partial passes (fewer sweeps than tsteps) stay eager.
//
//   * tblock: K = tsteps sweeps per kernel and per exchange (temporal
//     blocking): u(t) is read once and u(t+K) written once (gmt_jacobi5tb,
//     csrc/kernels/jacobi5tb.hip), the halo is K wide and exchanged once per pass with its
//     corners (one-phase exchange) — bitwise the same result as K single
//     sweeps.
// Storage is column-major (x contiguous) with the interior origin at x = 8
// so every interior row starts 64-B aligned and the sweep kernels take their
// 16-B vector path; the row pitch is padded to 64 doubles.
#pragma once

#include <functional>
#include <memory>
#include <utility>
#include <vector>

#include "gmt/buffer.hpp"
#include "gmt/halo.hpp"
#include "gmt/kernels.h"
#include "gmt/transport.hpp"

namespace gmt {

struct JacobiConfig {
  int64_t ny_global = 8192, nx_global = 8192;  // global interior extent
  int py = 1, px = 1;                            // process grid (rank = cy*px + cx)
  bool periodic = false;                         // else Dirichlet (fixed ghost ring)
  int periodic_axes = 3;                         // with periodic: bit0 wraps x (W/E), bit1 wraps y (S/N)
  bool overlap = true;
  // overlap_auto: time a few fused passes with and without overlap at
  // construction (then restore the initial field) and keep the faster — the
  // same choice on every rank (the per-pass times are averaged over ranks).  Whether hiding the
  // exchange pays for the frame pass depends on the link (self-exchange on
  // one GPU: serial 4-8 % faster, profiles/r01_frame.md); measure it.
  bool overlap_auto = false;
  bool graph = false;
  // temporal blocking: tsteps (2-24) sweeps per memory pass (gmt_jacobi5tb;
  // odd counts above 10 round down) and per halo exchange (ghost width
  // tsteps, corners in the same
  // exchange phase) — 1/tsteps of the HBM bytes and messages per lattice
  // update.  1 = off.  tblock = true with tsteps = 0 is tsteps = 2.
  bool tblock = false;
  int tsteps = 0;
  int wg_waves = 0;                              // gmt_tb_opts.wg_waves: strips per workgroup (0 = auto)
  int seg_rows = 0;                              // gmt_tb_opts.seg_rows (0 = auto)
  // -1 / 0: power-of-two scaled levels when max|u| * 4^K stays finite (the
  // initial field bounds every later one: Jacobi averages; max|u| is
  // measured on the device at start-up), 1: always exact
  int exact = -1;
  // initial field (interior and Dirichlet ring): 0 = x^3 + y^2 on the global
  // lattice (gmt_fill_poly mode 4), 1 = uniform [0, 1) random values, a hash
  // of the global lattice point and `seed` (mode 5) — both independent of the
  // decomposition, so every process grid computes the same numbers
  int init = 0;
  uint64_t seed = 0;
  // prepare() times one pass of every fused-pass size on this rank's real
  // share (max over ranks) and plan_passes uses those costs instead of the
  // built-in table (measured on one box for one kernel revision)
  bool calibrate = false;
  // Inline halo exchange (fused passes; gmt_tb_opts.push): every pass
  // stores its output faces straight into the neighbours' ghost cells of
  // their next input (IPC mappings traded over the transport's control
  // plane; this rank's own buffers on a periodic axis), then one small
  // hand-over launch (gmt_push_sync_dev) replaces the halo exchange.  With
  // `graph`, pass and hand-over replay from one hipGraph per parity.  Needs a
  // transport with a control plane (ipc) unless every neighbour is this
  // rank; off (the transport's exchange as before) when the share is too
  // small for the kernel's push rules.
  bool push = false;
  // gmt_tb_opts.shared of every fused pass, inline-halo ones included: -1 no
  // shared hand-off groups, 0 the kernel's default (an inline-halo pass then
  // runs the per-strip kernel), 1 / 4 four-strip groups, 2 two-strip groups.
  // Each rank decides its own launch: a share narrower than a group keeps
  // the per-strip kernel.
  int tb_shared = 0;
  // Poisson source term: a sweep is un = 1/4 ((W + E) + (S + N)) + s with a
  // fixed field s (for -Laplace(u) = f on a mesh of width h: s = h^2/4 f).
  // source: 0 none (Laplace: exactly the code paths of an engine without this
  // option), 1 poly (gmt_fill_poly mode 7: the s for which init 0's
  // x^3 + y^2 is the discrete fixed point), 2 uniform random in
  // [-source_amp, source_amp) (mode 6, seed `seed + 1`), 3 supplied by the
  // host (set_source; zero until then).
  // With tblock the fused Laplace passes stay as they are, by superposition:
  // a sweep is affine in (u, ring, s), so for a block of n sweeps
  //   u(t+n) = L^n(u(t)) + g_n,
  // L^n = n Laplace sweeps with the real ring (the fused passes, bitwise),
  // g_n = n source sweeps from a zero field with a zero ring, computed once
  // at set-up.  run(k) is k / src_every blocks — the passes of
  // plan_passes(src_every), then one streaming add of g (gmt_add2d, 24 B per
  // point) — and k % src_every single source sweeps.  src_every: sweeps per
  // block, 0 = tsteps, a positive multiple of tsteps; ignored without tblock
  // (every sweep is then a single source sweep).
  int source = 0;
  double source_amp = 1.0;
  int src_every = 0;
};

// JacobiSolver::solve: sweep until the residual d = J(u) - u of the current
// field meets r <= max(tol, rtol * r0) in the chosen norm (r0: the residual of
// the field the solve starts from), or max_sweeps have run.
struct SolveOpts {
  double tol = 0.0, rtol = 0.0;  // at least one must be positive
  int norm = 0;                  // 0: L2 (sqrt of the global sum of d^2), 1: max |d|
  int max_sweeps = 0;            // the cap: a positive multiple of check_every
  int check_every = 0;           // sweeps between two checks (0 = tsteps)
  int lag = 1;                   // the host decides on check i - lag after enqueuing check i (0..8)
};
// What solve(), cg() and cheby() report of their lagged checks.  An iteration
// is a sweep for solve(), a CG or Chebyshev iteration for the other two.
struct CheckResult {
  int converged = 0;        // the criterion was met
  int iters = 0;            // iterations run: residual_iters + lag * check_every unless the cap came first
  int checks = 0;           // checks enqueued
  int residual_iters = 0;   // iteration count of the deciding check
  double residual = 0.0;    // its residual in the chosen norm (cg: the recursive one),
  double residual_max = 0.0;  // its max |d|,
  double r0 = 0.0;          // and the residual of the starting field (chosen norm)
  int failed = 0;           // 1: a non-finite residual stopped the iteration
};
using SolveResult = CheckResult;

// JacobiSolver::cg: conjugate gradients on A u = b, A = I - J (J the Laplace
// sweep; symmetric positive definite on a Dirichlet interior, the ring and the
// source in b).  The residual r = b - A u is cell for cell the d of
// residual_norm; the criterion and the lagged host check are solve()'s.
struct CgOpts {
  double tol = 0.0, rtol = 0.0;  // both 0: fixed-count mode, exactly max_iters iterations
  int norm = 0;                  // 0: L2 (sqrt of the global sum of r^2), 1: max |r|
  int max_iters = 0;             // the cap: a positive multiple of check_every
  int check_every = 0;           // iterations between two checks (0 = 10)
  int lag = 1;                   // the host decides on check i - lag after enqueuing check i (0..8)
};
struct CgResult : CheckResult {
  double true_residual = 0.0;      // residual_norm() of the final field: L2,
  double true_residual_max = 0.0;  // and max
};

// JacobiSolver::cheby: Chebyshev semi-iteration over the sweep G (Golub-Varga),
//   u_1 = G(u_0);  u_{k+1} = u_{k-1} + w_{k+1} * (G(u_k) - u_{k-1}),
//   w_2 = 1/(1 - rho^2/2),  w_{k+1} = 1/(1 - rho^2 w_k/4),
// rho the spectral radius of J with a zero ring on the global interior
// (cheby_rho).  CG's order of convergence with the communication of one single
// sweep: a 1-wide halo exchange and one kernel per iteration, no reductions.
// The residual is not monotone from one iteration to the next; "converged"
// means what solve() means, the first check that meets the criterion.
struct ChebyOpts {
  double tol = 0.0, rtol = 0.0;  // both 0: fixed-count mode, exactly max_iters iterations
  int norm = 0;                  // 0: L2, 1: max |d|
  int max_iters = 0;             // the cap: a positive multiple of check_every
  int check_every = 0;           // iterations between two checks (0 = 10)
  int lag = 1;                   // the host decides on check i - lag after enqueuing check i (0..8)
  // 0: the closed form.  Otherwise finite and in (0, 1): an over-estimate
  // converges more slowly, an under-estimate can stagnate.
  double rho = 0.0;
};
struct ChebyResult : CheckResult {
  double rho = 0.0;         // the spectral radius used
};
// 0.5*(cos(pi/(nx+1)) + cos(pi/(ny+1))): the spectral radius of the Laplace
// sweep on an nx x ny interior with a zero ring
double cheby_rho(int64_t nx_global, int64_t ny_global);
// w_{k+1} from w_k (k >= 1; w_1 = 1): 1/(1 - rho2/2) for k = 1, else
// 1/(1 - rho2*w_k/4), every operation rounded once in exactly this order, so
// the weights are bit for bit Python's given the same rho
double cheby_next_weight(double rho2, double w, int k);

// JacobiSolver::mg: geometric multigrid V-cycles on (I - J) u = b.  Levels are
// vertex-centred: a level with global interior ny x nx has the coarser level
// (ny-1)/2 x (nx-1)/2, coarse point (J, I) on fine interior point (2J+1, 2I+1);
// a rank that owns fine columns [ox, ox+nx) owns coarse columns
// [ox/2, (ox+nx)/2), rows alike (mg_level_table).  One cycle on a level:
//   coarsest: u = 0, coarse_iters Chebyshev iterations (the first the plain
//             sweep, weights of cheby_next_weight, rho = cheby_rho of the level);
//   else:     nu1 damped Jacobi sweeps u' = u + omega*(G(u) - u), each after a
//             1-wide faces-only exchange; d = G(u) - u; the ring of d exchanged
//             with corners; s_coarse = full weighting of d (weights summing to
//             4: the coarse levels run the same operator, c0 = 0.25, c1 = 1);
//             u_coarse = 0; the cycle on the coarser level; the ring of
//             u_coarse exchanged with corners; u += bilinear interpolation of
//             u_coarse; nu2 sweeps.
// The fine ring is the real Dirichlet ring, coarse rings are zero.  An
// iteration is one cycle; criterion and lagged check are solve()'s.
//
// coarsen = 1 ("any") drops the nesting: each axis of each level is coarsened
// on its own to m = mg_coarse_extent(n) points on the same interval, (n-1)/2
// for odd n and n/2 - 1 for even n (8192 -> 4095 -> 2047 -> ... -> 1), with the
// same rediscretised operator on every level.  A level whose two axes are odd
// is the nested level above, kernels and all; any other level transfers by
// linear interpolation P with position-dependent weights and its exact
// transpose (gmt_mg_prolong_add_tab / gmt_mg_restrict_tab, tables of
// gmt/mg_tab.hpp, an odd axis being the table with weights 0.5 / 1 / 0.5):
// coarse point J belongs to the rank that owns fine cell floor(J*(n+1)/(m+1)),
// and the residual of such a level is exchanged 2 wide with corners.  Set-up
// computes every rank's needs from the tables: a level on which a coarse point
// would have other than 3 or 4 taps per axis, a tap more than 2 cells or an
// interpolated coarse cell more than 1 outside a rank's share, or a rank with
// a neighbour and fewer than 2 cells on that axis, is not created, and the
// hierarchy stops there.  The two hierarchies are built apart and never mixed.
struct MgOpts {
  double tol = 0.0, rtol = 0.0;  // both 0: fixed-count mode, exactly max_cycles cycles
  int norm = 0;                  // 0: L2, 1: max |d|
  int max_cycles = 0;            // the cap: a positive multiple of check_every
  int check_every = 0;           // cycles between two checks (0 = 1)
  int lag = 1;                   // the host decides on check i - lag after enqueuing check i (0..8)
  int nu1 = 2, nu2 = 2;          // sweeps before / after the coarse-level correction
  double omega = 0.8;            // the damping, in (0, 1]
  int max_levels = 0;            // 0: as many as the extents and the process grid allow; else >= 2
  int coarse_iters = 0;          // Chebyshev iterations on the coarsest level (0 = mg_coarse_iters(rho))
  int coarsen = 0;               // 0 nested; 1 any: every lattice size (both above)
  int fuse = 0;                  // 0, or 2..GMT_MG_MAX_FUSE: sweeps of a smoothing run per memory pass (below)
  int smoother = 0;              // 0 damped Jacobi; 1 red-black Gauss-Seidel (below)
  int fuse_resid = 0;            // 1: residual and restriction in one memory pass where a level allows it (below)
  int fuse_prolong = 0;          // 1: the interpolation inside the first post-smoothing pass where a level allows it
};
struct MgResult : CheckResult {
  int levels = 0;                          // levels used, the fine one included
  int64_t coarse_ny = 0, coarse_nx = 0;    // global extents of the coarsest
  int coarse_iters = 0;                    // Chebyshev iterations on it
  double coarse_rho = 0.0;                 // and their spectral radius
  int fuse = 0;                            // MgOpts::fuse as requested
  int fuse_fine = 1;                       // the depth of level 0 (1: it smooths sweep by sweep)
  int fuse_levels = 0;                     // smoothing levels with a depth >= 2
  int smoother = 0;                        // MgOpts::smoother as requested
  int fuse_resid = 0;                      // MgOpts::fuse_resid as requested
  int resid_levels = 0, resid_mask = 0;    // the levels that ran gmt_mg_resid_restrict, and bit l for level l
  int fuse_prolong = 0;                    // MgOpts::fuse_prolong as requested
  int prolong_levels = 0, prolong_mask = 0;  // the levels that ran gmt_mg_prolong_smooth, and bit l for level l
};
// MgOpts::fuse > 0 runs the sweeps of a smoothing run through gmt_mg_smooth_k,
// up to `fuse` of them per memory pass, for the same bits.  Every smoothing
// level l has a depth d_l, computed from global data only: the largest
// d <= fuse such that, on each axis of the process grid with more than one
// rank, every rank owns at least d cells of the level; on level 0 d <= the
// engine's ghost depth too when the grid has more than one rank (an engine
// with tsteps = 1 keeps its fine level unfused on several ranks, its coarse
// levels fuse).  A run of n sweeps is chunks of min(n, d_l): a chunk of two or
// more is one d_l-wide exchange of the current buffer with corners and one
// gmt_mg_smooth_k whose halo sides are the sides with a neighbour; a chunk of
// one is the single sweep above.  A level with neighbours keeps the
// (d_l - 1)-wide ring of its source current: exchanged after each restriction
// on coarse levels, once per source on level 0.  The coarse levels of such a
// call have GMT_MG_MAX_FUSE ghost rows and columns (one hierarchy per coarsen
// mode, built apart from the fuse = 0 ones, whose layout is unchanged).
// MgOpts::smoother = 1 smooths with red-black Gauss-Seidel (gmt_mg_smooth_rb).
// A cell of a level is red iff the sum of its 1-based global indices on that
// level's lattice is even; a sweep is the red half-sweep, then the black one
// (omega is the cell's, 1.0 for plain Gauss-Seidel).  A run of n sweeps is 2n
// half-sweeps in the chunks above with half-sweeps for sweeps: a chunk of two
// or more is one d_l-wide exchange with corners and one gmt_mg_smooth_rb, a
// chunk of one the 1-wide faces-only exchange and one launch with h = 1.  par
// comes from the rank's global offset on the level and the half-sweeps the run
// has done, so the field does not depend on the process grid.  Depths, halo
// plans, source rings, residual, transfers and the coarsest level are the same.
// MgOpts::fuse_resid = 1 replaces, on a restricting level, the ring exchange,
// the residual (gmt_cg_apply mode 1 into the field d), the exchange of d's ring
// and the restriction by one 2-wide exchange of the current buffer with
// corners and one gmt_mg_resid_restrict whose halo sides are the sides with a
// neighbour, for the same bits.  A level fuses iff its transfer is not
// table-driven, there is one rank or every rank owns at least 2 cells of the
// level on each axis the process grid shares, and, on level 0 of several
// ranks, the engine's ghost depth is at least 2; the other levels run the
// launches above.  A function of global shapes only.  Such a call uses the
// hierarchy of fused calls whatever `fuse` is, keeps the 1-wide ring of the
// level's source with corners current (with fused smoothing, the wider of the
// two), and a level that fuses gets its d and d's halo plan only when a later
// call runs it unfused.
// MgOpts::fuse_prolong = 1 replaces, on a level, gmt_mg_prolong_add and the
// first chunk of the post-smoothing run by one gmt_mg_prolong_smooth, for the
// same bits.  With n2 = nu2 sweeps (2 nu2 half-sweeps for red-black) and
// c = min(n2, d_l), level l fuses iff nu2 >= 1, its transfer is not
// table-driven, and there is one rank or every rank owns at least c/2 + 1
// cells of level l + 1 on each axis the process grid shares.  A function of
// global shapes only.  After the coarser level returns, its field is exchanged
// c/2 + 1 wide with corners (1 wide today); the c-deep halo of u must hold the
// neighbours' values before the correction, and u has not changed since the
// residual: a level that fuses its residual too widens that exchange to
// max(2, c), c = 1 needs nothing more than the ring the residual left current,
// and otherwise one c-wide exchange with corners runs before the launch.
// The launch computes the c sweeps or half-sweeps with par as the run would;
// the other n2 - c go through the run's chunks unchanged.  Such a call uses
// the hierarchy of fused calls whatever `fuse` is.
// 1 or 0 for each level that interpolates (the coarsest level has none).
std::vector<int> mg_prolong_levels(int64_t ny, int64_t nx, int py, int px, int ghost, int fuse, int nu2, int smoother,
                                   int max_levels, int coarsen);
// 1 or 0 for each restricting level (the coarsest level has none).
std::vector<int> mg_resid_levels(int64_t ny, int64_t nx, int py, int px, int ghost, int max_levels, int coarsen);
// The depth of each smoothing level (the coarsest level has none).
std::vector<int> mg_fuse_depths(int64_t ny, int64_t nx, int py, int px, int fuse, int ghost, int max_levels,
                                int coarsen);
// The default coarse_iters: with sigma = (1 - sqrt(1 - rho^2))/rho and t = sigma,
// the smallest k >= 1 with 2t/(1 + t^2) <= 0.1, t multiplied by sigma each
// time k grows by one; 1 for rho = 0.
int mg_coarse_iters(double rho);
// Global extents {ny, nx} of every level, the fine one first: coarsening goes
// on while nx + 1 and ny + 1 are even, every rank of the py x px grid keeps at
// least one coarse row and column, and max_levels (0: no limit) is not
// reached.  A function of the global extents and block_split only: every rank
// computes the same table.
std::vector<std::pair<int64_t, int64_t>> mg_level_table(int64_t ny, int64_t nx, int py, int px, int max_levels);
// The same for MgOpts::coarsen (0: the table above, bit for bit).
std::vector<std::pair<int64_t, int64_t>> mg_level_table(int64_t ny, int64_t nx, int py, int px, int max_levels,
                                                        int coarsen);

class JacobiSolver {
 public:
  JacobiSolver(comm::Transport& t, const JacobiConfig& c);
  ~JacobiSolver();
  JacobiSolver(const JacobiSolver&) = delete;
  JacobiSolver& operator=(const JacobiSolver&) = delete;

  void step();  // one sweep, asynchronous (compute stream)
  // k sweeps through the fused kernel (plan_passes) when tblock; with a source
  // and tblock: blocks of src_every sweeps (source_plan)
  void run(int k);
  // cheapest sequence of fused passes (sweeps per pass <= tsteps) covering k sweeps
  std::vector<int> plan_passes(int k) const;
  void synchronize();
  // sqrt(global sum (u_{k+1} - u_k)^2) of one extra sweep (advances the solution)
  double residual();
  // {sqrt(global sum d^2), global max |d|} of d = J(u) - u on the current
  // field, read-only (gmt_jacobi5_resid): the field, its parity and the sweep
  // count are unchanged.  A halo exchange it has to make is the next pass's
  // (fresh_).  Collective; synchronises the compute stream.
  void residual_norm(double out[2]);
  // Convergence-driven run: check i (the residual kernel, its two all-reduces,
  // an async copy into a page-locked ring, an event) is enqueued after
  // i * check_every sweeps, run(check_every) between checks, and the host
  // waits for the event of check i - lag only: with lag >= 1 the device never
  // idles for a check.  Every rank decides on the all-reduced values of the
  // same check.  Throws std::invalid_argument on bad options (nothing enqueued).
  SolveResult solve(const SolveOpts& o);
  // Conjugate gradients from the current field, the solution updated in place
  // (same buffer, same parity: run(k) afterwards keeps sweeping from it and
  // captured graphs stay valid).  One iteration is a 1-wide halo exchange of
  // the search direction, three kernels (gmt_cg_apply / _update / _dir, the
  // step lengths computed on the device) and two all-reduces; check i is
  // copied into the page-locked ring after i * check_every iterations and
  // decided `lag` checks behind, as solve() does.  The first call builds the
  // state (three fields, a halo plan: collective).  Throws
  // std::invalid_argument on bad options or an engine with a periodic axis
  // (A is singular there); nothing is enqueued then.
  CgResult cg(const CgOpts& o);
  // Chebyshev semi-iteration from the current field (ChebyOpts above).  One
  // iteration is a 1-wide faces-only exchange of the current buffer's ring,
  // one launch (the first of a call the plain sweep, later ones
  // gmt_cheby_step with that iteration's weight by value, writing u_{k+1} over
  // u_{k-1} in the other buffer) and the parity flip of step(), in serial
  // order on the compute stream.  Check i is solve()'s (the read-only residual
  // of the current field after i * check_every iterations), decided `lag`
  // checks behind.  Every cell's arithmetic is independent of the
  // decomposition: the field is bitwise the same on every process grid.
  // Every call restarts the recurrence from the current field; run(k)
  // afterwards keeps sweeping from it and captured graphs stay valid.  The
  // first call builds two halo plans (collective).  Throws
  // std::invalid_argument on bad options or an engine with a periodic axis
  // (rho = 1, the fixed point is not unique); nothing is enqueued then.
  ChebyResult cheby(const ChebyOpts& o);
  // Multigrid V-cycles from the current field (MgOpts above).  The solution
  // replaces the current field and the parity flips as in step() (with an odd
  // nu1 + nu2); run(k) afterwards keeps sweeping from it and captured graphs
  // stay valid.  A source enters as the fine level's f.  Every cell's
  // arithmetic is independent of the decomposition: the field is bitwise the
  // same on every process grid.  The first call builds the level hierarchy
  // (coarse fields, one fine field, halo plans: collective).  Throws
  // std::invalid_argument, nothing enqueued, on bad options, an engine with a
  // periodic axis, or a problem with no coarse level (nx + 1 or ny + 1 odd, or
  // a rank that would own no coarse point).
  MgResult mg(const MgOpts& o);
  // one blocking halo exchange of the current field (latency measurements);
  // ordered after every pass already enqueued
  void exchange_only();
  // launch one pass of every pass type run(k) uses, then restore the initial
  // field: first-launch costs (code object, occupancy query) stay out of a
  // timed run(k)
  void prepare(int k);
  // Source kind 3: this rank's share of s, row-major [ny][nx] (host memory,
  // the reverse of copy_interior).  Recomputes the block field and restores
  // the initial field.  Only before the first sweep (or after a prepare());
  // collective.  0, or non-zero with nothing changed: 1 not a kind-3 engine or
  // a NULL pointer, 2 a sweep has run, 3 the source is too large for the
  // scaled levels of the fused passes (construct with exact = 1).
  int set_source(const double* host_interior);
  // What run(k) enqueues on a source engine: {blocks, sweeps per block, single
  // source sweeps after them}; {0, 0, k} with a source and no tblock, all zero
  // without a source.  plan_passes keeps describing Laplace passes: those of
  // one block are plan_passes(src_every).
  void source_plan(int k, int out[3]) const;
  int source() const { return cfg_.source; }
  bool periodic() const { return cfg_.periodic && (cfg_.periodic_axes & 3) != 0; }
  int src_every() const { return src_every_; }
  double max_abs_source() const { return smax_; }
  // sweeps and wall-clock ms of the last set-up of the block field; its and
  // the source field's device bytes
  int source_setup_sweeps() const { return src_setup_sweeps_; }
  double source_setup_ms() const { return src_setup_ms_; }
  size_t source_bytes() const { return f_.bytes() + gsrc_.bytes(); }
  bool exact() const { return exact_; }
  // local interior, row-major [ny][nx] (host memory)
  void copy_interior(double* host) const;
  // Bitwise comparison of the current interiors of two solvers of the same
  // global problem and process grid, on the device (gmt_diff_bits):
  // out[0] = max |diff| (max over ranks), out[1] = elements whose bits differ
  // (sum over ranks).  bench.py's check of the timed run replays the timed
  // sweeps through single sweeps and compares (reference: the err_norm of the
  // timed field, mpi_stencil2d_gt.cc:541-570).  Collective.
  void compare(JacobiSolver& o, double out[2]);
  // Shader clock of the fused passes since the last clock_reset() (stream
  // ordered): one sampled wave per 256 workgroups stamps s_memtime and
  // s_memrealtime (gmt_tb_opts.clock).  out = {MHz (0 without samples or on
  // the CPU backend), samples, seconds sampled}.  GMT_CLOCK=0: no stamps.
  void clock_reset();
  void clock_read(double out[3]);
  // The launch of this rank's one-rect K-sweep pass (the serial or inline-
  // halo pass over the interior), without launching: gmt_jacobi5tb_plan's
  // {workgroups, resident workgroups, threads per workgroup, segment rows,
  // segments, VGPRs}.  Returns its error code (0: ok).
  int tb_launch_info(int K, int64_t out[6]) const;
  // strips per shared hand-off group of that pass (gmt_jacobi5tb_shared_path), 0: per-strip
  int tb_shared_strips(int K) const;

  int64_t nx() const { return nx_; }
  int64_t ny() const { return ny_; }
  int64_t off_x() const { return ox_; }
  int64_t off_y() const { return oy_; }
  size_t bytes_per_exchange() const { return halo_[0] ? halo_[0]->bytes_sent() : 0; }
  size_t messages() const { return halo_[0] ? halo_[0]->messages() : 0; }
  bool graph_active() const { return graph_[0] != nullptr || graph2_[0] != nullptr; }
  bool sweep_graph_active() const { return graph_[0] != nullptr; }  // the single sweeps replay
  // the full fused passes (inline-halo ones with their hand-over) replay from hipGraphs
  bool fused_graph_active() const { return graph2_[0] != nullptr; }
  bool tblock() const { return ks_ > 1; }
  int tsteps() const { return ks_; }
  int ghost() const { return g_; }
  bool overlap_active() const { return push_on_ || (cfg_.overlap && halo_[0] && halo_[0]->active()); }
  // the fused passes exchange their halo inline (cfg_.push took effect)
  bool push_active() const { return push_on_; }
  // the fused passes overlap band-first (enqueue_block)
  bool band_first() const { return ks_ > 1 && band_mode(ks_); }
  const Neighbors& neighbors() const { return nb_; }
  // overlap_auto: seconds per pass measured {overlap, serial} (mean over ranks), 0 if not tuned
  double tuned_overlap_s() const { return tune_s_[0]; }
  double tuned_serial_s() const { return tune_s_[1]; }
  // ms per fused pass of k sweeps: measured by prepare() with calibrate (0 if
  // not), and the built-in table's estimate for this share
  double measured_pass_ms(int k) const { return k >= 0 && k <= GMT_TB_MAX_SWEEPS ? meas_ms_[k] : 0.0; }
  double table_pass_ms(int k) const;
  double max_abs_u0() const { return umax_; }
  gmt_stream_t stream() const { return s_; }

 private:
  void enqueue_step(int parity);
  void enqueue_block(int parity, int k);  // k <= ks_ fused sweeps
  // one fused k-sweep launch on `n` output rects (gmt_jacobi5tb)
  void xk_launch(int k, int n, const int64_t* rects, int parity, int sig_rects, int sig_rows,
                 gmt_stream_t st = nullptr, int sig_cols = 0);
  // the band-first pass's rect (the interior) and its column / row bands
  bool band_rects(int k, int64_t* rects, int* sig_cols, int* sig_rows) const;
  bool band_mode(int k) const;  // the fused k-sweep pass runs band-first (overlap)
  void exchange_now(int parity);  // blocking-order halo exchange of buf_[parity] on the compute stream
  void step_block();
  void sweep_full(int parity, double* resid);
  void capture_graphs();
  void init_field();
  void autotune_overlap();
  void calibrate_costs();
  double measure_max_abs();
  int halo_mask() const;
  void split_cus();
  void setup_push();
  // {sum d^2, max |d|} over every rank into rn_dev_, stream-ordered on s_;
  // ring_current: the 1-wide faces of the current buffer were just exchanged
  void enqueue_residual(bool ring_current = false);
  void rn_setup();          // rn_ws_, rn_dev_, the ring and its events (first use)
  void allreduce_sum_max(double* pair);  // {sum, max} -> the same bits on every rank
  // the halo plan of the 1-wide faces around the interior of `field` (collective)
  std::unique_ptr<Halo2D> faces_halo(double* field);
  // the lagged check loop of solve(), cg() and cheby() (jacobi.cpp)
  struct CheckLoop;
  void run_checks(const CheckLoop& c, CheckResult& res, const std::function<void()>& advance,
                  const std::function<const double*(int)>& check);
  void cg_setup();          // the state of cg() (first use; collective)
  void cheby_setup();       // the halo plans of cheby() (first use; collective)
  // the ring of a field, `width` cells wide, with corners, or its faces only (collective)
  std::unique_ptr<Halo2D> ring_halo(double* field, int64_t xo, int64_t yo, int64_t nx, int64_t ny, int64_t ld,
                                    bool corners, int width = 1);
  void mg_setup();          // the levels of mg() for mgh_ (first use; collective)
  void mg_fuse_setup(int levels, const MgOpts& o);  // depths, fused transfers and what they need (collective)
  // n sweeps on level l, fused where its depth allows; the first `done` sweeps (red-black: half-sweeps) have run
  void mg_smooth_run(int l, int n, const MgOpts& o, int done = 0);
  void mg_cycle(int l, int levels, const MgOpts& o, int coarse_iters, double coarse_rho);
  void mg_ring(int l);      // the faces of level l's current buffer hold the neighbours' current values
  void maybe_corrupt(int parity);  // GMT_CORRUPT_PASS fault injection
  void push_block(int parity, int k);  // one inline-halo pass + its hand-over
  void push_pass(int parity, int k);   // the pass launch alone
  void push_handover();                // the hand-over launch alone (push_mask_ != 0)
  void run_laplace(int k);             // k sweeps of the Laplace operator through plan_passes(k)
  void fill_source();                  // f_ of kinds 1 and 2, zero for kind 3
  double measure_max_source();         // max |s| over every rank (gmt_abs_max)
  bool source_bound_ok(double smax, int k) const;  // (max|u0| + 2^31 smax) * 4^k stays finite
  // the kernels' f, ldf, c1: the source field with c1 = 1, or none
  const double* src_f() const { return f_.data(); }
  int64_t src_ld() const { return f_.data() ? ld_ : 0; }
  double src_c1() const { return f_.data() ? 1.0 : 0.0; }
  void build_block_field();            // gsrc_ = src_every_ source sweeps from zero, then init_field()
  void add_block_field();              // current interior += gsrc_ (gmt_add2d on s_)

  comm::Transport& t_;
  JacobiConfig cfg_;
  int64_t nx_ = 0, ny_ = 0, ox_ = 0, oy_ = 0;  // local interior + global offset
  int64_t xo_ = 8, yo_ = 1, ld_ = 0;           // interior origin (absolute), row pitch
  int g_ = 1;                                  // ghost width
  int ks_ = 1;                                 // sweeps per fused pass
  bool exact_ = false;                         // gmt_tb_opts.exact for the fused passes
  Neighbors nb_;
  Buffer<double> buf_[2];
  // source engines (cfg_.source != 0), both in buf_'s layout: the sweep
  // source s (the kernels' f with c1 = 1) and the block field g of src_every_
  // sweeps; allocated before capture_graphs, never reallocated
  Buffer<double> f_, gsrc_;
  int src_every_ = 0;     // sweeps per block; 0: no blocks (no source, or no tblock)
  double smax_ = 0.0;     // max |s| over every rank
  bool advanced_ = false;  // a sweep has run since the field was (re)initialised
  int src_setup_sweeps_ = 0;
  double src_setup_ms_ = 0.0;
  std::unique_ptr<Halo2D> halo_[2];
  Buffer<double> resid_ws_;
  // residual_norm / solve: the kernel's workspace, its device result and the
  // page-locked ring of check results with one event per slot (made on first use)
  static constexpr int kMaxLag = 8;
  Buffer<double> rn_ws_, rn_dev_, rn_ring_;
  gmt_event_t rn_ev_[kMaxLag + 1] = {};
  // cg(): residual, search direction and A p in buf_'s layout; the halo of p
  // (width 1, faces only); the kernels' workspace; device scalars {sum, max}:
  // rr by iteration parity at [0..1] and [2..3], p.q at [4..5]
  Buffer<double> cg_r_, cg_p_, cg_q_, cg_ws_, cg_sc_;
  std::unique_ptr<Halo2D> cg_halo_;
  // cheby(): the 1-wide ring of either buffer's interior (faces only)
  std::unique_ptr<Halo2D> cheby_halo_[2];
  // mg(): level 0 is buf_ and f_ with cheby_halo_ (u, s and the pair of halo
  // plans below stay empty there); coarser levels own their fields in buf_'s
  // layout (interior origin x = 8, y = 1, pitch padded to 64, a zero ring);
  // the hierarchies of fused calls (mg_[2], mg_[3]) give them
  // GMT_MG_MAX_FUSE ghost rows and columns (y = 4, 4 columns right of the interior)
  struct MgLevel {
    int64_t ny_g = 0, nx_g = 0;                        // global interior
    int64_t nx = 0, ny = 0, ox = 0, oy = 0;            // this rank's share and its global offset
    int64_t xo = 8, yo = 1, ld = 0;                    // interior origin, pitch
    Buffer<double> u[2], s, d;                         // d: the residual (none on the last level)
    // the transfer to the next level is table-driven: d then has its own
    // layout (interior origin (xo, dyo), pitch dld, room for a 2-wide ring)
    bool tab = false;
    int64_t dyo = 1, dld = 0;
    std::unique_ptr<void, void (*)(void*)> plan{nullptr, gmt_mg_xfer_plan_destroy};
    double* up[2] = {nullptr, nullptr};                // the level's buffer pair
    const double* sp = nullptr;                        // its source (level 0: NULL without one)
    int cur = 0;                                       // up[cur] is the level's current field
    bool ring = false;                                 // its faces are current
    std::unique_ptr<Halo2D> hu[2], hd;                 // rings with corners of u[0], u[1] and d
    // fused smoothing (MgOpts::fuse): the smallest share of any rank on this
    // level, the depth of the running call, and the w-wide rings with corners
    // of either buffer and of the source, made on first use
    int64_t min_nx = 0, min_ny = 0;
    int depth = 1;
    // MgOpts::fuse_resid: the level runs gmt_mg_resid_restrict in this call; the width at which the ring of its
    // source is kept current; the doubles of d, allocated when a call first needs it
    bool resid = false;
    int sw = 0;
    // MgOpts::fuse_prolong: the level runs gmt_mg_prolong_smooth in this call, with pc sweeps or half-sweeps
    bool prolong = false;
    int pc = 0;
    size_t delems = 0;
    std::unique_ptr<Halo2D> hk[2][GMT_MG_MAX_FUSE + 1], hs[GMT_MG_MAX_FUSE];
    double* hk_field[2] = {nullptr, nullptr};
  };
  std::vector<MgLevel> mg_[4];  // by MgOpts::coarsen, + 2 for the layout of a fused call
  int mgc_ = 0;                 // the coarsening of the running mg()
  int mgh_ = 0;                 // the hierarchy it uses
  int f_ring_ = 0;              // f_'s ring is current this wide (fused mg() on several ranks)
  Buffer<double> mg_ws_;  // gmt_cg_apply's workspace and its two results (level 0's size)
  Buffer<uint64_t> sig_;  // band-first completion signal (GMT_SPACE_FLAGS)
  bool fresh_[2] = {false, false};  // buf_[b]'s ghost ring holds the neighbours' current values
  gmt_stream_t s_ = nullptr, cs_ = nullptr;
  // band-first passes on split compute units (split_cus): the pass on sb_
  // (all but a few CUs), the exchange on cs_ (those few), so the exchange's
  // kernels start the moment the bands signal instead of waiting for the
  // pass's resident workgroups to retire
  gmt_stream_t sb_ = nullptr;
  int comm_cus_ = 0;
  // pack/unpack workgroups of the exchange a band-first pass hides
  // (Halo2D::set_pack_wgs): 0 = the full grid; GMT_PACK_WGS=N for A/B (64
  // and 128 measured no better on the N = 8 shares, profiles/r04_overlap.md)
  int beside_pack_wgs_ = 0;
  // a band-first pass was enqueued since the last synchronize(): only then
  // do the side streams and the band signal's error word need a look (a
  // D2H read and two stream syncs are ~2% of an N = 8 pass)
  bool band_ran_ = false;
  gmt_event_t ev_start_ = nullptr, ev_halo_ = nullptr, ev_band_ = nullptr;
  gmt_graph_t graph_[2] = {nullptr, nullptr};   // single sweep, per parity
  gmt_graph_t graph2_[2] = {nullptr, nullptr};  // fused ks_-sweep block, per parity
  int parity_ = 0;  // buf_[parity_] holds the current u
  int passes_ = 0;  // fused passes run() enqueued since the field was (re)initialised
  bool in_run_ = false;
  double tune_s_[2] = {0.0, 0.0};
  double meas_ms_[GMT_TB_MAX_SWEEPS + 1] = {};
  bool calibrated_ = false;
  double umax_ = 0.0;  // max |u| of the initial field over every rank
  // inline halo exchange (setup_push): per parity of the pass's INPUT, the
  // push targets (gmt_tb_opts.push) — the neighbours' other buffer with the
  // face translation folded in; the neighbours' flag slots for this rank;
  // the directions that are other ranks; the hand-over epoch and the
  // hand-over launch's arrival counter (device words: gmt_push_sync_dev)
  bool push_on_ = false;
  const double* push_base_[2][8] = {};
  uint64_t* push_remote_[8] = {};
  int push_mask_ = 0;
  Buffer<uint64_t> push_flags_;  // [d]: written by the neighbour in direction d
  Buffer<unsigned> push_err_;    // host-visible: bit d = the wait for direction d expired
  Buffer<unsigned> push_stop_;   // device word: a wait expired, later passes return at once
  Buffer<uint64_t> push_ctl_;    // device words: [0] hand-overs done (the epoch), [1] arrival counter
  Buffer<uint64_t> clk_;         // gmt_tb_opts.clock: cycles, 100 MHz ticks, samples
  std::vector<void*> push_opened_;
};

// Balanced block split of n over p parts: offset and length of part i.
inline void block_split(int64_t n, int p, int i, int64_t* off, int64_t* len) {
  const int64_t base = n / p, rem = n % p;
  *off = i * base + (i < rem ? i : rem);
  *len = base + (i < rem ? 1 : 0);
}

// The cheapest sequence of fused passes covering k sweeps, passes of at most
// ks sweeps, cost[K] = ms of a K-sweep pass (0: no such pass; K = 1 a single
// sweep); measured costs get a 2% handicap on passes shorter than ks (clock
// noise must not displace full passes).  Full passes first, then the rest,
// largest first.  JacobiSolver::plan_passes with this rank's costs.
std::vector<int> plan_pass_sequence(int k, int ks, std::vector<double> cost, bool measured);

// Process grid minimising the halo bytes per rank; strided x faces (which
// need a pack kernel) are weighted 1.5x a contiguous y face.
void choose_dims(int world, int64_t ny, int64_t nx, int* py, int* px);

}  // namespace gmt
