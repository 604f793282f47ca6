/*
 * gmt/engine.h — C ABI of the native Jacobi engine (libgmt_engine.so).
 *
 * The Python package drives the flagship benchmark through this ABI
 * (gpu_mpi_tests_amd/engine.py): torch.distributed does the rendezvous and
 * broadcasts a 128-byte id, then every step runs in C++ (hipGraph replay of
 * halo exchange + sweeps) with no Python on the critical path.  Transports:
 *   RCCL  one rank per GPU, xGMI; the id is an RCCL unique id;
 *   IPC   several ranks per GPU allowed (GPU oversubscription, the
 *         reference's mpi_daxpy.cc:43-54 mode) or one per GPU; HIP IPC
 *         mappings traded once over a Unix-socket mesh of the node named by
 *         the id (gmt_engine_control_id), one kernel launch per exchange;
 *   LOCAL one rank, no id.
 * No MPI in this library.
 */
#ifndef GMT_ENGINE_H
#define GMT_ENGINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum gmt_engine_transport { GMT_ENGINE_LOCAL = 0, GMT_ENGINE_RCCL = 1, GMT_ENGINE_IPC = 2 };

/* fills 128 bytes (an RCCL unique id); returns 0 or an error code */
int gmt_engine_unique_id(void* out128);
/* fills 128 bytes: the name of a socket control plane (GMT_ENGINE_IPC) */
int gmt_engine_control_id(void* out128);
/* Engine options (explicit fields; 0 = default everywhere). */
typedef struct gmt_engine_opts {
  int periodic; /* 1: periodic process grid, else Dirichlet (fixed ghost ring) */
  int overlap;  /* 0 off, 1 halo exchange overlapped with the core pass, 2 auto (time both once) */
  int graph;    /* 1: capture the per-parity passes into hipGraphs */
  int tsteps;   /* sweeps per fused pass and per halo exchange: 0 or 1 = single sweeps, else
                   2..GMT_TB_MAX_SWEEPS (odd values above 10 are rounded down to even) */
  int wg_waves; /* temporal-blocking kernel: waves per workgroup (0 = auto) */
  int seg_rows; /* temporal-blocking kernel: output rows per workgroup (0 = auto) */
  int exact;    /* -1 / 0: power-of-two scaled levels when the field bound allows (auto),
                   1: always the exact 1/4-per-level form */
  int init;     /* initial field: 0 = x^3 + y^2 on the global lattice, 1 = uniform [0, 1)
                   random (a hash of the global lattice point and `seed`) */
  int calibrate; /* 1: prepare() times every fused-pass size on the real share and the
                    planner uses those costs instead of the built-in table */
  int64_t seed;
  int push;     /* 1: inline halo exchange of the fused passes (JacobiConfig::push) */
  int shared;   /* gmt_tb_opts.shared of the fused passes, inline-halo ones included
                   (JacobiConfig::tb_shared): -1, 0 (default), 1, 2 or 4 */
  int source;   /* Poisson source term of the sweep (JacobiConfig::source): 0 none, 1 poly,
                   2 uniform random in [-source_amp, source_amp), 3 supplied by the host
                   (gmt_engine_jacobi_set_source) */
  int src_every; /* sweeps per source block with tsteps > 1: 0 = tsteps, else a positive
                    multiple of tsteps */
  double source_amp; /* amplitude of source 2 (finite, >= 0) */
} gmt_engine_opts;
/* id: 128 bytes (RCCL unique id / control id) or NULL (local); NULL on invalid options */
void* gmt_engine_jacobi_create(int64_t ny, int64_t nx, int py, int px, int rank, int world,
                               int transport, const void* ccl_id, const gmt_engine_opts* opts);
void gmt_engine_jacobi_destroy(void* h);
int gmt_engine_jacobi_run(void* h, int steps); /* enqueue `steps` steps */
int gmt_engine_jacobi_sync(void* h);
double gmt_engine_jacobi_residual(void* h);
int gmt_engine_jacobi_exchange(void* h); /* one blocking halo exchange */
/* {sqrt(sum over ranks of d^2), max over ranks of |d|} of d = J(u) - u on the
 * current field; read-only: the field and the sweep count are unchanged
 * (JacobiSolver::residual_norm).  Collective. */
int gmt_engine_jacobi_residual_norm(void* h, double out[2]);
/* Solve to tolerance (JacobiSolver::solve, gmt/jacobi.hpp SolveOpts /
 * SolveResult): r <= max(tol, rtol * r0) in the chosen norm, checked every
 * check_every sweeps, the host deciding `lag` checks behind the device. */
typedef struct gmt_engine_solve_opts {
  double tol, rtol; /* at least one positive */
  int norm;         /* 0 L2, 1 max */
  int max_sweeps;   /* a positive multiple of check_every */
  int check_every;  /* 0 = tsteps */
  int lag;          /* 0..8 */
} gmt_engine_solve_opts;
typedef struct gmt_engine_solve_result {
  int converged, sweeps, checks, residual_sweeps;
  double residual, residual_max, r0;
  int failed; /* 1: a non-finite residual stopped the solve */
} gmt_engine_solve_result;
/* 0, or 1 on invalid options (nothing enqueued).  Collective. */
int gmt_engine_jacobi_solve(void* h, const gmt_engine_solve_opts* opts, gmt_engine_solve_result* out);
/* Conjugate gradients from the current field (JacobiSolver::cg, gmt/jacobi.hpp
 * CgOpts / CgResult): the same criterion and lagged check; tol == rtol == 0
 * runs exactly max_iters iterations. */
typedef struct gmt_engine_cg_opts {
  double tol, rtol;
  int norm;        /* 0 L2, 1 max */
  int max_iters;   /* a positive multiple of check_every */
  int check_every; /* 0 = 10 */
  int lag;         /* 0..8 */
} gmt_engine_cg_opts;
typedef struct gmt_engine_cg_result {
  int converged, iters, checks, residual_iters;
  double residual, residual_max, r0, true_residual, true_residual_max;
  int failed; /* 1: a non-finite residual stopped the iteration */
} gmt_engine_cg_result;
/* 0; 1 on invalid options, 2 on an engine with a periodic axis (nothing
 * enqueued either way).  Collective. */
int gmt_engine_jacobi_cg(void* h, const gmt_engine_cg_opts* opts, gmt_engine_cg_result* out);
/* Chebyshev semi-iteration from the current field (JacobiSolver::cheby,
 * gmt/jacobi.hpp ChebyOpts / ChebyResult): cg's criterion, lagged check and
 * fixed-count mode; one halo exchange and one kernel per iteration. */
typedef struct gmt_engine_cheby_opts {
  double tol, rtol;
  int norm;        /* 0 L2, 1 max */
  int max_iters;   /* a positive multiple of check_every */
  int check_every; /* 0 = 10 */
  int lag;         /* 0..8 */
  double rho;      /* 0 = the closed form, else finite and in (0, 1) */
} gmt_engine_cheby_opts;
typedef struct gmt_engine_cheby_result {
  int converged, iters, checks, residual_iters;
  double residual, residual_max, r0, rho;
  int failed; /* 1: a non-finite residual stopped the iteration */
} gmt_engine_cheby_result;
/* 0; 1 on invalid options, 2 on an engine with a periodic axis (nothing
 * enqueued either way).  Collective. */
int gmt_engine_jacobi_cheby(void* h, const gmt_engine_cheby_opts* opts, gmt_engine_cheby_result* out);
/* the closed-form spectral radius of an nx x ny global interior */
double gmt_engine_cheby_rho(int64_t nx_global, int64_t ny_global);
/* Geometric multigrid V-cycles from the current field (JacobiSolver::mg,
 * gmt/jacobi.hpp MgOpts / MgResult): an iteration is one cycle, cg's
 * criterion, lagged check and fixed-count mode. */
typedef struct gmt_engine_mg_opts {
  double tol, rtol;
  int norm;         /* 0 L2, 1 max */
  int max_cycles;   /* a positive multiple of check_every */
  int check_every;  /* 0 = 1 */
  int lag;          /* 0..8 */
  int nu1, nu2;     /* damped Jacobi sweeps before / after the correction, nu1 + nu2 > 0 */
  double omega;     /* in (0, 1] */
  int max_levels;   /* 0 = no limit, else >= 2 */
  int coarse_iters; /* 0 = gmt_engine_mg_coarse_iters(rho of the coarsest level) */
  int coarsen;      /* 0 nested (nx + 1 and ny + 1 even on every level), 1 any lattice size (MgOpts::coarsen) */
  int fuse;         /* 0, or 2..4: sweeps of a smoothing run per memory pass (MgOpts::fuse) */
  int smoother;     /* 0 damped Jacobi, 1 red-black Gauss-Seidel (MgOpts::smoother); omega is taken as given */
  int fuse_resid;   /* 1: residual and restriction in one pass where a level allows it (MgOpts::fuse_resid) */
  int fuse_prolong; /* 1: the interpolation inside the first post-smoothing pass where a level allows it
                     * (MgOpts::fuse_prolong) */
} gmt_engine_mg_opts;
typedef struct gmt_engine_mg_result {
  int converged, iters, checks, residual_iters;
  double residual, residual_max, r0;
  int failed; /* 1: a non-finite residual stopped the iteration */
  int levels;
  int64_t coarse_ny, coarse_nx; /* global extents of the coarsest level */
  int coarse_iters;
  double coarse_rho;
  int fuse, fuse_fine, fuse_levels; /* as requested; the depth of level 0; levels with a depth >= 2 */
  int smoother;                     /* as requested */
  int fuse_resid, resid_levels;     /* as requested; the levels whose residual and restriction ran fused */
  int resid_mask;                   /* bit l: level l is one of them */
  int fuse_prolong, prolong_levels; /* as requested; the levels whose interpolation ran inside the smoothing pass */
  int prolong_mask;                 /* bit l: level l is one of them */
} gmt_engine_mg_result;
/* 0; 1 on invalid options, 2 on an engine with a periodic axis, 3 when the
 * problem has no coarse level: nx + 1 or ny + 1 odd, 4 when a rank of the
 * process grid would own no coarse point (nothing enqueued in any of these).
 * Collective. */
int gmt_engine_jacobi_mg(void* h, const gmt_engine_mg_opts* opts, gmt_engine_mg_result* out);
/* the default Chebyshev iteration count on a coarsest level of spectral radius rho */
int gmt_engine_mg_coarse_iters(double rho);
/* global {ny, nx} of every level of an ny x nx problem on a py x px grid into
 * out[2 * max] (level 0 first); returns the number of levels */
int gmt_engine_mg_levels(int64_t ny, int64_t nx, int py, int px, int max_levels, int64_t* out, int max);
/* the same under gmt_engine_mg_opts.coarsen (0: the table above); -1 on a bad argument */
int gmt_engine_mg_levels2(int64_t ny, int64_t nx, int py, int px, int max_levels, int coarsen, int64_t* out,
                          int max);
/* 1 or 0 per restricting level: its residual and restriction fuse under gmt_engine_mg_opts.fuse_resid on an
 * engine of ghost depth `ghost` (gmt::mg_resid_levels) into out[max]; returns their number, -1 on a bad argument */
int gmt_engine_mg_resid_levels(int64_t ny, int64_t nx, int py, int px, int ghost, int max_levels, int coarsen,
                               int* out, int max);
/* 1 or 0 per level that interpolates: it runs gmt_mg_prolong_smooth under gmt_engine_mg_opts.fuse_prolong with
 * these fuse, nu2 and smoother on an engine of ghost depth `ghost` (gmt::mg_prolong_levels) into out[max]; returns
 * their number, -1 on a bad argument */
int gmt_engine_mg_prolong_levels(int64_t ny, int64_t nx, int py, int px, int ghost, int fuse, int nu2, int smoother,
                                 int max_levels, int coarsen, int* out, int max);
/* the depth of every smoothing level under gmt_engine_mg_opts.fuse on an engine of ghost depth `ghost`
 * (gmt::mg_fuse_depths) into out[max]; returns their number, -1 on a bad argument */
int gmt_engine_mg_fuse_depths(int64_t ny, int64_t nx, int py, int px, int fuse, int ghost, int max_levels,
                              int coarsen, int* out, int max);
/* 1 when the engine has a periodic axis */
int gmt_engine_jacobi_periodic(void* h);
/* out[16]: nx, ny, off_x, off_y, bytes_per_exchange, messages, graph, overlap, py, px, tsteps,
 * overlap_auto ns per pass with overlap, without (0 if not tuned), exact arithmetic in use,
 * band-first passes, inline halo exchange in use */
int gmt_engine_jacobi_info(void* h, int64_t* out);
/* Which passes replay from hipGraphs: bit 0 = the single sweeps, bit 1 = the
 * full fused passes (tsteps sweeps; inline-halo passes with their hand-over).
 * 0 without `graph`, on the CPU backend, or after a failed capture. */
int gmt_engine_jacobi_graphs(void* h);
/* The fused passes (sweeps per pass, in launch order) that run(steps) enqueues:
 * writes min(n, max) entries, returns n. */
int gmt_engine_jacobi_plan(void* h, int steps, int* out, int max);
/* The launch of the rank's one-rect K-sweep pass (gmt_jacobi5tb_plan's
 * info[6]); returns its error code. */
int gmt_engine_jacobi_tb_info(void* h, int K, int64_t* out);
/* Strips per shared hand-off group (2 or 4) of that pass, 0 for a per-strip
 * launch (gmt_jacobi5tb_shared_path). */
int gmt_engine_jacobi_tb_shared(void* h, int K);
/* Launch one pass of every pass type run(steps) will use, then restore the
 * initial field (first-launch costs stay out of a timed run). */
int gmt_engine_jacobi_prepare(void* h, int steps);
int gmt_engine_jacobi_copy_interior(void* h, double* host);
/* Source 3: this rank's share of the sweep source, row-major [ny][nx] (the
 * reverse of copy_interior); recomputes the block field and restores the
 * initial field (JacobiSolver::set_source).  Only before the first sweep;
 * collective.  0, or 1 not a source-3 engine / NULL, 2 a sweep has run, 3 the
 * source is too large for the scaled levels (create with exact = 1). */
int gmt_engine_jacobi_set_source(void* h, const double* host);
/* What run(steps) enqueues on a source engine: out = {blocks, sweeps per block,
 * single source sweeps after them} (JacobiSolver::source_plan; all zero
 * without a source).  gmt_engine_jacobi_plan keeps describing Laplace passes:
 * a block's are those of plan(out[1]). */
int gmt_engine_jacobi_source_plan(void* h, int steps, int out[3]);
/* what: 0 = max |u| of the initial field (all ranks; drives the exactness
 * guard), 1 = measured ms of a full tsteps pass (0 before a calibrated
 * prepare), 2 = the built-in cost table's ms for that pass on this share,
 * 3 = max |s| of the source over all ranks, 4 / 5 = wall-clock ms / sweeps of
 * the last set-up of the source block field, 6 = device bytes of the source
 * and block fields */
/* bitwise comparison of the current interiors of two engines of the same
 * problem and process grid (collective): out[0] = max |diff| over ranks,
 * out[1] = elements whose bits differ, summed over ranks */
int gmt_engine_jacobi_compare(void* a, void* b, double* out);
/* gmt::plan_pass_sequence on given costs (cost[0..ks], ms per K-sweep pass):
 * the sweeps per pass, written to out[0..max); returns the plan length */
int gmt_engine_plan_from_costs(int k, int ks, const double* cost, int measured, int* out, int max);
/* reset != 0: zero the fused passes' clock record (stream ordered); else
 * out[3] = {shader MHz, samples, seconds sampled} since the last reset */
int gmt_engine_jacobi_clock(void* h, int reset, double* out);
double gmt_engine_jacobi_stat(void* h, int what);
const char* gmt_engine_backend(void);

/* A bare communicator on the same transports, for device collectives outside
 * the engine (bench.py's DAXPY partial-sum all-reduce, BASELINE config 3).
 * allreduce: in-place sum of n doubles in device memory, ordered on `stream`,
 * complete on return. */
void* gmt_engine_comm_create(int rank, int world, int transport, const void* id);
int gmt_engine_comm_allreduce_sum(void* h, double* buf, int64_t n, void* stream);
const char* gmt_engine_comm_name(void* h);
void gmt_engine_comm_destroy(void* h);
/* Hang watchdog (gmt/watchdog.hpp): armed by the first engine entry point
 * when GMT_TIMEOUT=<seconds> is set; the process exits with status 124 and a
 * "GMT WATCHDOG: rank R ... last phase '<phase>'" line when no phase mark
 * arrives for that long.  A caller marks progress of its own phases here. */
void gmt_engine_watchdog_kick(const char* phase);
double gmt_engine_watchdog_timeout(void); /* 0 when not armed */
/* Last words: when the watchdog fires, write `json` (an object) to stdout with
 * a "watchdog" field naming the stall and exit with `code` instead of 124; ""
 * exits with `code` silently; NULL restores the default. */
void gmt_engine_watchdog_epitaph(const char* json, int code);

/* The reference's halo-exchange benchmark (mpi_stencil2d_gt test_deriv for
 * dim 0 and dim 1, then test_sum), n_local x n_other per rank, 2 ghosts,
 * non-periodic 1-D slabs, on the RCCL or IPC transport (local for world == 1).
 * out[18]: per dim d (6 values at 6*d): exchange seconds median, mean, min,
 * max, bytes sent per exchange, this rank's err_norm; out[12] = all-reduce
 * (1024 doubles in place) median seconds, out[13] = its max relative error;
 * out[14 + d] = norm of the analytic derivative over this rank's output;
 * out[16 + d] = ghost cells found wrong after some exchange (check != 0: the
 * ghost rows are compared with the analytic field after EVERY exchange,
 * gmt/deriv.hpp; -1 without check). */
int gmt_engine_deriv_bench(int64_t n_local, int64_t n_other, int n_iter, int n_warmup, int rank,
                           int world, int transport, const void* ccl_id, double* out, int check);
/* The two derivative tests of gmt_engine_deriv_bench as whole steps
 * (exchange + derivative through to completion) in two orders, interleaved
 * (gmt/deriv.hpp DerivConfig::overlap): the serial one, and the exchange on
 * a high-priority stream beside the interior of the derivative, then the
 * ghost-dependent bands.  out[12]: per dim d (6 values at 6*d): serial step
 * median seconds, overlapped step median seconds, err_norm of the last
 * (overlapped) step, the largest err_norm of any overlapped step (check != 0;
 * else -1), ghost cells found wrong (check != 0; else -1), norm of the
 * analytic derivative. */
int gmt_engine_deriv_step_bench(int64_t n_local, int64_t n_other, int n_iter, int n_warmup, int rank,
                                int world, int transport, const void* ccl_id, double* out, int check);

#ifdef __cplusplus
}
#endif
#endif /* GMT_ENGINE_H */
