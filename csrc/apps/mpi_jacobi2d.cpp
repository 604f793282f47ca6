// mpi_jacobi2d — distributed 2-D 5-point Jacobi (fp64) with halo/interior
// overlap: the BASELINE stencil-MLUPS benchmark as a native MPI app.
//
// BASELINE.json configs "mpi_stencil2d 8192² fp64 single GPU" and
// "mpi_stencil2d 32768² on 8 GPUs (2×4 decomp), halo exchange/interior
// overlap".  The reference never overlaps and never reports a lattice-update
// rate; the loop it times is mpi_stencil2d_gt.cc:511-535.
//
// CLI: mpi_jacobi2d [n] [n_iter]       global n x n interior (default 8192, 100)
//   --nx=, --ny=            rectangular global domain
//   --weak                  n x n PER RANK (global = py*n x px*n)
//   --dims=PYxPX            process grid (default: minimise halo bytes)
//   --transport=auto|rccl|ipc|mpi-host|mpi-direct
//   --overlap=auto          time overlapped and serial passes once, keep the faster
//   --no-overlap --graph --periodic[=x|y] --warmup=W
//   --tblock                temporal blocking (gmt_jacobi5tb): K sweeps per memory pass
//                           and per (K-wide) halo exchange
//   --tsteps=K              sweeps per fused pass with --tblock (2-20; default 2; odd
//                           counts above 10 round down)
//   --wg-strips=N --seg-rows=L   gmt_tb_opts launch shape (0 = default)
//   --halo-iters=K          K blocking halo exchanges -> latency line
//   --push                  inline halo exchange of the fused passes (JacobiConfig::push: the
//                           pass stores its faces into the neighbours' ghost cells; ipc or
//                           a single rank)
//   --shared=N              gmt_tb_opts.shared of the fused passes, --push ones included
//                           (JacobiConfig::tb_shared: -1 no shared hand-off groups, 0 default,
//                           1 / 4 groups of four strips, 2 of two; a push pass takes groups
//                           only when asked for here)
//   --tol=T --rtol=R        solve to tolerance (JacobiSolver::solve): sweep until the residual
//                           r = |J(u) - u| meets r <= max(T, R * r0); n_iter is then the sweep
//                           cap (rounded up to a multiple of E) and the timed region is one
//                           solve() from the initial field.  Exit status 4 when the cap is hit
//                           unconverged or the residual is not finite
//   --norm=l2|max           the norm of r (default l2)
//   --check-every=E         sweeps between two residual checks (default: tsteps)
//   --lag=L                 the host decides on a check L checks behind the device (default 1,
//                           0..8): with L >= 1 the device never idles for a check
//   --source=poly|random[:AMP]   Poisson source term of the sweep, un = J(u) + s
//                           (JacobiConfig::source): poly = the s for which the initial field
//                           x^3 + y^2 is the discrete fixed point, random = uniform in
//                           [-AMP, AMP) (default 1).  With --tblock the fused passes stay
//                           Laplace passes and a block of B sweeps ends with one add
//   --src-every=B           sweeps per source block (default tsteps; a multiple of it)
//   --init=analytic|random  the initial field and Dirichlet ring (JacobiConfig::init): x^3 + y^2,
//                           or uniform [0, 1) hashed from the lattice point and --seed=S (default 0)
//   --cg                    conjugate gradients on (I - J) u = b instead of sweeps
//                           (JacobiSolver::cg; Dirichlet only): --tol / --rtol / --norm / --lag as
//                           above, --check-every=E iterations (default 10), n_iter the iteration
//                           cap (rounded up to a multiple of E).  With neither --tol nor --rtol:
//                           exactly n_iter iterations, and the time per iteration.  --check then
//                           runs the same number of iterations of the serial whole-problem CG and
//                           compares within 1e-10 * max|u0| (dot products depend on the
//                           decomposition: not bitwise)
//   --cheby [--rho=R]       Chebyshev semi-iteration over the sweep instead of sweeps
//                           (JacobiSolver::cheby; Dirichlet only, exclusive with --cg): the options
//                           of --cg; R the spectral radius of the sweep, finite and in (0, 1)
//                           (default: the closed form of the global interior; an over-estimate
//                           converges more slowly, an under-estimate can stagnate).  --check runs
//                           the same number of serial Chebyshev iterations with the same rho and
//                           compares within 1e-10 * max|u0|
//   --mg [--nu=A,B] [--omega=W] [--levels=N] [--coarse-iters=C] [--coarsen=nested|any] [--fuse=K]
//        [--smoother=jacobi|rb] [--fuse-resid] [--fuse-prolong]
//                           geometric multigrid V-cycles instead of sweeps (JacobiSolver::mg;
//                           Dirichlet only, exclusive with --cg and --cheby; nx + 1 and ny + 1 even):
//                           the options of --cg with --check-every=E cycles (default 1) and n_iter the
//                           cycle cap; A / B damped Jacobi sweeps before / after the correction
//                           (default 2,2), W their damping (default 0.8), N the number of levels
//                           (default: all), C the Chebyshev iterations on the coarsest level
//                           (default: from its spectral radius).  --check runs the same number of
//                           serial cycles and compares within 1e-10 * max|u0|.  K (0, or 2..4) runs
//                           up to K sweeps of a smoothing run in one memory pass (MgOpts::fuse) for
//                           the same bits.  --smoother=rb smooths with red-black Gauss-Seidel
//                           (MgOpts::smoother; W then defaults to 1.0, and K counts half-sweeps);
//                           only with --mg.  --fuse-resid computes the residual and its restriction
//                           in one memory pass on every level that allows it (MgOpts::fuse_resid).
//                           --fuse-prolong interpolates inside the first post-smoothing pass on every
//                           level that allows it (MgOpts::fuse_prolong)
//                           for the same bits
//   --check                 rank 0 re-runs the whole problem serially on the host
//   --json=FILE
#include <mpi.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <string>
#include <vector>

#include "gmt/comm.hpp"
#include "gmt/device.hpp"
#include "gmt/jacobi.hpp"
#include "gmt/mg_tab.hpp"
#include "gmt/util.hpp"

using namespace gmt;

// gmt_fill_poly mode 5's hash of a lattice point (csrc/kernels/reduce.hip lattice_uniform)
static double lattice_uniform(int64_t gx, int64_t gy, uint64_t seed) {
  uint64_t k = (static_cast<uint64_t>(gy + (int64_t(1) << 30)) << 32) ^ static_cast<uint64_t>(gx + (int64_t(1) << 30));
  k ^= seed;
  k += 0x9E3779B97F4A7C15ull;
  k = (k ^ (k >> 30)) * 0xBF58476D1CE4E5B9ull;
  k = (k ^ (k >> 27)) * 0x94D049BB133111EBull;
  k ^= k >> 31;
  return static_cast<double>(k >> 11) * 0x1.0p-53;
}

// The engine's sweep source over the global interior (JacobiConfig::source 1
// or 2 with `amp` and the engine's seed + 1), and its initial field with the
// ghost ring (JacobiConfig::init), (ny + 2) x (nx + 2).
static std::vector<double> serial_source(int64_t ny, int64_t nx, int source, double amp, uint64_t seed) {
  const double h = 1.0 / (static_cast<double>(ny > nx ? ny : nx) + 1);
  std::vector<double> src(ny * nx);
  for (int64_t j = 0; j < ny; ++j)
    for (int64_t i = 0; i < nx; ++i) {
      const double x = static_cast<double>(i) * h;
      src[j * nx + i] = source == 1 ? -(1.5 * x + 0.5) * h * h : amp * (2.0 * lattice_uniform(i, j, seed + 1) - 1.0);
    }
  return src;
}
static std::vector<double> serial_init(int64_t ny, int64_t nx, int init, uint64_t seed) {
  const int64_t ld = nx + 2;
  const double h = 1.0 / (static_cast<double>(ny > nx ? ny : nx) + 1);
  std::vector<double> u((ny + 2) * ld);
  for (int64_t j = 0; j < ny + 2; ++j)
    for (int64_t i = 0; i < nx + 2; ++i) {
      const double x = (i - 1) * h, y = (j - 1) * h;
      u[j * ld + i] = init == 1 ? lattice_uniform(i - 1, j - 1, seed) : x * x * x + y * y;
    }
  return u;
}

// Serial host reference of the same problem (init, boundary, update order, source).
static std::vector<double> serial_jacobi(int64_t ny, int64_t nx, int steps, bool periodic, int axes = 3,
                                         int source = 0, double amp = 1.0, uint64_t seed = 0, int init = 0) {
  const int64_t ld = nx + 2;
  std::vector<double> u = serial_init(ny, nx, init, seed), un, src;
  if (source != 0) src = serial_source(ny, nx, source, amp, seed);
  un = u;
  for (int s = 0; s < steps; ++s) {
    if (periodic && (axes & 1))
      for (int64_t j = 1; j <= ny; ++j) {
        u[j * ld] = u[j * ld + nx];
        u[j * ld + nx + 1] = u[j * ld + 1];
      }
    if (periodic && (axes & 2))
      for (int64_t i = 1; i <= nx; ++i) {
        u[i] = u[ny * ld + i];
        u[(ny + 1) * ld + i] = u[ld + i];
      }
    for (int64_t j = 1; j <= ny; ++j)
      for (int64_t i = 1; i <= nx; ++i) {
        const double* p = &u[j * ld + i];
        un[j * ld + i] = 0.25 * ((p[-1] + p[1]) + (p[-ld] + p[ld]));
        if (source != 0) un[j * ld + i] += src[(j - 1) * nx + i - 1];
      }
    std::swap(u, un);
  }
  std::vector<double> out(ny * nx);
  for (int64_t j = 0; j < ny; ++j)
    for (int64_t i = 0; i < nx; ++i) out[j * nx + i] = u[(j + 1) * ld + i + 1];
  return out;
}

// Serial conjugate gradients on the whole Dirichlet problem, the definition of
// JacobiSolver::cg (gmt/jacobi.hpp): `iters` iterations from the initial
// field, the cell expressions in the kernels' order, the dot products summed
// row by row.  *umax = max |u0| over the field and its ring.
static std::vector<double> serial_cg(int64_t ny, int64_t nx, int iters, int source, double amp, uint64_t seed,
                                     int init, double* umax) {
  const int64_t ld = nx + 2;
  std::vector<double> u = serial_init(ny, nx, init, seed), src;
  if (source != 0) src = serial_source(ny, nx, source, amp, seed);
  *umax = 0;
  for (double v : u) *umax = std::fmax(*umax, std::fabs(v));
  std::vector<double> r(u.size(), 0.0), p(u.size(), 0.0), q(u.size(), 0.0);
  double rr = 0;
  for (int64_t j = 1; j <= ny; ++j)
    for (int64_t i = 1; i <= nx; ++i) {
      const double* c = &u[j * ld + i];
      double o = 0.25 * ((c[-1] + c[1]) + (c[-ld] + c[ld]));
      if (source != 0) o = o + 1.0 * src[(j - 1) * nx + i - 1];
      const double d = o - c[0];
      r[j * ld + i] = p[j * ld + i] = d;
      rr += d * d;
    }
  for (int it = 0; it < iters; ++it) {
    double pq = 0;
    for (int64_t j = 1; j <= ny; ++j)
      for (int64_t i = 1; i <= nx; ++i) {
        const double* c = &p[j * ld + i];
        const double v = c[0] - 0.25 * ((c[-1] + c[1]) + (c[-ld] + c[ld]));
        q[j * ld + i] = v;
        pq += c[0] * v;
      }
    const double alpha = pq > 0 ? rr / pq : 0.0;
    double rn = 0;
    for (int64_t j = 1; j <= ny; ++j)
      for (int64_t i = 1; i <= nx; ++i) {
        const int64_t k = j * ld + i;
        const double tp = alpha * p[k], tq = alpha * q[k];
        u[k] = u[k] + tp;
        r[k] = r[k] - tq;
        rn += r[k] * r[k];
      }
    const double beta = rr > 0 ? rn / rr : 0.0;
    for (int64_t j = 1; j <= ny; ++j)
      for (int64_t i = 1; i <= nx; ++i) {
        const int64_t k = j * ld + i;
        const double t = beta * p[k];
        p[k] = r[k] + t;
      }
    rr = rn;
  }
  std::vector<double> out(ny * nx);
  for (int64_t j = 0; j < ny; ++j)
    for (int64_t i = 0; i < nx; ++i) out[j * nx + i] = u[(j + 1) * ld + i + 1];
  return out;
}

// Serial Chebyshev semi-iteration on the whole Dirichlet problem, the
// definition of JacobiSolver::cheby (gmt/jacobi.hpp): `iters` iterations from
// the initial field with the weights of `rho`, the cell in the kernel's order.
// *umax = max |u0| over the field and its ring.
static std::vector<double> serial_cheby(int64_t ny, int64_t nx, int iters, double rho, int source, double amp,
                                        uint64_t seed, int init, double* umax) {
  const int64_t ld = nx + 2;
  std::vector<double> u = serial_init(ny, nx, init, seed), src;
  if (source != 0) src = serial_source(ny, nx, source, amp, seed);
  *umax = 0;
  for (double v : u) *umax = std::fmax(*umax, std::fabs(v));
  std::vector<double> v = u;
  const double rho2 = rho * rho;
  double w = 1.0;
  for (int it = 0; it < iters; ++it) {
    if (it > 0) w = cheby_next_weight(rho2, w, it);
    for (int64_t j = 1; j <= ny; ++j)
      for (int64_t i = 1; i <= nx; ++i) {
        const double* c = &u[j * ld + i];
        double o = 0.25 * ((c[-1] + c[1]) + (c[-ld] + c[ld]));
        if (source != 0) o = o + 1.0 * src[(j - 1) * nx + i - 1];
        if (it == 0) {
          v[j * ld + i] = o;
        } else {
          const double pv = v[j * ld + i];
          volatile double t = o - pv;  // each operation rounded once
          t = w * t;
          v[j * ld + i] = pv + t;
        }
      }
    std::swap(u, v);
  }
  std::vector<double> out(ny * nx);
  for (int64_t j = 0; j < ny; ++j)
    for (int64_t i = 0; i < nx; ++i) out[j * nx + i] = u[(j + 1) * ld + i + 1];
  return out;
}

// Serial multigrid V-cycles on the whole Dirichlet problem, the definition of
// JacobiSolver::mg (gmt/jacobi.hpp): `cycles` cycles from the initial field on
// `levels` levels, every cell in the kernels' order (csrc/kernels/mg.hip).
// Fields carry a 1-wide ring: the real one on the fine level, zero below it.
static std::vector<double> serial_mg(int64_t ny, int64_t nx, int cycles, const MgOpts& o, int levels, int coarse_iters,
                                     double coarse_rho, int source, double amp, uint64_t seed, int init,
                                     double* umax) {
  struct Level {
    int64_t ny, nx, ld;
    std::vector<double> u[2], s, d;
    bool has_s;
  };
  std::vector<Level> lv(levels);
  for (int l = 0; l < levels; ++l) {
    Level& v = lv[l];
    // coarsen = any: mg_coarse_extent per axis, (n - 1)/2 on an odd one as under the nested rule
    v.ny = l == 0 ? ny : mg_coarse_extent(lv[l - 1].ny);
    v.nx = l == 0 ? nx : mg_coarse_extent(lv[l - 1].nx);
    v.ld = v.nx + 2;
    v.has_s = l > 0 || source != 0;
    for (auto* f : {&v.u[0], &v.u[1], &v.s, &v.d}) f->assign((v.ny + 2) * v.ld, 0.0);
  }
  lv[0].u[0] = serial_init(ny, nx, init, seed);
  lv[0].u[1] = lv[0].u[0];
  *umax = 0;
  for (double v : lv[0].u[0]) *umax = std::fmax(*umax, std::fabs(v));
  if (source != 0) {
    const std::vector<double> src = serial_source(ny, nx, source, amp, seed);
    for (int64_t j = 0; j < ny; ++j)
      for (int64_t i = 0; i < nx; ++i) lv[0].s[(j + 1) * lv[0].ld + i + 1] = src[j * nx + i];
  }
  const double rho2 = coarse_rho * coarse_rho;
  std::function<int(int, int)> cycle = [&](int l, int cur) -> int {
    Level& v = lv[l];
    const int64_t ld = v.ld;
    auto sweep = [&](const std::vector<double>& u, int64_t k) {
      const double* c = &u[k];
      double g = 0.25 * ((c[-1] + c[1]) + (c[-ld] + c[ld]));
      if (v.has_s) g = g + 1.0 * v.s[k];
      return g;
    };
    // out = c + w*(G(u) - c) over the interior, each operation rounded once
    auto relax = [&](double w, bool from_other) {
      const std::vector<double>& u = v.u[cur];
      std::vector<double>& out = v.u[cur ^ 1];
      for (int64_t j = 1; j <= v.ny; ++j)
        for (int64_t i = 1; i <= v.nx; ++i) {
          const int64_t k = j * ld + i;
          const double c = from_other ? out[k] : u[k];
          volatile double t = sweep(u, k) - c;
          t = w * t;
          out[k] = c + t;
        }
      cur ^= 1;
    };
    // one red-black sweep (MgOpts::smoother = 1): the red half-sweep (1-based i + j even), then the black
    // one, each into the other buffer, which keeps every cell of the other colour
    auto relax_rb = [&](double w) {
      for (int colour = 0; colour < 2; ++colour) {
        const std::vector<double>& u = v.u[cur];
        std::vector<double>& out = v.u[cur ^ 1];
        for (int64_t j = 1; j <= v.ny; ++j)
          for (int64_t i = 1; i <= v.nx; ++i) {
            const int64_t k = j * ld + i;
            const double c = u[k];
            if ((i + j) % 2 != colour) {
              out[k] = c;
              continue;
            }
            volatile double t = sweep(u, k) - c;
            t = w * t;
            out[k] = c + t;
          }
        cur ^= 1;
      }
    };
    auto smooth = [&](int n) {
      for (int i = 0; i < n; ++i) {
        if (o.smoother == 1)
          relax_rb(o.omega);
        else
          relax(o.omega, false);
      }
    };
    if (l == levels - 1) {  // Chebyshev from zero; the first iteration is the plain sweep
      double w = 1.0;
      for (int k = 0; k < coarse_iters; ++k) {
        if (k > 0) w = cheby_next_weight(rho2, w, k);
        if (k == 0) {
          for (int64_t j = 1; j <= v.ny; ++j)
            for (int64_t i = 1; i <= v.nx; ++i) v.u[cur ^ 1][j * ld + i] = sweep(v.u[cur], j * ld + i);
          cur ^= 1;
        } else {
          relax(w, true);
        }
      }
      return cur;
    }
    smooth(o.nu1);
    for (int64_t j = 1; j <= v.ny; ++j)
      for (int64_t i = 1; i <= v.nx; ++i) v.d[j * ld + i] = sweep(v.u[cur], j * ld + i) - v.u[cur][j * ld + i];
    Level& c = lv[l + 1];
    // a level with an even extent is not nested: the table-driven transfers of
    // gmt_mg_restrict_tab / gmt_mg_prolong_add_tab over the whole level
    const bool tab = v.ny % 2 == 0 || v.nx % 2 == 0;
    MgAxisTab tx, ty;
    if (tab && (mg_axis_tab_build(v.nx, c.nx, 0, v.nx, 0, c.nx, &tx) != 0 ||
                mg_axis_tab_build(v.ny, c.ny, 0, v.ny, 0, c.ny, &ty) != 0)) {
      std::printf("ERROR: serial multigrid: level %d has no transfer tables\n", l);
      std::exit(1);
    }
    if (tab) {
      auto hrow = [&](const double* q, const double* w, int cnt) {
        volatile double a0 = w[0] * q[0], a1 = w[1] * q[1], a2 = w[2] * q[2];
        double r = (a0 + a1) + a2;
        if (cnt == 4) {
          volatile double a3 = w[3] * q[3];
          r = r + a3;
        }
        return r;
      };
      for (int64_t J = 0; J < c.ny; ++J)
        for (int64_t I = 0; I < c.nx; ++I) {
          const double *wx = &tx.rw[4 * I], *wy = &ty.rw[4 * J];
          const int cx = tx.rf[2 * I + 1], cy = ty.rf[2 * J + 1];
          const double* q = &v.d[(1 + ty.rf[2 * J]) * ld + 1 + tx.rf[2 * I]];
          volatile double a0 = wy[0] * hrow(q, wx, cx), a1 = wy[1] * hrow(q + ld, wx, cx),
                          a2 = wy[2] * hrow(q + 2 * ld, wx, cx);
          double r = (a0 + a1) + a2;
          if (cy == 4) {
            volatile double a3 = wy[3] * hrow(q + 3 * ld, wx, cx);
            r = r + a3;
          }
          c.s[(J + 1) * c.ld + I + 1] = r;
        }
    } else {
      auto h = [&](int64_t k) { return (v.d[k - 1] + v.d[k + 1]) + 2.0 * v.d[k]; };
      for (int64_t J = 1; J <= c.ny; ++J)
        for (int64_t I = 1; I <= c.nx; ++I) {
          const int64_t k = 2 * J * ld + 2 * I;  // coarse point (J-1, I-1) sits on fine interior point (2J-1, 2I-1)
          c.s[J * c.ld + I] = 0.25 * ((h(k - ld) + h(k + ld)) + 2.0 * h(k));
        }
    }
    std::fill(c.u[0].begin(), c.u[0].end(), 0.0);
    const std::vector<double>& e = c.u[cycle(l + 1, 0)];
    std::vector<double>& u = v.u[cur];
    if (tab) {
      for (int64_t j = 0; j < v.ny; ++j)
        for (int64_t i = 0; i < v.nx; ++i) {
          const double* q = &e[(1 + ty.pq[j]) * c.ld + 1 + tx.pq[i]];
          const double t1x = tx.pt[i], t1y = ty.pt[j];
          const double w0x = 1.0 - t1x, w0y = 1.0 - t1y;
          volatile double b0 = w0x * q[0], b1 = t1x * q[1];
          const double bot = b0 + b1;
          volatile double t0 = w0x * q[c.ld], t1 = t1x * q[c.ld + 1];
          const double top = t0 + t1;
          volatile double vb = w0y * bot, vt = t1y * top;
          const double add = vb + vt;
          u[(j + 1) * ld + i + 1] = u[(j + 1) * ld + i + 1] + add;
        }
    } else {
      for (int64_t j = 1; j <= v.ny; ++j)
        for (int64_t i = 1; i <= v.nx; ++i) {
          const bool ony = j % 2 == 0, onx = i % 2 == 0;
          const double* p = &e[(ony ? j / 2 : (j - 1) / 2) * c.ld + (onx ? i / 2 : (i - 1) / 2)];
          double t;
          if (onx && ony)
            t = p[0];
          else if (ony)
            t = 0.5 * (p[0] + p[1]);
          else if (onx)
            t = 0.5 * (p[0] + p[c.ld]);
          else
            t = 0.25 * ((p[0] + p[1]) + (p[c.ld] + p[c.ld + 1]));
          u[j * ld + i] = u[j * ld + i] + t;
        }
    }
    smooth(o.nu2);
    return cur;
  };
  int cur = 0;
  for (int k = 0; k < cycles; ++k) cur = cycle(0, cur);
  std::vector<double> out(ny * nx);
  for (int64_t j = 0; j < ny; ++j)
    for (int64_t i = 0; i < nx; ++i) out[j * nx + i] = lv[0].u[cur][(j + 1) * lv[0].ld + i + 1];
  return out;
}

int main(int argc, char** argv) {
  Cli cli(argc, argv);
  int64_t n = cli.positional(0) ? std::atoll(cli.positional(0)) : 8192;
  const int n_iter = cli.positional(1) ? std::atoi(cli.positional(1)) : 100;
  const int n_warmup = static_cast<int>(cli.geti("warmup", 10));
  mpi_init_pinned(&argc, &argv);  // pinned near the GPU first (gmt/device.hpp)
  int world = 1, rank = 0;
  MPI_Comm_size(MPI_COMM_WORLD, &world);
  MPI_Comm_rank(MPI_COMM_WORLD, &rank);
  RankBinding b = set_rank_device(MPI_COMM_WORLD, false);

  JacobiConfig c;
  c.ny_global = cli.geti("ny", n);
  c.nx_global = cli.geti("nx", n);
  const std::string dims = cli.get("dims", "");
  if (!dims.empty()) {
    if (std::sscanf(dims.c_str(), "%dx%d", &c.py, &c.px) != 2 || c.py * c.px != world) {
      if (rank == 0) std::printf("ERROR: --dims=%s does not match %d ranks\n", dims.c_str(), world);
      MPI_Abort(MPI_COMM_WORLD, 1);
    }
  } else {
    choose_dims(world, c.ny_global, c.nx_global, &c.py, &c.px);
  }
  if (cli.flag("weak")) {
    c.ny_global *= c.py;
    c.nx_global *= c.px;
  }
  // --periodic wraps both axes, --periodic=x / =y one of them
  c.periodic = cli.has("periodic") && cli.get("periodic", "1") != "0";
  {
    const std::string pa = cli.get("periodic", "1");
    c.periodic_axes = pa == "x" ? 1 : (pa == "y" ? 2 : 3);
  }
  c.overlap = !cli.flag("no-overlap");
  c.overlap_auto = cli.get("overlap", "") == "auto";  // --overlap=auto: time both, keep the faster
  c.graph = cli.flag("graph");
  c.tblock = cli.has("tblock") && cli.get("tblock", "1") != "0";
  if (c.tblock) c.tsteps = static_cast<int>(cli.geti("tsteps", 2));
  c.wg_waves = static_cast<int>(cli.geti("wg-strips", 0));
  c.seg_rows = static_cast<int>(cli.geti("seg-rows", 0));
  c.push = cli.flag("push");
  c.tb_shared = static_cast<int>(cli.geti("shared", 0));
  if (c.tb_shared != -1 && c.tb_shared != 0 && c.tb_shared != 1 && c.tb_shared != 2 && c.tb_shared != 4) {
    if (rank == 0) std::printf("ERROR: --shared=%d is not one of -1, 0, 1, 2, 4\n", c.tb_shared);
    std::fflush(stdout);
    MPI_Abort(MPI_COMM_WORLD, 1);
  }
  // --init=analytic|random, --seed=S
  if (cli.has("init")) {
    const std::string in = cli.get("init", "analytic");
    c.init = in == "random" ? 1 : 0;
    c.seed = static_cast<uint64_t>(cli.geti("seed", 0));
    if (in != "analytic" && in != "random") {
      if (rank == 0) std::printf("ERROR: --init=%s is not analytic or random\n", in.c_str());
      std::fflush(stdout);
      MPI_Abort(MPI_COMM_WORLD, 1);
    }
  }
  // --source=poly | random[:AMP], --src-every=B
  const std::string src_arg = cli.get("source", "");
  if (!src_arg.empty()) {
    const std::string kind = src_arg.substr(0, src_arg.find(':'));
    c.source = kind == "poly" ? 1 : (kind == "random" ? 2 : -1);
    if (c.source == 2 && src_arg.find(':') != std::string::npos)
      c.source_amp = std::atof(src_arg.c_str() + src_arg.find(':') + 1);
    c.src_every = static_cast<int>(cli.geti("src-every", 0));
    const int ks = c.tblock ? (c.tsteps > 1 ? c.tsteps : 2) : 1;
    if (c.source < 0 || !(c.source_amp >= 0) || !std::isfinite(c.source_amp) || c.src_every < 0 ||
        (ks > 1 && c.src_every % ks != 0)) {
      if (rank == 0)
        std::printf("ERROR: --source=poly|random[:AMP] (AMP finite, >= 0) and --src-every a positive multiple of "
                    "--tsteps (%d); got --source=%s --src-every=%d\n", ks, src_arg.c_str(), c.src_every);
      std::fflush(stdout);
      MPI_Abort(MPI_COMM_WORLD, 1);
    }
  }
  // with one rank and no periodic wrap there is nothing to exchange; with a
  // periodic wrap a single rank exchanges with itself
  comm::Kind kind = comm::parse_kind(cli.get("transport", "auto"));
  if (kind == comm::Kind::Auto && world == 1) kind = comm::Kind::Local;
  auto tr = comm::make_transport(comm::resolve(kind, b), MPI_COMM_WORLD, b);

  // solve to tolerance: --tol / --rtol
  // cg_mode covers both Krylov-rate modes (their options, timing and report
  // are shared); cheby_mode picks JacobiSolver::cheby
  const bool cheby_mode = cli.flag("cheby");
  if (cheby_mode && cli.flag("cg")) {
    if (rank == 0) std::printf("ERROR: --cheby and --cg are exclusive\n");
    std::fflush(stdout);
    MPI_Abort(MPI_COMM_WORLD, 1);
  }
  // mg_mode picks JacobiSolver::mg: a cycle is its iteration
  const bool mg_mode = cli.flag("mg");
  if (mg_mode && (cheby_mode || cli.flag("cg"))) {
    if (rank == 0) std::printf("ERROR: --mg is exclusive with --cg and --cheby\n");
    std::fflush(stdout);
    MPI_Abort(MPI_COMM_WORLD, 1);
  }
  if (!mg_mode && cli.has("smoother")) {
    if (rank == 0) std::printf("ERROR: --smoother needs --mg\n");
    std::fflush(stdout);
    MPI_Abort(MPI_COMM_WORLD, 1);
  }
  const bool cg_mode = cli.flag("cg") || cheby_mode || mg_mode;
  const char* mode_name = mg_mode ? "--mg" : (cheby_mode ? "--cheby" : "--cg");
  MgOpts mo;
  MgResult mr;
  if (mg_mode) {
    // a refused --mg option: every rank decides the same from the command line and global shapes, so they
    // leave in order; a rank's MPI_Abort could take the launcher down before it has forwarded rank 0's message
    auto refuse = [&] {
      std::fflush(stdout);
      tr.reset();
      MPI_Finalize();
      return 1;
    };
    const std::string nu = cli.get("nu", "2,2");
    const bool nu_ok = std::sscanf(nu.c_str(), "%d,%d", &mo.nu1, &mo.nu2) == 2;
    const std::string smoother = cli.get("smoother", "jacobi");
    if (smoother != "jacobi" && smoother != "rb") {
      if (rank == 0) std::printf("ERROR: --smoother must be jacobi or rb\n");
      return refuse();
    }
    mo.smoother = smoother == "rb" ? 1 : 0;
    mo.omega = std::atof(cli.get("omega", mo.smoother ? "1.0" : "0.8").c_str());
    mo.max_levels = static_cast<int>(cli.geti("levels", 0));
    mo.coarse_iters = static_cast<int>(cli.geti("coarse-iters", 0));
    const std::string coarsen = cli.get("coarsen", "nested");
    if (coarsen != "nested" && coarsen != "any") {
      if (rank == 0) std::printf("ERROR: --coarsen must be nested or any\n");
      return refuse();
    }
    mo.coarsen = coarsen == "any" ? 1 : 0;
    mo.fuse = static_cast<int>(cli.geti("fuse", 0));
    mo.fuse_resid = cli.flag("fuse-resid") ? 1 : 0;
    mo.fuse_prolong = cli.flag("fuse-prolong") ? 1 : 0;
    if (mo.fuse != 0 && (mo.fuse < 2 || mo.fuse > GMT_MG_MAX_FUSE)) {
      if (rank == 0) std::printf("ERROR: --fuse must be 0 or 2..%d\n", GMT_MG_MAX_FUSE);
      return refuse();
    }
    if (!nu_ok || mo.nu1 < 0 || mo.nu2 < 0 || mo.nu1 + mo.nu2 == 0 || !(mo.omega > 0 && mo.omega <= 1) ||
        mo.max_levels < 0 || mo.max_levels == 1 || mo.coarse_iters < 0) {
      if (rank == 0)
        std::printf("ERROR: --mg needs --nu=A,B (A, B >= 0, A + B > 0), --omega in (0, 1], --levels 0 or >= 2 and "
                    "--coarse-iters >= 0\n");
      return refuse();
    }
    if (!c.periodic && mg_level_table(c.ny_global, c.nx_global, c.py, c.px, mo.max_levels, mo.coarsen).size() < 2) {
      if (rank == 0) {
        if (mo.coarsen == 0 && (c.ny_global % 2 == 0 || c.nx_global % 2 == 0))
          std::printf("ERROR: --mg has no coarse level for %lld x %lld: nx + 1 and ny + 1 must be even (8191 and "
                      "32767 coarsen, 8192 does not), or pass --coarsen=any\n", (long long)c.ny_global,
                      (long long)c.nx_global);
        else
          std::printf("ERROR: --mg has no coarse level for %lld x %lld on a %dx%d grid: %sa rank would own no coarse "
                      "point\n", (long long)c.ny_global, (long long)c.nx_global, c.py, c.px,
                      mo.coarsen ? "the extents are too small or " : "");
      }
      return refuse();
    }
  }
  const bool solve_mode = !cg_mode && (cli.has("tol") || cli.has("rtol"));
  CgOpts co;
  CgResult cr;
  ChebyOpts ho;
  double rho_used = 0;
  if (cheby_mode) {
    ho.rho = std::atof(cli.get("rho", "0").c_str());
    if (cli.has("rho") && !(std::isfinite(ho.rho) && ho.rho > 0 && ho.rho < 1)) {
      if (rank == 0) std::printf("ERROR: --rho must be finite and in (0, 1)\n");
      std::fflush(stdout);
      MPI_Abort(MPI_COMM_WORLD, 1);
    }
  }
  if (cg_mode) {
    co.tol = std::atof(cli.get("tol", "0").c_str());
    co.rtol = std::atof(cli.get("rtol", "0").c_str());
    const std::string nm = cli.get("norm", "l2");
    co.norm = nm == "max" ? 1 : 0;
    co.lag = static_cast<int>(cli.geti("lag", 1));
    co.check_every = static_cast<int>(cli.geti("check-every", 0));
    if (co.check_every == 0) co.check_every = mg_mode ? 1 : 10;
    if (c.periodic || (nm != "l2" && nm != "max") || co.lag < 0 || co.lag > 8 || co.check_every < 1 || n_iter < 1 ||
        !(co.tol >= 0) || !(co.rtol >= 0) || !std::isfinite(co.tol) || !std::isfinite(co.rtol)) {
      if (rank == 0)
        std::printf("ERROR: %s needs Dirichlet sides (no --periodic: I - J is singular on a periodic axis), "
                    "--tol and --rtol >= 0, --norm=l2|max, --lag=0..8, --check-every >= 1 and an iteration cap "
                    "(n_iter) >= 1\n", mode_name);
      std::fflush(stdout);
      MPI_Abort(MPI_COMM_WORLD, 1);
    }
    co.max_iters = (n_iter + co.check_every - 1) / co.check_every * co.check_every;
    ho.tol = co.tol;
    ho.rtol = co.rtol;
    ho.norm = co.norm;
    ho.lag = co.lag;
    ho.check_every = co.check_every;
    ho.max_iters = co.max_iters;
    mo.tol = co.tol;
    mo.rtol = co.rtol;
    mo.norm = co.norm;
    mo.lag = co.lag;
    mo.check_every = co.check_every;
    mo.max_cycles = co.max_iters;
  }
  const bool cg_fixed = cg_mode && !(co.tol > 0) && !(co.rtol > 0);
  SolveOpts so;
  SolveResult sr;
  double solve_ms = 0;
  const int cap_asked = n_iter;
  if (solve_mode) {
    so.tol = std::atof(cli.get("tol", "0").c_str());
    so.rtol = std::atof(cli.get("rtol", "0").c_str());
    const std::string nm = cli.get("norm", "l2");
    so.norm = nm == "max" ? 1 : 0;
    so.lag = static_cast<int>(cli.geti("lag", 1));
    so.check_every = static_cast<int>(cli.geti("check-every", 0));
    if ((nm != "l2" && nm != "max") || so.lag < 0 || so.lag > 8 || so.check_every < 0 || n_iter < 1 ||
        !(so.tol >= 0) || !(so.rtol >= 0) || !(so.tol > 0 || so.rtol > 0)) {
      if (rank == 0)
        std::printf("ERROR: solve mode needs --tol or --rtol > 0, --norm=l2|max, --lag=0..8, --check-every >= 1 "
                    "and a sweep cap (n_iter) >= 1\n");
      std::fflush(stdout);
      MPI_Abort(MPI_COMM_WORLD, 1);
    }
  }

  double t_step = 0, resid = 0, halo_us = 0, max_diff = -1, check_bound = 1e-10;
  bool graph = false, overlap = false, band = false, push = false, graph_sweep = false, graph_fused = false;
  size_t hbytes = 0, hmsgs = 0;
  int64_t lnx = 0, lny = 0;
  int sh_strips = 0;
  int src_every = 0, src_setup_sweeps = 0;
  double src_setup_ms = 0, src_mib = 0, src_err = -1;
  {
    JacobiSolver solver(*tr, c);
    src_every = solver.src_every();
    src_setup_sweeps = solver.source_setup_sweeps();
    src_setup_ms = solver.source_setup_ms();
    src_mib = static_cast<double>(solver.source_bytes()) / (1 << 20);
    graph = solver.graph_active();
    graph_sweep = solver.sweep_graph_active();
    graph_fused = solver.fused_graph_active();
    overlap = solver.overlap_active();
    band = solver.band_first();
    push = solver.push_active();
    if (c.tblock && c.tsteps > 1) sh_strips = solver.tb_shared_strips(solver.tsteps());
    hbytes = solver.bytes_per_exchange();
    hmsgs = solver.messages();
    lnx = solver.nx();
    lny = solver.ny();
    int total_sweeps = n_warmup + n_iter;  // what --check replays
    if (mg_mode) {
      // the warm-up as for --cg below: one check's worth of cycles (first
      // launches, the level hierarchy), then the field is the initial one again
      MgOpts w = mo;
      w.tol = w.rtol = 0;
      w.max_cycles = w.check_every = mo.check_every;
      w.lag = 0;
      solver.mg(w);
      solver.prepare(1);
      MPI_Barrier(MPI_COMM_WORLD);
      const double t0 = wtime();
      mr = solver.mg(mo);
      double dt = wtime() - t0;
      MPI_Allreduce(MPI_IN_PLACE, &dt, 1, MPI_DOUBLE, MPI_MAX, MPI_COMM_WORLD);
      solve_ms = dt * 1e3;
      t_step = dt / (mr.iters > 0 ? mr.iters : 1);
      total_sweeps = mr.iters;
      static_cast<CheckResult&>(cr) = mr;  // reported through --cg's lines
    } else if (cheby_mode) {
      // the warm-up as for --cg below: one check's worth of iterations (first
      // launches, the halo plans), then the field is the initial one again
      ChebyOpts w;
      w.max_iters = w.check_every = ho.check_every;
      w.lag = 0;
      w.rho = ho.rho;
      solver.cheby(w);
      solver.prepare(1);
      MPI_Barrier(MPI_COMM_WORLD);
      const double t0 = wtime();
      const ChebyResult hr = solver.cheby(ho);
      double dt = wtime() - t0;
      MPI_Allreduce(MPI_IN_PLACE, &dt, 1, MPI_DOUBLE, MPI_MAX, MPI_COMM_WORLD);
      solve_ms = dt * 1e3;
      t_step = dt / (hr.iters > 0 ? hr.iters : 1);
      total_sweeps = hr.iters;
      rho_used = hr.rho;
      static_cast<CheckResult&>(cr) = hr;  // reported through --cg's lines
    } else if (cg_mode) {
      // the warm-up runs one check's worth of iterations (first launches, the
      // state of cg()), then the field is the initial one again
      CgOpts w;
      w.max_iters = w.check_every = co.check_every;
      w.lag = 0;
      solver.cg(w);
      solver.prepare(1);
      MPI_Barrier(MPI_COMM_WORLD);
      const double t0 = wtime();
      cr = solver.cg(co);
      double dt = wtime() - t0;
      MPI_Allreduce(MPI_IN_PLACE, &dt, 1, MPI_DOUBLE, MPI_MAX, MPI_COMM_WORLD);
      solve_ms = dt * 1e3;
      t_step = dt / (cr.iters > 0 ? cr.iters : 1);
      total_sweeps = cr.iters;
    } else if (solve_mode) {
      // the warm-up launches one pass of every kind and the residual kernel,
      // then the field is the initial one again: the solve starts from it
      if (so.check_every == 0) so.check_every = solver.tsteps();
      so.max_sweeps = (n_iter + so.check_every - 1) / so.check_every * so.check_every;
      solver.prepare(so.check_every);
      double warm[2];
      solver.residual_norm(warm);
      MPI_Barrier(MPI_COMM_WORLD);
      const double t0 = wtime();
      sr = solver.solve(so);
      double dt = wtime() - t0;
      MPI_Allreduce(MPI_IN_PLACE, &dt, 1, MPI_DOUBLE, MPI_MAX, MPI_COMM_WORLD);
      solve_ms = dt * 1e3;
      t_step = dt / (sr.iters > 0 ? sr.iters : 1);
      total_sweeps = sr.iters;
    } else {
      solver.run(n_warmup);
      solver.synchronize();
      MPI_Barrier(MPI_COMM_WORLD);
      const double t0 = wtime();
      solver.run(n_iter);
      solver.synchronize();
      double dt = wtime() - t0;
      MPI_Allreduce(MPI_IN_PLACE, &dt, 1, MPI_DOUBLE, MPI_MAX, MPI_COMM_WORLD);
      t_step = dt / (n_iter > 0 ? n_iter : 1);
    }

    if (cli.flag("check")) {
      std::vector<double> loc(static_cast<size_t>(lnx * lny));
      solver.copy_interior(loc.data());
      // gather every rank's block on rank 0 and compare with the serial run
      long long meta[4] = {solver.off_y(), solver.off_x(), lny, lnx};
      std::vector<long long> all(4 * world);
      MPI_Gather(meta, 4, MPI_LONG_LONG, all.data(), 4, MPI_LONG_LONG, 0, MPI_COMM_WORLD);
      std::vector<int> counts(world), displs(world);
      for (int r = 0; r < world; ++r) counts[r] = static_cast<int>(all[4 * r + 2] * all[4 * r + 3]);
      for (int r = 1; r < world; ++r) displs[r] = displs[r - 1] + counts[r - 1];
      std::vector<double> g(rank == 0 ? static_cast<size_t>(c.ny_global * c.nx_global) : 1);
      MPI_Gatherv(loc.data(), static_cast<int>(loc.size()), MPI_DOUBLE, g.data(), counts.data(),
                  displs.data(), MPI_DOUBLE, 0, MPI_COMM_WORLD);
      if (rank == 0) {
        double umax = 0;
        std::vector<double> ref =
            mg_mode ? serial_mg(c.ny_global, c.nx_global, total_sweeps, mo, mr.levels, mr.coarse_iters, mr.coarse_rho,
                                c.source, c.source_amp, c.seed, c.init, &umax)
            : cheby_mode ? serial_cheby(c.ny_global, c.nx_global, total_sweeps, rho_used, c.source, c.source_amp,
                                      c.seed, c.init, &umax)
            : cg_mode ? serial_cg(c.ny_global, c.nx_global, total_sweeps, c.source, c.source_amp, c.seed, c.init, &umax)
                    : serial_jacobi(c.ny_global, c.nx_global, total_sweeps, c.periodic, c.periodic_axes, c.source,
                                    c.source_amp, c.seed, c.init);
        if (cg_mode) check_bound = 1e-10 * umax;
        // the poly source makes the initial field the discrete fixed point (fixed ring)
        std::vector<double> u0;
        if (c.source == 1 && c.init == 0 && !c.periodic && !cg_mode) {
          u0 = serial_jacobi(c.ny_global, c.nx_global, 0, c.periodic, c.periodic_axes);
          src_err = 0;
        }
        max_diff = 0;
        for (int r = 0; r < world; ++r) {
          const long long oy = all[4 * r], ox = all[4 * r + 1], ny = all[4 * r + 2], nx = all[4 * r + 3];
          const double* blk = g.data() + displs[r];
          for (long long j = 0; j < ny; ++j)
            for (long long i = 0; i < nx; ++i)
              max_diff = std::fmax(max_diff, std::fabs(blk[j * nx + i] -
                                                       ref[(oy + j) * c.nx_global + ox + i]));
          if (!u0.empty())
            for (long long j = 0; j < ny; ++j)
              for (long long i = 0; i < nx; ++i)
                src_err = std::fmax(src_err, std::fabs(blk[j * nx + i] - u0[(oy + j) * c.nx_global + ox + i]));
        }
      }
    }
    const int halo_iters = static_cast<int>(cli.geti("halo-iters", 0));
    if (halo_iters > 0 && hmsgs > 0) {
      Stats st;
      for (int k = 0; k < halo_iters + 3; ++k) {
        MPI_Barrier(MPI_COMM_WORLD);
        const double h0 = wtime();
        solver.exchange_only();
        if (k >= 3) st.add(wtime() - h0);
      }
      double med = st.median();
      MPI_Allreduce(&med, &halo_us, 1, MPI_DOUBLE, MPI_MAX, MPI_COMM_WORLD);
      halo_us *= 1e6;
    }
    // solve mode: the deciding residual, without the extra sweep
    resid = cg_mode ? cr.residual : (solve_mode ? sr.residual : solver.residual());
  }
  if (rank == 0) {
    const double pts = static_cast<double>(c.ny_global) * c.nx_global;
    const double mlups = pts / t_step / 1e6;
    std::printf("n procs   = %d\n", world);
    std::printf("grid      = %dx%d (py x px)\n", c.py, c.px);
    std::printf("global    = %lld x %lld\n", (long long)c.ny_global, (long long)c.nx_global);
    std::printf("local     = %lld x %lld (rank 0)\n", (long long)lny, (long long)lnx);
    std::printf("transport = %s overlap=%d%s graph=%d periodic=%d tblock=%d backend=%s\n", tr->name(),
                overlap, band ? " (band-first)" : (push ? " (inline halo)" : ""), graph, c.periodic, c.tblock,
                gmt_rt_backend_name());
    // which passes replay from hipGraphs: single sweeps, full fused passes
    // (inline-halo ones with their hand-over); partial passes are always eager
    if (c.graph) std::printf("graphs    = sweep:%d fused:%d\n", graph_sweep, graph_fused);
    if (c.tb_shared != 0)
      std::printf("shared    = %d (rank 0: %d strips per shared hand-off group, 0 = per-strip launch)\n", c.tb_shared,
                  sh_strips);
    if (c.source != 0) {
      char amp[48] = "";
      if (c.source == 2) std::snprintf(amp, sizeof(amp), ":%g", c.source_amp);
      if (src_every > 0)
        std::printf("source    = %s%s every %d sweeps (set-up %d sweeps, %0.3f ms, %0.1f MiB)\n",
                    c.source == 1 ? "poly" : "random", amp, src_every, src_setup_sweeps, src_setup_ms, src_mib);
      else
        std::printf("source    = %s%s every 1 sweeps (set-up 0 sweeps, %0.3f ms, %0.1f MiB)\n",
                    c.source == 1 ? "poly" : "random", amp, src_setup_ms, src_mib);
    }
    const char* solver_name = mg_mode ? "multigrid" : (cheby_mode ? "chebyshev" : "cg");
    const char* unit = mg_mode ? "cycle" : "iteration";
    if (cg_mode) {
      std::printf("solver    = %s\n", solver_name);
      if (mg_mode && mo.smoother == 1) std::printf("smoother  = rb (omega %g)\n", mo.omega);
      if (cheby_mode) std::printf("rho       = %.17g%s\n", rho_used, ho.rho == 0 ? " (closed form)" : "");
      if (mg_mode) {
        std::printf("levels    = %d (coarsest %lld x %lld, %d iterations, rho %.6g)\n", mr.levels,
                    (long long)mr.coarse_ny, (long long)mr.coarse_nx, mr.coarse_iters, mr.coarse_rho);
        std::printf("cycle     = V(%d,%d), omega %g\n", mo.nu1, mo.nu2, mo.omega);
        std::printf("coarsen   = %s\n", mo.coarsen ? "any" : "nested");
        if (mo.fuse)
          std::printf("fuse      = %d (fine level %d, %d of %d levels fused)\n", mr.fuse, mr.fuse_fine, mr.fuse_levels,
                      mr.levels - 1);
        if (mo.fuse_resid)
          std::printf("resid     = fused (%d of %d levels)\n", mr.resid_levels, mr.levels - 1);
        if (mo.fuse_prolong)
          std::printf("prolong   = fused (%d of %d levels)\n", mr.prolong_levels, mr.levels - 1);
      }
      if (cg_fixed)
        std::printf("solve     = fixed count, %s norm, check every %d %ss\n", co.norm ? "max" : "l2",
                    co.check_every, unit);
      else
        std::printf("solve     = r <= max(%g, %g * r0), %s norm, check every %d %ss, lag %d\n", co.tol, co.rtol,
                    co.norm ? "max" : "l2", co.check_every, unit, co.lag);
      if (co.max_iters != cap_asked)
        std::printf("steps     = at most %d (%d rounded up to a multiple of %d)\n", co.max_iters, cap_asked,
                    co.check_every);
      else
        std::printf("steps     = at most %d\n", co.max_iters);
      const char* count = mg_mode ? "cycles   " : "iters    ";
      if (cg_fixed) {
        std::printf("%s : %d (fixed count, %d checks)\n", count, cr.iters, cr.checks);
      } else {
        std::printf("converged : %s%s\n", cr.converged ? "yes" : "no", cr.failed ? " (non-finite residual)" : "");
        std::printf("%s : %d (criterion met at %d, %d checks, lag %d)\n", count, cr.iters, cr.residual_iters, cr.checks,
                    co.lag);
      }
      std::printf("TIME solve: %0.6f ms\n", solve_ms);
      if (mg_mode)
        std::printf("TIME cycle: %0.6f ms per cycle\n", t_step * 1e3);
      else
        std::printf("TIME iter : %0.6f ms per iteration\n", t_step * 1e3);
    } else if (solve_mode) {
      std::printf("solve     = r <= max(%g, %g * r0), %s norm, check every %d sweeps, lag %d\n", so.tol, so.rtol,
                  so.norm ? "max" : "l2", so.check_every, so.lag);
      if (so.max_sweeps != cap_asked)
        std::printf("steps     = at most %d (%d rounded up to a multiple of %d)\n", so.max_sweeps, cap_asked,
                    so.check_every);
      else
        std::printf("steps     = at most %d\n", so.max_sweeps);
      std::printf("converged : %s%s\n", sr.converged ? "yes" : "no", sr.failed ? " (non-finite residual)" : "");
      std::printf("sweeps    : %d (criterion met at %d, %d checks, lag %d)\n", sr.iters, sr.residual_iters, sr.checks,
                  so.lag);
      std::printf("TIME solve: %0.6f ms\n", solve_ms);
    } else {
      std::printf("steps     = %d (warmup %d)\n", n_iter, n_warmup);
    }
    if (!cg_mode) {
      std::printf("TIME step : %0.6f ms\n", t_step * 1e3);
      std::printf("MLUPS     : %0.1f (per GPU %0.1f, %0.1f GB/s per GPU at 16 B/pt)\n", mlups,
                  mlups / world, 16.0 * pts / world / t_step / 1e9);
    }
    if (halo_us > 0)
      std::printf("halo      : %0.2f us per exchange (%zu B, %zu msgs per rank)\n", halo_us, hbytes, hmsgs);
    std::printf("residual  : %.10e\n", resid);
    if (cg_mode && !cheby_mode && !mg_mode)
      std::printf("true resid: %.10e (max %.10e)\n", cr.true_residual, cr.true_residual_max);
    if (max_diff >= 0 && cg_mode)
      std::printf("check     : max|diff| vs serial %s = %.3e (bound %.3e) %s\n", solver_name,
                  max_diff, check_bound,
                  max_diff <= check_bound ? "OK" : "FAIL");
    else if (max_diff >= 0)
      std::printf("check     : max|diff| vs serial = %.3e %s\n", max_diff, max_diff < 1e-10 ? "OK" : "FAIL");
    if (src_err >= 0) std::printf("source err: max|u - u0| = %.3e\n", src_err);
    JsonRecord j;
    j.add("app", "mpi_jacobi2d").add("ranks", world).add("py", c.py).add("px", c.px)
        .add("ny", (long long)c.ny_global).add("nx", (long long)c.nx_global).add("transport", tr->name())
        .add("overlap", overlap).add("band_first", band).add("push", push).add("shared_strips", sh_strips).add("graph", graph).add("graph_fused", graph_fused).add("tblock", c.tblock).add("steps", n_iter).add("ms_per_step", t_step * 1e3)
        .add("MLUPS", mlups).add("halo_us", halo_us).add("halo_bytes", hbytes).add("residual", resid)
        .add("check_max_diff", max_diff);
    if (solve_mode)
      j.add("converged", sr.converged != 0).add("sweeps", sr.iters).add("residual_sweeps", sr.residual_iters)
          .add("checks", sr.checks).add("solve_ms", solve_ms).add("r0", sr.r0).add("residual_max", sr.residual_max);
    if (mg_mode && mo.fuse_prolong)
      j.add("fuse_prolong", true).add("prolong_levels", mr.prolong_levels).add("prolong_mask", mr.prolong_mask);
    if (mg_mode)
      j.add("solver", "multigrid").add("coarsen", mo.coarsen ? "any" : "nested").add("levels", mr.levels)
          .add("cycles", mr.iters).add("fuse", mr.fuse).add("fuse_fine", mr.fuse_fine)
          .add("fuse_levels", mr.fuse_levels).add("smoother", mo.smoother ? "rb" : "jacobi")
          .add("fuse_resid", mr.fuse_resid != 0).add("resid_levels", mr.resid_levels).add("resid_mask", mr.resid_mask)
          .add("residual_cycles", mr.residual_iters).add("checks", mr.checks).add("converged", mr.converged != 0)
          .add("solve_ms", solve_ms).add("r0", mr.r0).add("residual_max", mr.residual_max);
    else if (cg_mode)
      j.add("solver", cheby_mode ? "chebyshev" : "cg").add("converged", cr.converged != 0).add("iters", cr.iters)
          .add("residual_iters", cr.residual_iters).add("checks", cr.checks).add("solve_ms", solve_ms).add("r0", cr.r0)
          .add("residual_max", cr.residual_max);
    if (cheby_mode)
      j.add("rho", rho_used);
    else if (cg_mode && !mg_mode)
      j.add("true_residual", cr.true_residual);
    if (c.source != 0)
      j.add("source", c.source == 1 ? "poly" : "random").add("src_every", src_every > 0 ? src_every : 1)
          .add("source_setup_ms", src_setup_ms);
    j.append_to(cli.get("json", ""));
  }
  tr.reset();
  MPI_Finalize();
  // rank 0 ran the check: its verdict is every rank's exit status
  int check_failed = cg_mode ? (max_diff > check_bound) : (max_diff >= 1e-10);
  if (cg_mode) return check_failed ? 3 : (cr.failed || (!cg_fixed && !cr.converged) ? 4 : EXIT_SUCCESS);
  if (check_failed) return 3;
  return solve_mode && (!sr.converged || sr.failed) ? 4 : EXIT_SUCCESS;
}
