// gmt_kernel_bench — A/B timing of every hand-written kernel variant.
//
// Not in the reference (it has no kernels of its own).  Times
// the gfx950 kernels with hipEvents, median of --iters launches, and prints
// the effective HBM bandwidth from the kernel's compulsory bytes:
//   daxpy      24 B/elem      (variants 1-5)
//   jacobi5    16 B/point     (variants 1-8)
//   stencil5   16 B/point     (dim 0 / dim 1, the reference's derivative)
//   copy2d     16 B/elem      (halo pack of a dim-0 face: strided 16-B reads)
// CLI: gmt_kernel_bench [--daxpy-n=N] [--jacobi-n=N] [--iters=K] [--json=FILE]
//      [--only=daxpy,jacobi,stencil,pack]
//      --only=edges [--reps=5]: the boundary-band split of the derivative
//      (gmt_stencil5_2d_edges / _interior) against the whole-field kernels
//      --only=resid [--reps=5]: the read-only Jacobi residual (8 B/point) against
//      the sweep with residual (16 B/point) and gmt_sum, at 8192^2 and 32768^2
//      --only=add2d [--reps=5]: the source-block add (gmt_add2d) alternated with
//      gmt_daxpy on the same element count (24 B/point each)
//      --only=cheby [--reps=5] [--cheby-n=N]: the launch of a Chebyshev iteration
//      (gmt_cheby_step, 24 B/point, 32 with f) against gmt_daxpy, as --only=cg.
//      --only=cg [--reps=5] [--cg-n=N]: the three launches of a conjugate-gradient
//      iteration (gmt_cg_apply 16 B/point, gmt_cg_update 48, gmt_cg_dir 24), each
//      alternated with gmt_daxpy on the same element count
//      --only=mg [--reps=5] [--mg-n=N]: the kernels of a multigrid cycle
//      (gmt_mg_smooth 16 B/fine point, 24 with f, gmt_mg_restrict 10,
//      gmt_mg_prolong_add 18) on N x N (default 8191; an even N times them at
//      N - 1 and the table-driven transfers of coarsen = any at N), as --only=cg;
//      then the fused smoother gmt_mg_smooth_k for k = 2, 3, 4 without and with
//      f, compared bitwise with k single sweeps and timed beside them and DAXPY,
//      and the red-black smoother gmt_mg_smooth_rb for h = 1, 2, 4 half-sweeps
//      without and with f, compared bitwise with h launches of h = 1 and timed
//      beside gmt_mg_smooth_k of k = h, and the fused transfer
//      gmt_mg_resid_restrict without and with f, compared bitwise with
//      gmt_cg_apply mode 1 + gmt_mg_restrict and timed beside the two, and the
//      fused interpolation gmt_mg_prolong_smooth for h = 1, 2, 4 (Jacobi and
//      red-black) without and with f, compared bitwise with gmt_mg_prolong_add +
//      gmt_mg_smooth_k / gmt_mg_smooth_rb and timed beside the two
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <string>
#include <vector>

#include "gmt/buffer.hpp"
#include "gmt/util.hpp"

using namespace gmt;

// --sustained=1: the mean of `iters` back-to-back launches (one event pair,
// the GPU never idles: what a solver loop sees, clocks included); default:
// the median of `iters` launches each synchronised on its own
static bool g_sustained = false;

static double time_ms(gmt_stream_t s, int iters, const std::function<void()>& f) {
  gmt_event_t e0, e1;
  GMT_CHECK("event", gmt_rt_event_create(&e0, 1));
  GMT_CHECK("event", gmt_rt_event_create(&e1, 1));
  // the process's first measurement starts from an idle GPU: without a
  // longer warm-up it read 6-12% low whatever it measured (profiles/r04_shares.md)
  static bool first = true;
  if (first) {
    first = false;
    const double t0 = wtime();
    while (wtime() - t0 < 0.2) {
      for (int w = 0; w < 4; ++w) f();
      GMT_CHECK("sync", gmt_rt_stream_synchronize(s));
    }
  }
  for (int w = 0; w < 3; ++w) f();
  if (g_sustained) {
    GMT_CHECK("rec", gmt_rt_event_record(e0, s));
    for (int k = 0; k < iters; ++k) f();
    GMT_CHECK("rec", gmt_rt_event_record(e1, s));
    GMT_CHECK("sync", gmt_rt_event_synchronize(e1));
    float ms = 0;
    GMT_CHECK("elapsed", gmt_rt_event_elapsed_ms(&ms, e0, e1));
    gmt_rt_event_destroy(e0);
    gmt_rt_event_destroy(e1);
    return ms / iters;
  }
  Stats st;
  for (int k = 0; k < iters; ++k) {
    GMT_CHECK("rec", gmt_rt_event_record(e0, s));
    f();
    GMT_CHECK("rec", gmt_rt_event_record(e1, s));
    GMT_CHECK("sync", gmt_rt_event_synchronize(e1));
    float ms = 0;
    GMT_CHECK("elapsed", gmt_rt_event_elapsed_ms(&ms, e0, e1));
    st.add(ms);
  }
  gmt_rt_event_destroy(e0);
  gmt_rt_event_destroy(e1);
  return st.median();
}

int main(int argc, char** argv) {
  Cli cli(argc, argv);
  const int iters = static_cast<int>(cli.geti("iters", 20));
  const std::string only = cli.get("only", "daxpy,jacobi,stencil,pack");
  const std::string json = cli.get("json", "");
  g_sustained = cli.geti("sustained", 0) != 0;
  gmt_stream_t s = nullptr;
  GMT_CHECK("stream", gmt_rt_stream_create(&s, 0));
  auto report = [&](const char* kernel, int variant, const char* shape, double ms, double bytes) {
    const double gbps = bytes / (ms * 1e-3) / 1e9;
    std::printf("%-10s v%-2d %-22s %9.4f ms  %8.1f GB/s\n", kernel, variant, shape, ms, gbps);
    JsonRecord j;
    j.add("app", "gmt_kernel_bench").add("kernel", kernel).add("variant", variant).add("shape", shape)
        .add("ms", ms).add("GBps", gbps).add("backend", gmt_rt_backend_name());
    j.append_to(json);
  };
  std::printf("# gmt_kernel_bench backend=%s iters=%d (%s)\n", gmt_rt_backend_name(), iters,
              g_sustained ? "sustained mean" : "median");

  if (only.find("daxpy") != std::string::npos) {
    const size_t n = static_cast<size_t>(cli.geti("daxpy-n", 1LL << 28));
    Buffer<double> x(n, GMT_SPACE_DEVICE), y(n, GMT_SPACE_DEVICE);
    GMT_CHECK("fill", gmt_fill_poly(1, n, 1, 0.0, 1e-9, 0.0, 0.0, x.data(), n, s));
    GMT_CHECK("fill", gmt_fill_poly(1, n, 1, 1.0, 1e-9, 0.0, 0.0, y.data(), n, s));
    char shape[64];
    std::snprintf(shape, sizeof(shape), "n=%zu", n);
    double ms = time_ms(s, iters, [&] { GMT_CHECK("daxpy", gmt_daxpy(n, 1e-3, x.data(), y.data(), s)); });
    report("daxpy", 0, shape, ms, 24.0 * n);
    ms = time_ms(s, iters, [&] { GMT_CHECK("daxpy", gmt_blas_daxpy(n, 1e-3, x.data(), y.data(), s)); });
    report("rocblas", 0, shape, ms, 24.0 * n);
  }
  if (only.find("hot") != std::string::npos) {
    // --only=hot: just the production (default) configuration of the
    // temporal-blocking kernel, `iters` launches each — the target of
    // rocprofv3 --pmc passes (profiles/r02_pmc).  --hot-k=12,20 sweeps per
    // pass, --jacobi-n=32768.
    const int64_t n = cli.geti("jacobi-n", 32768);
    const std::string ks = cli.get("hot-k", "12,20");
    for (int K = 1; K <= GMT_TB_MAX_SWEEPS; ++K) {
      if (("," + ks + ",").find("," + std::to_string(K) + ",") == std::string::npos) continue;
      const int64_t g = K, xk = ((g + 7) / 8) * 8;
      const int64_t ld2 = ((xk + n + g + 63) / 64) * 64, rows = n + 2 * g;
      Buffer<double> a(static_cast<size_t>(ld2) * rows, GMT_SPACE_DEVICE), b(a.size(), GMT_SPACE_DEVICE);
      GMT_CHECK("fill", gmt_fill_poly(0, ld2, rows, 0.0, 1e-5, 0.0, 1e-5, a.data(), ld2, s));
      GMT_CHECK("fill", gmt_fill_poly(0, ld2, rows, 0.0, 1e-5, 0.0, 1e-5, b.data(), ld2, s));
      const int64_t rect[4] = {xk, n, g, n};
      gmt_tb_opts o{K, 0, 0, 0};
      const double ms = time_ms(s, iters, [&] {
        GMT_CHECK("tb", gmt_jacobi5tb(&o, 1, rect, rect, 0, a.data(), b.data(), ld2, rows, s));
      });
      char tag[64];
      std::snprintf(tag, sizeof(tag), "%lldx%lld x%d default", (long long)n, (long long)n, K);
      report("jacobi5tb", K, tag, ms, K * 16.0 * n * n);
      std::printf("%-10s    %-22s %9.1f MLUPS\n", "", tag, K * double(n) * n / (ms * 1e-3) / 1e6);
    }
  }
  if (only.find("tb") != std::string::npos) {
    // --only=tb: temporal-blocking kernel (jacobi5tb.hip),
    // --tb-k=12,14,16 --tb-nw=1,2,4,8 --tb-seg=0 --jacobi-n=32768
    // --tb-mask=0 (Dirichlet everywhere: rule workgroups at the edges)
    // --jacobi-ny=8192 --jacobi-nx=16384 (default: n x n)
    // --tb-shared=N (gmt_tb_opts.shared of the plain and the --tb-push=1 pass)
    const int64_t n = cli.geti("jacobi-n", 32768);
    // --jacobi-ny / --jacobi-nx: a rectangular domain (a strong-scaling share)
    const int64_t ny = cli.geti("jacobi-ny", n), nx = cli.geti("jacobi-nx", n);
    auto list = [&](const char* key, const char* def) {
      std::vector<int> v;
      std::string str = cli.get(key, def);
      size_t p = 0;
      while (p < str.size()) {
        size_t q = str.find(',', p);
        if (q == std::string::npos) q = str.size();
        v.push_back(std::atoi(str.substr(p, q - p).c_str()));
        p = q + 1;
      }
      return v;
    };
    const int mask = static_cast<int>(cli.geti("tb-mask", 0));
    const int shared = static_cast<int>(cli.geti("tb-shared", 0));
    for (int K : list("tb-k", "12,14,16")) {
      const int64_t g = K, xk = ((g + 7) / 8) * 8;
      const int64_t ld2 = ((xk + nx + g + 63) / 64) * 64, rows = ny + 2 * g;
      Buffer<double> a(static_cast<size_t>(ld2) * rows, GMT_SPACE_DEVICE), b(a.size(), GMT_SPACE_DEVICE);
      GMT_CHECK("fill", gmt_fill_poly(0, ld2, rows, 0.0, 1e-5, 0.0, 1e-5, a.data(), ld2, s));
      GMT_CHECK("fill", gmt_fill_poly(0, ld2, rows, 0.0, 1e-5, 0.0, 1e-5, b.data(), ld2, s));
      const int64_t rect[4] = {xk, nx, g, ny};
      for (int nw : list("tb-nw", "0"))
        for (int P : list("tb-p", "3"))
          for (int seg : list("tb-seg", "0")) {
            gmt_tb_opts o{K, nw, seg, 0};
            o.shared = shared;
            const double ms = time_ms(s, iters, [&] {
              GMT_CHECK("tb", gmt_jacobi5tb(&o, 1, rect, rect, mask, a.data(), b.data(), ld2, rows, s));
            });
            char tag[96];
            std::snprintf(tag, sizeof(tag), "%lldx%lld x%d nw%d P%d seg%d m%d", (long long)ny, (long long)nx, K, nw,
                          P, seg, mask);
            report("jacobi5tb", K, tag, ms, K * 16.0 * ny * nx);
            if (cli.geti("tb-push", 0) && K % 2 == 0 && gmt_jacobi5tb_push_supported(K)) {
              // --tb-push=1: the same pass with the inline halo exchange of a
              // one-rank periodic domain (the engine's layout: every face lands
              // in the opposite ghost ring of the output), alternated with the
              // plain pass so clock drift hits both alike
              gmt_tb_opts op = o;
              double* bb = b.data();
              const int64_t dy = ny * ld2, dx = nx;
              const double* tgt[8] = {bb + dy, bb - dy, bb + dx, bb - dx, bb + dy + dx, bb + dy - dx, bb - dy + dx, bb - dy - dx};
              for (int d = 0; d < 8; ++d) op.push[d] = tgt[d];  // GMT_PUSH_S, N, W, E, SW, SE, NW, NE
              op.push_w = g;  // even K: the faces fill the g-wide ghost ring
              // --tb-shared=N with a push pass in shared hand-off groups: the
              // per-strip push pass (shared = -1) joins the alternation, so one
              // run gives push-group, plain group and per-strip push
              gmt_tb_opts ops = op;
              ops.shared = -1;
              const int push_path = gmt_jacobi5tb_shared_path(&op, 1, rect, mask);
              for (int rep = 0; rep < 2; ++rep) {
                const double mp = time_ms(s, iters, [&] {
                  GMT_CHECK("tb push", gmt_jacobi5tb(&op, 1, rect, rect, mask, a.data(), b.data(), ld2, rows, s));
                });
                const double m0 = time_ms(s, iters, [&] {
                  GMT_CHECK("tb", gmt_jacobi5tb(&o, 1, rect, rect, mask, a.data(), b.data(), ld2, rows, s));
                });
                if (push_path > 0) {
                  const double m1 = time_ms(s, iters, [&] {
                    GMT_CHECK("tb push", gmt_jacobi5tb(&ops, 1, rect, rect, mask, a.data(), b.data(), ld2, rows, s));
                  });
                  std::printf("%-10s    %-30s push-group%d %.4f ms  plain %.4f ms  per-strip push %.4f ms  "
                              "ratio to plain %.4f  to per-strip push %.4f\n",
                              "", tag, push_path, mp, m0, m1, mp / m0, mp / m1);
                } else {
                  std::printf("%-10s    %-30s push %.4f ms  plain %.4f ms  ratio %.4f\n", "", tag, mp, m0, mp / m0);
                }
              }
              int64_t pp[6] = {};
              GMT_CHECK("plan", gmt_jacobi5tb_plan(&op, 1, rect, rect, mask, ld2, rows, pp));
              std::printf("%-10s    %-30s push plan: shared path %d (wgs %lld resident %lld threads %lld seg %lld x %lld vgpr %lld)\n",
                          "", tag, push_path, (long long)pp[0], (long long)pp[1], (long long)pp[2], (long long)pp[3],
                          (long long)pp[4], (long long)pp[5]);
            }
            int64_t pi[6] = {};
            GMT_CHECK("plan", gmt_jacobi5tb_plan(&o, 1, rect, rect, mask, ld2, rows, pi));
            std::printf("%-10s    %-30s %9.1f MLUPS  (shared path %d wgs %lld resident %lld threads %lld seg %lld x %lld vgpr %lld)\n",
                        "", tag, K * double(ny) * nx / (ms * 1e-3) / 1e6, gmt_jacobi5tb_shared_path(&o, 1, rect, mask),
                        (long long)pi[0], (long long)pi[1], (long long)pi[2], (long long)pi[3], (long long)pi[4],
                        (long long)pi[5]);
          }
    }
  }
  if (only.find("jacobi") != std::string::npos) {
    const int64_t n = cli.geti("jacobi-n", 32768);
    const int64_t xo = 8, ld = ((xo + n + 1 + 63) / 64) * 64;
    Buffer<double> u(static_cast<size_t>(ld) * (n + 2), GMT_SPACE_DEVICE), un(u.size(), GMT_SPACE_DEVICE);
    GMT_CHECK("fill", gmt_fill_poly(0, ld, n + 2, 0.0, 1e-5, 0.0, 1e-5, u.data(), ld, s));
    GMT_CHECK("fill", gmt_fill_poly(0, ld, n + 2, 0.0, 1e-5, 0.0, 1e-5, un.data(), ld, s));
    char shape[64];
    std::snprintf(shape, sizeof(shape), "%lldx%lld", (long long)n, (long long)n);
    // single sweep (the K-sweep kernel: --only=tb; A/B variants: variant_bench)
    const double ms = time_ms(s, iters, [&] {
      GMT_CHECK("jacobi", gmt_jacobi5(xo, n, 1, n, u.data(), un.data(), ld, nullptr, 0, 0.25, 0.0, nullptr, s));
    });
    report("jacobi5", 0, shape, ms, 16.0 * n * n);
  }
  if (only.find("stencil") != std::string::npos) {
    // the reference's default deriv shapes: 1028 x 524288 (dim 0), 524288 x 1028 (dim 1)
    const int64_t a = 1024, b = 512 * 1024;
    Buffer<double> in(static_cast<size_t>(a + 4) * b, GMT_SPACE_DEVICE), out(static_cast<size_t>(a) * b, GMT_SPACE_DEVICE);
    GMT_CHECK("fill", gmt_fill_poly(0, a + 4, b, 0.0, 1e-3, 0.0, 1e-3, in.data(), a + 4, s));
    const double c[5] = {1.0 / 12, -2.0 / 3, 0.0, 2.0 / 3, -1.0 / 12};
    // bytes: the input (n + 4 rows / columns) read once, the output written once
    const double bytes = 8.0 * ((a + 4) * b + a * b);
    double ms = time_ms(s, iters, [&] {
      GMT_CHECK("d0", gmt_stencil5_2d(0, a, b, c, 128.0, in.data(), a + 4, out.data(), a, s));
    });
    report("stencil5", 0, "dim0 1028->1024 x 524288", ms, bytes);
    ms = time_ms(s, iters, [&] {
      GMT_CHECK("d1", gmt_stencil5_2d(1, b, a, c, 128.0, in.data(), b, out.data(), b, s));
    });
    report("stencil5", 1, "dim1 524288 x 1028->1024", ms, bytes);
  }
  if (only.find("edges") != std::string::npos) {
    // --only=edges: the boundary-band split of the derivative at the
    // reference's shapes, --reps=5 rounds that alternate the variants (clock
    // drift hits all alike): the two 2-deep bands by one gmt_stencil5_2d_edges
    // launch against two gmt_stencil5_2d launches on the band sub-rectangles
    // (the only way without the band kernels), and interior + edges back to
    // back against the single full launch.
    const int64_t a = 1024, b = 512 * 1024;
    const int reps = static_cast<int>(cli.geti("reps", 5));
    Buffer<double> in(static_cast<size_t>(a + 4) * b, GMT_SPACE_DEVICE), out(static_cast<size_t>(a) * b, GMT_SPACE_DEVICE);
    GMT_CHECK("fill", gmt_fill_poly(0, a + 4, b, 0.0, 1e-3, 0.0, 1e-3, in.data(), a + 4, s));
    const double c[5] = {1.0 / 12, -2.0 / 3, 0.0, 2.0 / 3, -1.0 / 12};
    for (int dim = 0; dim < 2; ++dim) {
      const int64_t nx = dim == 0 ? a : b, ny = dim == 0 ? b : a, ld_in = dim == 0 ? a + 4 : b, ld_out = nx;
      const int64_t hi_in = dim == 0 ? a - 2 : (a - 2) * ld_in, hi_out = dim == 0 ? a - 2 : (a - 2) * ld_out;
      const int64_t bx = dim == 0 ? 2 : nx, by = dim == 0 ? ny : 2;
      const std::function<void()> variant[4] = {
          [&] {
            GMT_CHECK("band lo", gmt_stencil5_2d(dim, bx, by, c, 128.0, in.data(), ld_in, out.data(), ld_out, s));
            GMT_CHECK("band hi", gmt_stencil5_2d(dim, bx, by, c, 128.0, in.data() + hi_in, ld_in,
                                                 out.data() + hi_out, ld_out, s));
          },
          [&] { GMT_CHECK("edges", gmt_stencil5_2d_edges(dim, nx, ny, c, 128.0, in.data(), ld_in, out.data(), ld_out, 3, s)); },
          [&] { GMT_CHECK("full", gmt_stencil5_2d(dim, nx, ny, c, 128.0, in.data(), ld_in, out.data(), ld_out, s)); },
          [&] {
            GMT_CHECK("interior", gmt_stencil5_2d_interior(dim, nx, ny, c, 128.0, in.data(), ld_in, out.data(), ld_out, 3, s));
            GMT_CHECK("edges", gmt_stencil5_2d_edges(dim, nx, ny, c, 128.0, in.data(), ld_in, out.data(), ld_out, 3, s));
          }};
      const char* name[4] = {"2 x stencil5_2d bands", "stencil5_2d_edges", "stencil5_2d full", "interior + edges"};
      Stats st[4];
      for (int rep = 0; rep < reps; ++rep)
        for (int v = 0; v < 4; ++v) {
          const double ms = time_ms(s, iters, variant[v]);
          st[v].add(ms);
          std::printf("edges dim%d rep %d  %-22s %9.4f ms\n", dim, rep, name[v], ms);
        }
      for (int v = 0; v < 4; ++v)
        std::printf("edges dim%d summary %-22s min %9.4f  median %9.4f  max %9.4f ms  (range %.4f)\n", dim, name[v],
                    st[v].min(), st[v].median(), st[v].max(), st[v].max() - st[v].min());
      std::printf("edges dim%d  edges / bands = %.4f   (interior + edges) / full = %.4f  (medians)\n", dim,
                  st[1].median() / st[0].median(), st[3].median() / st[2].median());
    }
  }
  if (only.find("resid") != std::string::npos) {
    // --only=resid: the read-only residual (gmt_jacobi5_resid, A) against
    // what a residual cost before it existed (gmt_jacobi5 with resid: a whole
    // sweep, B) and the read-only streaming yardstick (gmt_sum over the same
    // number of doubles, C), at 8192^2 and 32768^2, --reps=5 rounds in the
    // order A B C C B A (clock drift hits all alike); the best of the rounds
    // is the figure compared.  --resid-n=N: one size only.
    const int reps = static_cast<int>(cli.geti("reps", 5));
    std::vector<int64_t> sizes = {8192, 32768};
    if (cli.has("resid-n")) sizes = {static_cast<int64_t>(cli.geti("resid-n", 8192))};
    for (const int64_t n : sizes) {
      const int64_t xo = 8, ld = ((xo + n + 1 + 63) / 64) * 64;
      Buffer<double> u(static_cast<size_t>(ld) * (n + 2), GMT_SPACE_DEVICE), un(u.size(), GMT_SPACE_DEVICE);
      GMT_CHECK("fill", gmt_fill_poly(0, ld, n + 2, 0.0, 1e-5, 0.0, 1e-5, u.data(), ld, s));
      GMT_CHECK("fill", gmt_fill_poly(0, ld, n + 2, 0.0, 1e-5, 0.0, 1e-5, un.data(), ld, s));
      Buffer<double> ws(static_cast<size_t>(gmt_jacobi5_resid_workspace(n, n)), GMT_SPACE_DEVICE), out(2, GMT_SPACE_DEVICE);
      Buffer<double> rws(static_cast<size_t>(gmt_jacobi_resid_workspace(n, n)) + 1, GMT_SPACE_DEVICE);
      Buffer<double> sws(static_cast<size_t>(gmt_sum_workspace(n * n)) + 1, GMT_SPACE_DEVICE);
      const std::function<void()> variant[3] = {
          [&] {
            GMT_CHECK("resid", gmt_jacobi5_resid(xo, n, 1, n, u.data(), ld, nullptr, 0, 0.25, 0.0, out.data(), ws.data(), s));
          },
          [&] {
            GMT_CHECK("jacobi+resid", gmt_jacobi5(xo, n, 1, n, u.data(), un.data(), ld, nullptr, 0, 0.25, 0.0, rws.data(), s));
          },
          [&] { GMT_CHECK("sum", gmt_sum(n * n, u.data(), out.data(), sws.data(), s)); }};
      const char* name[3] = {"jacobi5_resid", "jacobi5 + resid", "sum"};
      const double bytes[3] = {8.0 * n * n, 16.0 * n * n, 8.0 * n * n};
      int64_t seg = 0;
      const int path = gmt_jacobi5_resid_path(xo, n, n, u.data(), ld, nullptr, 0, &seg);
      std::printf("resid %lldx%lld  path %d, %lld rows per segment\n", (long long)n, (long long)n, path, (long long)seg);
      Stats st[3];
      const int order[6] = {0, 1, 2, 2, 1, 0};
      for (int rep = 0; rep < reps; ++rep)
        for (int k = 0; k < 6; ++k) {
          const int v = order[k];
          const double ms = time_ms(s, iters, variant[v]);
          st[v].add(ms);
          std::printf("resid %lldx%lld rep %d  %-16s %9.4f ms\n", (long long)n, (long long)n, rep, name[v], ms);
        }
      char shape[64];
      std::snprintf(shape, sizeof(shape), "%lldx%lld best", (long long)n, (long long)n);
      for (int v = 0; v < 3; ++v) {
        std::printf("resid %lldx%lld summary %-16s min %9.4f  median %9.4f  max %9.4f ms\n", (long long)n, (long long)n,
                    name[v], st[v].min(), st[v].median(), st[v].max());
        report(name[v], v, shape, st[v].min(), bytes[v]);
      }
      std::printf("resid %lldx%lld  resid / (jacobi5 + resid) = %.4f   sum / resid = %.4f  (best of %d)\n", (long long)n,
                  (long long)n, st[0].min() / st[1].min(), st[2].min() / st[0].min(), reps);
    }
  }
  if (only.find("add2d") != std::string::npos) {
    // --only=add2d: the add that ends a source block of the Jacobi engine
    // (gmt_add2d, A: the engine's layout — interior at column 8, pitch padded
    // to 64) against gmt_daxpy on the same number of elements (B: the same
    // 24 B per element, contiguous), at 8192^2 and 32768^2, --reps=5 rounds in
    // the order A B B A; the best of the rounds is compared.  --add2d-n=N: one size.
    const int reps = static_cast<int>(cli.geti("reps", 5));
    std::vector<int64_t> sizes = {8192, 32768};
    if (cli.has("add2d-n")) sizes = {static_cast<int64_t>(cli.geti("add2d-n", 8192))};
    for (const int64_t n : sizes) {
      const int64_t xo = 8, ld = ((xo + n + 1 + 63) / 64) * 64;
      Buffer<double> g(static_cast<size_t>(ld) * (n + 2), GMT_SPACE_DEVICE), u(g.size(), GMT_SPACE_DEVICE);
      GMT_CHECK("fill", gmt_fill_poly(0, ld, n + 2, 0.0, 1e-5, 0.0, 1e-5, u.data(), ld, s));
      GMT_CHECK("fill", gmt_fill_poly(3, ld, n + 2, 0.0, 1e-9, 0.0, 0.0, g.data(), ld, s));
      const std::function<void()> variant[2] = {
          [&] { GMT_CHECK("add2d", gmt_add2d(n, n, g.data() + ld + xo, ld, u.data() + ld + xo, ld, s)); },
          [&] { GMT_CHECK("daxpy", gmt_daxpy(n * n, 1e-3, g.data(), u.data(), s)); }};
      const char* name[2] = {"add2d", "daxpy"};
      std::printf("add2d %lldx%lld  path %d, pitch %lld\n", (long long)n, (long long)n,
                  gmt_add2d_path(n, g.data() + ld + xo, ld, u.data() + ld + xo, ld), (long long)ld);
      Stats st[2];
      const int order[4] = {0, 1, 1, 0};
      for (int rep = 0; rep < reps; ++rep)
        for (int k = 0; k < 4; ++k) {
          const int v = order[k];
          const double ms = time_ms(s, iters, variant[v]);
          st[v].add(ms);
          std::printf("add2d %lldx%lld rep %d  %-8s %9.4f ms\n", (long long)n, (long long)n, rep, name[v], ms);
        }
      char shape[64];
      std::snprintf(shape, sizeof(shape), "%lldx%lld best", (long long)n, (long long)n);
      for (int v = 0; v < 2; ++v) {
        std::printf("add2d %lldx%lld summary %-8s min %9.4f  median %9.4f  max %9.4f ms\n", (long long)n, (long long)n,
                    name[v], st[v].min(), st[v].median(), st[v].max());
        report(name[v], v, shape, st[v].min(), 24.0 * n * n);
      }
      std::printf("add2d %lldx%lld  add2d / daxpy = %.4f  (best of %d)\n", (long long)n, (long long)n,
                  st[0].min() / st[1].min(), reps);
    }
  }
  if (only.find("cg") != std::string::npos) {
    // --only=cg: the kernels of JacobiSolver::cg in the engine's layout
    // (interior at column 8, pitch padded to 64) at 8192^2, each against
    // gmt_daxpy on n * n contiguous elements (24 B per element), --reps=5
    // rounds in the order A B B A; the best of the rounds is compared.
    // GB/s from the compulsory bytes: apply 16, update 48, dir 24 B per point.
    const int reps = static_cast<int>(cli.geti("reps", 5));
    const int64_t n = cli.geti("cg-n", 8192);
    const int64_t xo = 8, ld = ((xo + n + 1 + 63) / 64) * 64;
    const size_t elems = static_cast<size_t>(ld) * (n + 2);
    Buffer<double> x(elems, GMT_SPACE_DEVICE), r(elems, GMT_SPACE_DEVICE), p(elems, GMT_SPACE_DEVICE),
        q(elems, GMT_SPACE_DEVICE), sc(8, GMT_SPACE_DEVICE),
        ws(static_cast<size_t>(gmt_cg_workspace(n, n)), GMT_SPACE_DEVICE);
    GMT_CHECK("fill", gmt_fill_poly(0, ld, n + 2, 0.0, 1e-5, 0.0, 1e-5, x.data(), ld, s));
    GMT_CHECK("fill", gmt_fill_poly(3, ld, n + 2, 0.0, 1e-9, 0.0, 0.0, r.data(), ld, s));
    GMT_CHECK("fill", gmt_fill_poly(0, ld, n + 2, 0.0, 1e-5, 0.0, 1e-5, p.data(), ld, s));
    GMT_CHECK("fill", gmt_fill_poly(3, ld, n + 2, 0.0, 1e-9, 0.0, 0.0, q.data(), ld, s));
    GMT_CHECK("sync", gmt_rt_stream_synchronize(s));
    // coefficients a = 1e-3 (update) and b = 0.5 (dir): the fields stay bounded over the repeats
    const double host_sc[8] = {1e-3, 1.0, 0.5, 1.0, 0, 0, 0, 0};
    GMT_CHECK("scalars", gmt_rt_memcpy(sc.data(), host_sc, sizeof(host_sc)));
    int64_t seg = 0;
    const int apply_path = gmt_cg_apply_path(xo, n, n, p.data(), ld, nullptr, 0, q.data(), ld, &seg);
    std::printf("cg %lldx%lld  apply path %d (%lld rows per segment), update path %d, dir path %d, pitch %lld\n",
                (long long)n, (long long)n, apply_path, (long long)seg,
                gmt_cg_update_path(xo, p.data(), ld, q.data(), ld, x.data(), ld, r.data(), ld),
                gmt_cg_dir_path(xo, r.data(), ld, p.data(), ld), (long long)ld);
    const std::function<void()> kernel[3] = {
        [&] { GMT_CHECK("cg_apply", gmt_cg_apply(0, xo, n, 1, n, p.data(), ld, nullptr, 0, 0.25, 0.0, q.data(), ld,
                                                 sc.data() + 4, ws.data(), s)); },
        [&] { GMT_CHECK("cg_update", gmt_cg_update(xo, n, 1, n, sc.data(), sc.data() + 1, p.data(), ld, q.data(), ld,
                                                   x.data(), ld, r.data(), ld, sc.data() + 6, ws.data(), s)); },
        [&] { GMT_CHECK("cg_dir", gmt_cg_dir(xo, n, 1, n, sc.data() + 2, sc.data() + 3, r.data(), ld, p.data(), ld, s)); }};
    const std::function<void()> daxpy = [&] { GMT_CHECK("daxpy", gmt_daxpy(n * n, 1e-3, q.data(), x.data(), s)); };
    const char* name[3] = {"cg_apply", "cg_update", "cg_dir"};
    const double bytes[3] = {16.0, 48.0, 24.0};
    for (int k = 0; k < 3; ++k) {
      Stats st[2];
      const int order[4] = {0, 1, 1, 0};
      for (int rep = 0; rep < reps; ++rep)
        for (int o = 0; o < 4; ++o) {
          const int v = order[o];
          const double ms = time_ms(s, iters, v == 0 ? kernel[k] : daxpy);
          st[v].add(ms);
          std::printf("cg %lldx%lld rep %d  %-9s %9.4f ms\n", (long long)n, (long long)n, rep, v == 0 ? name[k] : "daxpy",
                      ms);
        }
      char shape[64];
      std::snprintf(shape, sizeof(shape), "%lldx%lld best", (long long)n, (long long)n);
      report(name[k], 0, shape, st[0].min(), bytes[k] * n * n);
      report("daxpy", k + 1, shape, st[1].min(), 24.0 * n * n);
      std::printf("cg %lldx%lld  %s GB/s / daxpy GB/s = %.4f  (best of %d)\n", (long long)n, (long long)n, name[k],
                  (bytes[k] / st[0].min()) / (24.0 / st[1].min()), reps);
    }
  }
  if (only.find("cheby") != std::string::npos) {
    // --only=cheby: the launch of a JacobiSolver::cheby iteration
    // (gmt_cheby_step) in the engine's layout (interior at column 8, pitch
    // padded to 64) at 8192^2, without and with f, each against gmt_daxpy on
    // n * n contiguous elements, --reps=5 rounds in the order A B B A; the
    // best of the rounds is compared.  GB/s from the compulsory bytes: 24 B
    // per point, 32 with f.
    const int reps = static_cast<int>(cli.geti("reps", 5));
    const int64_t n = cli.geti("cheby-n", 8192);
    const int64_t xo = 8, ld = ((xo + n + 1 + 63) / 64) * 64;
    const size_t elems = static_cast<size_t>(ld) * (n + 2);
    Buffer<double> u(elems, GMT_SPACE_DEVICE), v(elems, GMT_SPACE_DEVICE), f(elems, GMT_SPACE_DEVICE);
    GMT_CHECK("fill", gmt_fill_poly(0, ld, n + 2, 0.0, 1e-5, 0.0, 1e-5, u.data(), ld, s));
    GMT_CHECK("fill", gmt_fill_poly(0, ld, n + 2, 0.0, 1e-5, 0.0, 1e-5, v.data(), ld, s));
    GMT_CHECK("fill", gmt_fill_poly(3, ld, n + 2, 0.0, 1e-9, 0.0, 0.0, f.data(), ld, s));
    GMT_CHECK("sync", gmt_rt_stream_synchronize(s));
    int64_t seg = 0, segf = 0;
    const int path = gmt_cheby_step_path(xo, n, n, u.data(), ld, nullptr, 0, v.data(), ld, &seg);
    const int pathf = gmt_cheby_step_path(xo, n, n, u.data(), ld, f.data(), ld, v.data(), ld, &segf);
    std::printf("cheby %lldx%lld  path %d (%lld rows per segment), with f %d (%lld), pitch %lld\n", (long long)n,
                (long long)n, path, (long long)seg, pathf, (long long)segf, (long long)ld);
    // w = 0.5: v converges to G(u), the fields stay bounded over the repeats
    const std::function<void()> kernel[2] = {
        [&] { GMT_CHECK("cheby_step", gmt_cheby_step(xo, n, 1, n, u.data(), ld, nullptr, 0, 0.25, 0.0, 0.5, v.data(),
                                                     ld, s)); },
        [&] { GMT_CHECK("cheby_step_f", gmt_cheby_step(xo, n, 1, n, u.data(), ld, f.data(), ld, 0.25, 1.0, 0.5,
                                                       v.data(), ld, s)); }};
    const std::function<void()> daxpy = [&] { GMT_CHECK("daxpy", gmt_daxpy(n * n, 1e-3, f.data(), u.data(), s)); };
    const char* name[2] = {"cheby_step", "cheby_step_f"};
    const double bytes[2] = {24.0, 32.0};
    for (int k = 0; k < 2; ++k) {
      Stats st[2];
      const int order[4] = {0, 1, 1, 0};
      for (int rep = 0; rep < reps; ++rep)
        for (int o = 0; o < 4; ++o) {
          const int w = order[o];
          const double ms = time_ms(s, iters, w == 0 ? kernel[k] : daxpy);
          st[w].add(ms);
          std::printf("cheby %lldx%lld rep %d  %-12s %9.4f ms\n", (long long)n, (long long)n, rep,
                      w == 0 ? name[k] : "daxpy", ms);
        }
      char shape[64];
      std::snprintf(shape, sizeof(shape), "%lldx%lld best", (long long)n, (long long)n);
      report(name[k], 0, shape, st[0].min(), bytes[k] * n * n);
      report("daxpy", k + 1, shape, st[1].min(), 24.0 * n * n);
      std::printf("cheby %lldx%lld  %s GB/s / daxpy GB/s = %.4f  (best of %d)\n", (long long)n, (long long)n, name[k],
                  (bytes[k] / st[0].min()) / (24.0 / st[1].min()), reps);
    }
  }
  if (only.find("mg") != std::string::npos) {
    // --only=mg: the three kernels of a JacobiSolver::mg cycle (gmt_mg_smooth
    // without and with f, gmt_mg_restrict, gmt_mg_prolong_add) on a fine level
    // of n x n (default 8191) and its (n-1)/2 coarse level, in the engine's
    // layout, each against gmt_daxpy on n * n contiguous elements, --reps=5
    // rounds in the order A B B A; the best of the rounds is compared.  GB/s
    // from the compulsory bytes per fine point: smooth 16 (24 with f), restrict
    // 8 + 2, prolong_add 16 + 2.
    const int reps = static_cast<int>(cli.geti("reps", 5));
    // an even --mg-n = N: the nested kernels at N - 1 and, in the same process,
    // the table-driven transfers of coarsen = any at N x N -> (N/2 - 1)^2
    const int64_t nt = cli.geti("mg-n", 8191), n = nt % 2 == 0 ? nt - 1 : nt, m = (n - 1) / 2;
    if (n < 3) {
      std::printf("ERROR: --mg-n must be >= 3\n");
      return 1;
    }
    const int64_t xo = 8, ld = ((xo + n + 1 + 63) / 64) * 64, ldc = ((xo + m + 1 + 63) / 64) * 64;
    const size_t elems = static_cast<size_t>(ld) * (n + 2), celems = static_cast<size_t>(ldc) * (m + 2);
    Buffer<double> u(elems, GMT_SPACE_DEVICE), v(elems, GMT_SPACE_DEVICE), f(elems, GMT_SPACE_DEVICE),
        e(celems, GMT_SPACE_DEVICE);
    GMT_CHECK("fill", gmt_fill_poly(0, ld, n + 2, 0.0, 1e-5, 0.0, 1e-5, u.data(), ld, s));
    GMT_CHECK("fill", gmt_fill_poly(0, ld, n + 2, 0.0, 1e-5, 0.0, 1e-5, v.data(), ld, s));
    GMT_CHECK("fill", gmt_fill_poly(3, ld, n + 2, 0.0, 1e-9, 0.0, 0.0, f.data(), ld, s));
    GMT_CHECK("fill", gmt_fill_poly(3, ldc, m + 2, 0.0, 1e-12, 0.0, 0.0, e.data(), ldc, s));
    GMT_CHECK("sync", gmt_rt_stream_synchronize(s));
    int64_t seg = 0, segf = 0;
    const int path = gmt_mg_smooth_path(xo, n, n, u.data(), ld, nullptr, 0, v.data(), ld, &seg);
    const int pathf = gmt_mg_smooth_path(xo, n, n, u.data(), ld, f.data(), ld, v.data(), ld, &segf);
    std::printf("mg %lldx%lld  smooth path %d (%lld rows per segment), with f %d (%lld), restrict path %d, prolong path "
                "%d, pitch %lld, coarse %lldx%lld pitch %lld\n", (long long)n, (long long)n, path, (long long)seg, pathf,
                (long long)segf, gmt_mg_restrict_path(xo, xo, u.data(), ld, e.data(), ldc),
                gmt_mg_prolong_add_path(xo, e.data(), ldc, v.data(), ld), (long long)ld, (long long)m, (long long)m,
                (long long)ldc);
    // prolong_add adds a field of 1e-12 a call: v stays bounded over the repeats
    const std::function<void()> kernel[4] = {
        [&] { GMT_CHECK("mg_smooth", gmt_mg_smooth(xo, n, 1, n, u.data(), ld, nullptr, 0, 0.25, 0.0, 0.8, v.data(), ld,
                                                   s)); },
        [&] { GMT_CHECK("mg_smooth_f", gmt_mg_smooth(xo, n, 1, n, u.data(), ld, f.data(), ld, 0.25, 1.0, 0.8, v.data(),
                                                     ld, s)); },
        [&] { GMT_CHECK("mg_restrict", gmt_mg_restrict(xo, n, 1, n, 1, 1, u.data(), ld, 0.25, e.data(), xo, 1, ldc, s)); },
        [&] { GMT_CHECK("mg_prolong_add", gmt_mg_prolong_add(xo, n, 1, n, 1, 1, e.data(), xo, 1, ldc, v.data(), ld, s)); }};
    const std::function<void()> daxpy = [&] { GMT_CHECK("daxpy", gmt_daxpy(n * n, 1e-3, f.data(), u.data(), s)); };
    const char* name[4] = {"mg_smooth", "mg_smooth_f", "mg_restrict", "mg_prolong_add"};
    const double bytes[4] = {16.0, 24.0, 10.0, 18.0};
    // one kernel against DAXPY on npts elements, in the order A B B A
    auto compare = [&](const char* nm, int idx, const std::function<void()>& fn, const std::function<void()>& dax,
                       double bytes_pt, int64_t side) {
      Stats st[2];
      const int order[4] = {0, 1, 1, 0};
      for (int rep = 0; rep < reps; ++rep)
        for (int o = 0; o < 4; ++o) {
          const int w = order[o];
          const double ms = time_ms(s, iters, w == 0 ? fn : dax);
          st[w].add(ms);
          std::printf("mg %lldx%lld rep %d  %-18s %9.4f ms\n", (long long)side, (long long)side, rep,
                      w == 0 ? nm : "daxpy", ms);
        }
      char shape[64];
      std::snprintf(shape, sizeof(shape), "%lldx%lld best", (long long)side, (long long)side);
      report(nm, 0, shape, st[0].min(), bytes_pt * side * side);
      report("daxpy", idx + 1, shape, st[1].min(), 24.0 * side * side);
      std::printf("mg %lldx%lld  %s GB/s / daxpy GB/s = %.4f  (best of %d)\n", (long long)side, (long long)side, nm,
                  (bytes_pt / st[0].min()) / (24.0 / st[1].min()), reps);
      return st[0].min();
    };
    double best[4] = {0, 0, 0, 0};
    for (int k = 0; k < 4; ++k) {
      if (k == 3) GMT_CHECK("fill", gmt_fill_poly(3, ldc, m + 2, 0.0, 1e-12, 0.0, 0.0, e.data(), ldc, s));
      best[k] = compare(name[k], k, kernel[k], daxpy, bytes[k], n);
    }
    {
      // the fused smoother (gmt_mg_smooth_k, mask 0) for k = 2, 3, 4 without and with f: first compared
      // bitwise with k single sweeps between two buffers that hold u's ring, then timed beside those k
      // launches and DAXPY in the order A B C C B A.  GB/s from the same compulsory 16 (24) bytes a point.
      Buffer<double> w(elems, GMT_SPACE_DEVICE), x(elems, GMT_SPACE_DEVICE);
      Buffer<double> dws(static_cast<size_t>(2 * gmt_diff_sq_workspace(n, n)) + 2, GMT_SPACE_DEVICE);
      GMT_CHECK("memset", gmt_rt_memset_async(w.data(), 0, w.bytes(), s));
      for (int k = 2; k <= GMT_MG_MAX_FUSE; ++k)
        for (int wf = 0; wf < 2; ++wf) {
          // the same field and ring in the three buffers (DAXPY below updates u)
          for (double* b : {u.data(), v.data(), x.data()})
            GMT_CHECK("fill", gmt_fill_poly(0, ld, n + 2, 0.0, 1e-5, 0.0, 1e-5, b, ld, s));
          const double* fp = wf ? f.data() : nullptr;
          const int64_t ldf = wf ? ld : 0;
          const double c1 = wf ? 1.0 : 0.0, bpp = wf ? 24.0 : 16.0;
          char nm[32], nms[32], nmd[32];
          std::snprintf(nm, sizeof(nm), "mg_smooth_k%d%s", k, wf ? "_f" : "");
          std::snprintf(nms, sizeof(nms), "mg_smooth_x%d%s", k, wf ? "_f" : "");
          std::snprintf(nmd, sizeof(nmd), "daxpy_k%d%s", k, wf ? "_f" : "");
          const std::function<void()> fused = [&] {
            GMT_CHECK(nm, gmt_mg_smooth_k(k, xo, n, 1, n, 0, u.data(), ld, fp, ldf, 0.25, c1, 0.8, w.data(), ld, s));
          };
          // u -> v -> x -> v ...: the result is in v for an odd k, in x for an even one
          const std::function<void()> singles = [&] {
            const double* src = u.data();
            for (int j = 0; j < k; ++j) {
              double* dst = j % 2 == 0 ? v.data() : x.data();
              GMT_CHECK(nms, gmt_mg_smooth(xo, n, 1, n, src, ld, fp, ldf, 0.25, c1, 0.8, dst, ld, s));
              src = dst;
            }
          };
          int64_t segk = 0;
          const int pk = gmt_mg_smooth_k_path(k, xo, n, n, 0, u.data(), ld, fp, ldf, w.data(), ld, &segk);
          fused();
          singles();
          const double* last = k % 2 ? v.data() : x.data();
          GMT_CHECK("diff", gmt_diff_bits(n, n, w.data() + ld + xo, ld, last + ld + xo, ld, dws.data(), dws.data() + 2, s));
          double dres[2] = {-1.0, -1.0};
          GMT_CHECK("D2H", gmt_rt_memcpy_async(dres, dws.data(), sizeof(dres), s));
          GMT_CHECK("sync", gmt_rt_stream_synchronize(s));
          std::printf("mg %lldx%lld  %s path %d (%lld rows per segment), %s bitwise %d x mg_smooth: %s\n", (long long)n,
                      (long long)n, nm, pk, (long long)segk, nm, k, dres[1] == 0.0 ? "yes" : "NO");
          if (dres[1] != 0.0) return 1;
          Stats st[3];
          const int order[6] = {0, 1, 2, 2, 1, 0};
          const std::function<void()>* fn[3] = {&fused, &singles, &daxpy};
          const char* label[3] = {nm, nms, "daxpy"};
          for (int rep = 0; rep < reps; ++rep)
            for (int o = 0; o < 6; ++o) {
              const double ms = time_ms(s, iters, *fn[order[o]]);
              st[order[o]].add(ms);
              std::printf("mg %lldx%lld rep %d  %-18s %9.4f ms\n", (long long)n, (long long)n, rep, label[order[o]], ms);
            }
          char shape[64];
          std::snprintf(shape, sizeof(shape), "%lldx%lld best", (long long)n, (long long)n);
          report(nm, 0, shape, st[0].min(), bpp * n * n);
          report(nms, 0, shape, st[1].min(), bpp * k * n * n);
          report(nmd, 0, shape, st[2].min(), 24.0 * n * n);
          std::printf("mg %lldx%lld  %s ms / %d x mg_smooth ms = %.4f, GB/s / daxpy GB/s = %.4f  (best of %d)\n",
                      (long long)n, (long long)n, nm, k, st[0].min() / st[1].min(),
                      (bpp / st[0].min()) / (24.0 / st[2].min()), reps);
        }
    }
    {
      // the red-black smoother (gmt_mg_smooth_rb, mask 0, par 0) for h = 1, 2, 4 half-sweeps without and with
      // f: first compared bitwise with h launches of h = 1 whose par alternates, between two buffers that hold
      // u's ring, then timed beside gmt_mg_smooth_k of k = h (the same walk without the colour) in the order
      // A B B A.  GB/s from the same compulsory 16 (24) bytes a point.
      Buffer<double> w(elems, GMT_SPACE_DEVICE), x(elems, GMT_SPACE_DEVICE);
      Buffer<double> dws(static_cast<size_t>(2 * gmt_diff_sq_workspace(n, n)) + 2, GMT_SPACE_DEVICE);
      GMT_CHECK("memset", gmt_rt_memset_async(w.data(), 0, w.bytes(), s));
      for (int h : {1, 2, 4})
        for (int wf = 0; wf < 2; ++wf) {
          for (double* b : {u.data(), v.data(), x.data()})
            GMT_CHECK("fill", gmt_fill_poly(0, ld, n + 2, 0.0, 1e-5, 0.0, 1e-5, b, ld, s));
          const double* fp = wf ? f.data() : nullptr;
          const int64_t ldf = wf ? ld : 0;
          const double c1 = wf ? 1.0 : 0.0, bpp = wf ? 24.0 : 16.0;
          char nm[32], nmk[32];
          std::snprintf(nm, sizeof(nm), "mg_smooth_rb%d%s", h, wf ? "_f" : "");
          std::snprintf(nmk, sizeof(nmk), "mg_smooth_k%d%s", h, wf ? "_f" : "");
          const std::function<void()> rb = [&] {
            GMT_CHECK(nm, gmt_mg_smooth_rb(h, 0, xo, n, 1, n, 0, u.data(), ld, fp, ldf, 0.25, c1, 1.0, w.data(), ld, s));
          };
          const std::function<void()> jac = [&] {
            GMT_CHECK(nmk, gmt_mg_smooth_k(h, xo, n, 1, n, 0, u.data(), ld, fp, ldf, 0.25, c1, 0.8, w.data(), ld, s));
          };
          int64_t segh = 0;
          const int ph = gmt_mg_smooth_rb_path(h, 0, xo, n, n, 0, u.data(), ld, fp, ldf, w.data(), ld, &segh);
          rb();
          const double* src = u.data();  // u -> v -> x -> v ...
          for (int j = 0; j < h; ++j) {
            double* dst = j % 2 == 0 ? v.data() : x.data();
            GMT_CHECK(nm, gmt_mg_smooth_rb(1, j % 2, xo, n, 1, n, 0, src, ld, fp, ldf, 0.25, c1, 1.0, dst, ld, s));
            src = dst;
          }
          GMT_CHECK("diff", gmt_diff_bits(n, n, w.data() + ld + xo, ld, src + ld + xo, ld, dws.data(), dws.data() + 2, s));
          double dres[2] = {-1.0, -1.0};
          GMT_CHECK("D2H", gmt_rt_memcpy_async(dres, dws.data(), sizeof(dres), s));
          GMT_CHECK("sync", gmt_rt_stream_synchronize(s));
          std::printf("mg %lldx%lld  %s path %d (%lld rows per segment), %s bitwise %d x mg_smooth_rb1: %s\n",
                      (long long)n, (long long)n, nm, ph, (long long)segh, nm, h, dres[1] == 0.0 ? "yes" : "NO");
          if (dres[1] != 0.0) return 1;
          Stats st[2];
          const int order[4] = {0, 1, 1, 0};
          for (int rep = 0; rep < reps; ++rep)
            for (int o = 0; o < 4; ++o) {
              const double ms = time_ms(s, iters, order[o] == 0 ? rb : jac);
              st[order[o]].add(ms);
              std::printf("mg %lldx%lld rep %d  %-18s %9.4f ms\n", (long long)n, (long long)n, rep,
                          order[o] == 0 ? nm : nmk, ms);
            }
          char shape[64];
          std::snprintf(shape, sizeof(shape), "%lldx%lld best", (long long)n, (long long)n);
          report(nm, 0, shape, st[0].min(), bpp * n * n);
          report(nmk, 0, shape, st[1].min(), bpp * n * n);
          std::printf("mg %lldx%lld  %s ms / %s ms = %.4f  (best of %d)\n", (long long)n, (long long)n, nm, nmk,
                      st[0].min() / st[1].min(), reps);
        }
    }
    {
      // the fused transfer (gmt_mg_resid_restrict, mask 0) without and with f: first compared bitwise with
      // gmt_cg_apply mode 1 into a field whose ring is zero followed by gmt_mg_restrict, then timed beside those
      // two launches in the order A B B A.  The byte model per fine point: 8 + 2 against 16 + 10 (16 + 2 against
      // 24 + 10 with f).
      Buffer<double> d(elems, GMT_SPACE_DEVICE), e2(celems, GMT_SPACE_DEVICE);
      Buffer<double> cws(static_cast<size_t>(gmt_cg_workspace(n, n)) + 2, GMT_SPACE_DEVICE);
      Buffer<double> dws(static_cast<size_t>(2 * gmt_diff_sq_workspace(m, m)) + 2, GMT_SPACE_DEVICE);
      GMT_CHECK("memset", gmt_rt_memset_async(d.data(), 0, d.bytes(), s));
      GMT_CHECK("fill", gmt_fill_poly(0, ld, n + 2, 0.0, 1e-5, 0.0, 1e-5, u.data(), ld, s));
      for (int wf = 0; wf < 2; ++wf) {
        const double* fp = wf ? f.data() : nullptr;
        const int64_t ldf = wf ? ld : 0;
        const double c1 = wf ? 1.0 : 0.0;
        const char* nm = wf ? "mg_resid_restrict_f" : "mg_resid_restrict";
        const char* nmp = wf ? "cg_apply+restrict_f" : "cg_apply+restrict";
        const std::function<void()> fused = [&] {
          GMT_CHECK(nm, gmt_mg_resid_restrict(xo, n, 1, n, 1, 1, 0, u.data(), ld, fp, ldf, 0.25, c1, 0.25, e.data(), xo,
                                              1, ldc, s));
        };
        const std::function<void()> pair = [&] {
          GMT_CHECK(nmp, gmt_cg_apply(1, xo, n, 1, n, u.data(), ld, fp, ldf, 0.25, c1, d.data(), ld, cws.data(),
                                      cws.data() + 2, s));
          GMT_CHECK(nmp, gmt_mg_restrict(xo, n, 1, n, 1, 1, d.data(), ld, 0.25, e2.data(), xo, 1, ldc, s));
        };
        int64_t segr = 0;
        const int pr = gmt_mg_resid_restrict_path(xo, n, 1, n, 1, 1, 0, u.data(), ld, fp, ldf, e.data(), xo, 1, ldc, &segr);
        fused();
        pair();
        GMT_CHECK("diff", gmt_diff_bits(m, m, e.data() + ldc + xo, ldc, e2.data() + ldc + xo, ldc, dws.data(),
                                        dws.data() + 2, s));
        double dres[2] = {-1.0, -1.0};
        GMT_CHECK("D2H", gmt_rt_memcpy_async(dres, dws.data(), sizeof(dres), s));
        GMT_CHECK("sync", gmt_rt_stream_synchronize(s));
        std::printf("mg %lldx%lld  %s path %d (%lld rows per segment), %s bitwise cg_apply + mg_restrict: %s\n",
                    (long long)n, (long long)n, nm, pr, (long long)segr, nm, dres[1] == 0.0 ? "yes" : "NO");
        if (dres[1] != 0.0) return 1;
        Stats st[2];
        const int order[4] = {0, 1, 1, 0};
        for (int rep = 0; rep < reps; ++rep)
          for (int o = 0; o < 4; ++o) {
            const double ms = time_ms(s, iters, order[o] == 0 ? fused : pair);
            st[order[o]].add(ms);
            std::printf("mg %lldx%lld rep %d  %-18s %9.4f ms\n", (long long)n, (long long)n, rep,
                        order[o] == 0 ? nm : nmp, ms);
          }
        char shape[64];
        std::snprintf(shape, sizeof(shape), "%lldx%lld best", (long long)n, (long long)n);
        report(nm, 0, shape, st[0].min(), (wf ? 18.0 : 10.0) * n * n);
        report(nmp, 0, shape, st[1].min(), (wf ? 34.0 : 26.0) * n * n);
        std::printf("mg %lldx%lld  %s ms / (cg_apply + mg_restrict) ms = %.4f, bytes model %s  (best of %d)\n",
                    (long long)n, (long long)n, nm, st[0].min() / st[1].min(), wf ? "18/34" : "10/26", reps);
      }
    }
    {
      // the interpolation fused into the first post-smoothing pass (gmt_mg_prolong_smooth, mask 0) for h = 1, 2, 4
      // sweeps (Jacobi) and half-sweeps (red-black), without and with f: first compared bitwise with
      // gmt_mg_prolong_add on a copy of u followed by gmt_mg_smooth_k / gmt_mg_smooth_rb, then timed beside those
      // two launches in the order A B B A.  The byte model per fine point: 16 + 2 against 18 + 16 (24 + 2 against
      // 18 + 24 with f), whatever h.  The pair's prolong_add adds a field of 1e-12 a call: v stays bounded.
      Buffer<double> w(elems, GMT_SPACE_DEVICE), x(elems, GMT_SPACE_DEVICE);
      Buffer<double> dws(static_cast<size_t>(2 * gmt_diff_sq_workspace(n, n)) + 2, GMT_SPACE_DEVICE);
      GMT_CHECK("memset", gmt_rt_memset_async(w.data(), 0, w.bytes(), s));
      GMT_CHECK("memset", gmt_rt_memset_async(x.data(), 0, x.bytes(), s));
      GMT_CHECK("fill", gmt_fill_poly(3, ldc, m + 2, 0.0, 1e-12, 0.0, 0.0, e.data(), ldc, s));
      for (int rb = 0; rb < 2; ++rb)
        for (int h : {1, 2, 4})
          for (int wf = 0; wf < 2; ++wf) {
            for (double* b : {u.data(), v.data()})
              GMT_CHECK("fill", gmt_fill_poly(0, ld, n + 2, 0.0, 1e-5, 0.0, 1e-5, b, ld, s));
            const double* fp = wf ? f.data() : nullptr;
            const int64_t ldf = wf ? ld : 0;
            const double c1 = wf ? 1.0 : 0.0, om = rb ? 1.0 : 0.8;
            char nm[40], nmp[40];
            std::snprintf(nm, sizeof(nm), "mg_prolong_%s%d%s", rb ? "rb" : "k", h, wf ? "_f" : "");
            std::snprintf(nmp, sizeof(nmp), "prolong_add+%s%d%s", rb ? "rb" : "k", h, wf ? "_f" : "");
            const std::function<void()> fused = [&] {
              GMT_CHECK(nm, gmt_mg_prolong_smooth(h, rb, 0, xo, n, 1, n, 1, 1, 0, e.data(), xo, 1, ldc, u.data(), ld, fp,
                                                  ldf, 0.25, c1, om, w.data(), ld, s));
            };
            const std::function<void()> pair = [&] {
              GMT_CHECK(nmp, gmt_mg_prolong_add(xo, n, 1, n, 1, 1, e.data(), xo, 1, ldc, v.data(), ld, s));
              if (rb)
                GMT_CHECK(nmp, gmt_mg_smooth_rb(h, 0, xo, n, 1, n, 0, v.data(), ld, fp, ldf, 0.25, c1, om, x.data(), ld, s));
              else
                GMT_CHECK(nmp, gmt_mg_smooth_k(h, xo, n, 1, n, 0, v.data(), ld, fp, ldf, 0.25, c1, om, x.data(), ld, s));
            };
            int64_t segp = 0;
            const int pp = gmt_mg_prolong_smooth_path(h, rb, 0, xo, n, 1, n, 1, 1, 0, e.data(), xo, 1, ldc, u.data(), ld,
                                                      fp, ldf, w.data(), ld, &segp);
            fused();
            pair();  // v is u here: the first correction
            GMT_CHECK("diff", gmt_diff_bits(n, n, w.data() + ld + xo, ld, x.data() + ld + xo, ld, dws.data(),
                                            dws.data() + 2, s));
            double dres[2] = {-1.0, -1.0};
            GMT_CHECK("D2H", gmt_rt_memcpy_async(dres, dws.data(), sizeof(dres), s));
            GMT_CHECK("sync", gmt_rt_stream_synchronize(s));
            std::printf("mg %lldx%lld  %s path %d (%lld rows per segment), %s bitwise mg_prolong_add + mg_smooth_%s: %s\n",
                        (long long)n, (long long)n, nm, pp, (long long)segp, nm, rb ? "rb" : "k",
                        dres[1] == 0.0 ? "yes" : "NO");
            if (dres[1] != 0.0) return 1;
            Stats st[2];
            const int order[4] = {0, 1, 1, 0};
            for (int rep = 0; rep < reps; ++rep)
              for (int o = 0; o < 4; ++o) {
                const double ms = time_ms(s, iters, order[o] == 0 ? fused : pair);
                st[order[o]].add(ms);
                std::printf("mg %lldx%lld rep %d  %-18s %9.4f ms\n", (long long)n, (long long)n, rep,
                            order[o] == 0 ? nm : nmp, ms);
              }
            char shape[64];
            std::snprintf(shape, sizeof(shape), "%lldx%lld best", (long long)n, (long long)n);
            report(nm, 0, shape, st[0].min(), (wf ? 26.0 : 18.0) * n * n);
            report(nmp, 0, shape, st[1].min(), (wf ? 42.0 : 34.0) * n * n);
            std::printf("mg %lldx%lld  %s ms / (mg_prolong_add + mg_smooth_%s) ms = %.4f, bytes model %s  (best of %d)\n",
                        (long long)n, (long long)n, nm, rb ? "rb" : "k", st[0].min() / st[1].min(),
                        wf ? "26/42" : "18/34", reps);
          }
    }
    if (nt % 2 == 0) {
      // the general transfers on nt x nt: d with room for a 2-wide ring (interior origin (8, 2)), the same
      // compulsory bytes per fine point as the nested pair; each beside DAXPY on nt * nt elements and beside
      // the nested kernel's best time above
      const int64_t mt = nt / 2 - 1;
      const int64_t ldt = ((xo + nt + 2 + 63) / 64) * 64, ldct = ((xo + mt + 1 + 63) / 64) * 64;
      const size_t telems = static_cast<size_t>(ldt) * (nt + 4);
      Buffer<double> dt(telems, GMT_SPACE_DEVICE), vt(telems, GMT_SPACE_DEVICE), ft(telems, GMT_SPACE_DEVICE),
          et(static_cast<size_t>(ldct) * (mt + 2), GMT_SPACE_DEVICE);
      GMT_CHECK("fill", gmt_fill_poly(0, ldt, nt + 4, 0.0, 1e-5, 0.0, 1e-5, dt.data(), ldt, s));
      GMT_CHECK("fill", gmt_fill_poly(0, ldt, nt + 4, 0.0, 1e-5, 0.0, 1e-5, vt.data(), ldt, s));
      GMT_CHECK("fill", gmt_fill_poly(3, ldt, nt + 4, 0.0, 1e-9, 0.0, 0.0, ft.data(), ldt, s));
      GMT_CHECK("fill", gmt_fill_poly(3, ldct, mt + 2, 0.0, 1e-12, 0.0, 0.0, et.data(), ldct, s));
      GMT_CHECK("sync", gmt_rt_stream_synchronize(s));
      const gmt_mg_xfer_desc desc{{nt, nt}, {mt, mt}, {0, 0}, {nt, nt}, {0, 0}, {mt, mt}};
      void* plan = nullptr;
      GMT_CHECK("plan", gmt_mg_xfer_plan_create(&desc, &plan));
      std::printf("mg %lldx%lld  restrict_tab path %d, prolong_add_tab path %d, pitch %lld, coarse %lldx%lld pitch "
                  "%lld\n", (long long)nt, (long long)nt, gmt_mg_restrict_tab_path(xo, xo, dt.data(), ldt, et.data(), ldct),
                  gmt_mg_prolong_add_tab_path(xo, et.data(), ldct, vt.data(), ldt), (long long)ldt, (long long)mt,
                  (long long)mt, (long long)ldct);
      const std::function<void()> daxpyt = [&] { GMT_CHECK("daxpy", gmt_daxpy(nt * nt, 1e-3, ft.data(), dt.data(), s)); };
      const double tr = compare("mg_restrict_tab", 4, [&] {
        GMT_CHECK("mg_restrict_tab", gmt_mg_restrict_tab(plan, xo, 2, dt.data(), ldt, et.data(), xo, 1, ldct, s));
      }, daxpyt, 10.0, nt);
      GMT_CHECK("fill", gmt_fill_poly(3, ldct, mt + 2, 0.0, 1e-12, 0.0, 0.0, et.data(), ldct, s));
      const double tp = compare("mg_prolong_add_tab", 5, [&] {
        GMT_CHECK("mg_prolong_add_tab", gmt_mg_prolong_add_tab(plan, xo, 2, et.data(), xo, 1, ldct, vt.data(), ldt, s));
      }, daxpyt, 18.0, nt);
      GMT_CHECK("sync", gmt_rt_stream_synchronize(s));
      gmt_mg_xfer_plan_destroy(plan);
      std::printf("mg %lldx%lld  mg_restrict_tab ms / mg_restrict ms at %lld = %.4f, mg_prolong_add_tab ms / "
                  "mg_prolong_add ms = %.4f\n", (long long)nt, (long long)nt, (long long)n, tr / best[2], tp / best[3]);
    }
  }
  if (only.find("pack") != std::string::npos) {
    // dim-0 halo faces of the reference's field: 2 rows x 524288 columns, pitch 1028
    const int64_t ld = 1028, ny = 512 * 1024;
    Buffer<double> z(static_cast<size_t>(ld) * ny, GMT_SPACE_DEVICE), b0(2 * ny, GMT_SPACE_DEVICE),
        b1(2 * ny, GMT_SPACE_DEVICE);
    gmt_copy2d_desc d[2] = {{z.data() + 2, b0.data(), ld, 2, 2, ny}, {z.data() + 1024, b1.data(), ld, 2, 2, ny}};
    const double ms = time_ms(s, iters, [&] { GMT_CHECK("pack", gmt_copy2d_batched(2, d, 8, s)); });
    report("pack", 0, "2 faces 2x524288", ms, 2.0 * 2 * 16.0 * ny);
  }
  gmt_rt_stream_destroy(s);
  return 0;
}
