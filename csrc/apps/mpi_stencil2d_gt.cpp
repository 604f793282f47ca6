// mpi_stencil2d_gt — the reference's main benchmark, MI355X-native.
//
// Reference: /root/reference/mpi_stencil2d_gt.cc:651-734.  Same positional
// CLI `[n_local_deriv] [n_iter]`, same header, same 8 test_deriv lines
// ({dim0, dim1} x {device, managed} x {buf 1, 0}) and 4 test_sum lines, same
// timing semantics (exchange wall time summed over timed iterations and over
// ranks, MPI_Reduce to rank 0).
//
// Where a TEST line's number is not measured the reference's way it says so
// in a bracketed tag after the reference's fields:
//   [persistent buffers]  the halo staging buffers and exchange plan are
//                         created once; the reference allocates its buffers
//                         inside every timed call (mpi_stencil2d_gt.cc:141-156;
//                         --alloc-per-call re-creates them per call: no tag)
//   [managed: host-resident, xnack off]  managed memory on a GPU running with
//                         XNACK off is not migrated: those lines time
//                         pinned-host memory over PCIe.
//
// Options (not in the reference):
//   --transport=auto|mpi-host|mpi-direct|rccl|ipc   force one data plane
//   --no-managed          skip the managed-memory variants (TEST_MANAGED off)
//   --tests=deriv,sum     subset
//   --host-init --host-verify   reference host loops instead of GPU fill/check
//   --alloc-per-call      re-create halo buffers inside the timed region (the
//                         reference's semantics; default: persistent, tagged)
//   --json=FILE           one JSON record per test (per-exchange µs, GB/s, transport)
//   --dim=0|1 --mem=device|managed --buf=0|1   run one slice of the test matrix
//   --iters=N --warmup=W  (positional n_iter still wins when given; warmup default 5)
//   --timeout=S           hang watchdog (gmt/watchdog.hpp)
//   --check               compare the ghost rows with the analytic field after EVERY
//                         exchange (GMT_CORRUPT_GHOST=R:K injects a bad cell); exit 5 on a mismatch
//   --overlap             after each derivative test, time whole steps (exchange + derivative
//                         through to completion) in two orders, interleaved: the serial one
//                         above, and one that runs the exchange on a high-priority stream
//                         beside the interior of the derivative and then the ghost-dependent
//                         bands (gmt_stencil5_2d_interior / _edges, gmt/deriv.hpp).  One more
//                         line per test, seconds summed over timed steps and ranks:
//                         "STEP dim:%d, %s, buf:%d; serial=%0.8f, overlap=%0.8f [transport]";
//                         err= is then the last overlapped step's.  With --check the line
//                         carries step_err=, the largest err_norm any overlapped step's
//                         derivative had on any rank; exit 5 above n_global / 192 (half of
//                         what one stale ghost cell costs)
//   --debug               the reference's DEBUG-build per-rank lines: "%d/%d exchange time
//                         %0.8f ms" and "%d/%d [%d:0x%08x] err_norm = %.8f" after each
//                         test_deriv, "%d/%d allreduce time %0.8f ms" after each test_sum
//                         (mpi_stencil2d_gt.cc:536-539,557-560,635-638)
#include <mpi.h>

#include <cstdio>
#include <cstdlib>
#include <string>

#include "deriv_common.hpp"
#include "gmt/device.hpp"

using namespace gmt;
using namespace gmt::apps;

int main(int argc, char** argv) {
  Cli cli(argc, argv);
  size_t n_local_deriv = 1024;
  int n_iter = static_cast<int>(cli.geti("iters", 1000));
  const int n_warmup = static_cast<int>(cli.geti("warmup", 5));
  if (cli.positional(0)) n_local_deriv = std::atol(cli.positional(0));
  if (cli.positional(1)) n_iter = std::atoi(cli.positional(1));
  const int only_dim = static_cast<int>(cli.geti("dim", -1));
  const std::string only_mem = cli.get("mem", "");
  const int only_buf = static_cast<int>(cli.geti("buf", -1));
  const size_t n_global_other = static_cast<size_t>(cli.geti("n-other", 512 * 1024));
  const bool managed = !cli.flag("no-managed") && only_mem != "device";
  const bool alloc_per_call = cli.flag("alloc-per-call");
  const std::string tests = cli.get("tests", "deriv,sum");
  const std::string json = cli.get("json", "");
  const bool debug = cli.flag("debug");
  const bool overlap = cli.flag("overlap");

  mpi_init_pinned(&argc, &argv);  // pinned near the GPU first (gmt/device.hpp)
  int world_size = 1, world_rank = 0;
  GMT_MPI_CHECK(MPI_Comm_size(MPI_COMM_WORLD, &world_size));
  GMT_MPI_CHECK(MPI_Comm_rank(MPI_COMM_WORLD, &world_rank));
  const size_t n_global_deriv = n_local_deriv * world_size;

  RankBinding b = set_rank_device(MPI_COMM_WORLD, false);

  if (world_rank == 0) {
    std::printf("n procs        = %d\n", world_size);
    std::printf("n_global_deriv = %zu\n", n_global_deriv);
    std::printf("n_global_other = %zu\n", n_global_other);
    std::printf("n_iter         = %d\n", n_iter);
    // byte parity with the reference header: it prints its variable's 10,
    // which no test uses (each runs 5 warm-up iterations,
    // mpi_stencil2d_gt.cc:658,687,693); an explicit --warmup prints itself
    std::printf("n_warmup       = %d\n", cli.get("warmup", "").empty() ? 10 : n_warmup);
    std::printf("# n_warmup: the tests run %d warm-up iterations each (the reference: 5, whatever its header "
                "says)\n", n_warmup);
    std::printf("# backend=%s device=%s arch=%s managed_memory=%d xnack=%d\n",
                gmt_rt_backend_name(), b.info.name, b.info.arch, b.info.managed_memory,
                b.info.xnack);
  }
  std::fflush(stdout);

  auto pool_owner = std::make_unique<TransportPool>(MPI_COMM_WORLD, b);
  TransportPool& pool = *pool_owner;
  const comm::Kind want = comm::parse_kind(cli.get("transport", "auto"));

  // bracketed tags after the reference's fields (see the header comment)
  const bool host_resident_managed = gmt_rt_backend() != GMT_BACKEND_HOST && !b.info.xnack;
  auto tags = [&](int space, bool exchange) {
    std::string t;
    if (exchange && !alloc_per_call) t += " [persistent buffers]";
    if (space == GMT_SPACE_MANAGED && host_resident_managed) t += " [managed: host-resident, xnack off]";
    return t;
  };
  auto report = [&](const char* name, int dim, int space, bool buf, const DerivResult& r) {
    if (debug) {  // every rank, as the reference's DEBUG build (mpi_stencil2d_gt.cc:536-539,557-560)
      std::printf("%d/%d exchange time %0.8f ms\n", world_rank, world_size, r.total_time / n_iter * 1000);
      std::printf("%d/%d [%d:0x%08x] err_norm = %.8f\n", world_rank, world_size, b.device, b.info.vendor_id,
                  r.err_norm);
      std::fflush(stdout);
    }
    double time_sum = 0, err_sum = 0;
    MPI_Reduce(&r.total_time, &time_sum, 1, MPI_DOUBLE, MPI_SUM, 0, MPI_COMM_WORLD);
    MPI_Reduce(&r.err_norm, &err_sum, 1, MPI_DOUBLE, MPI_SUM, 0, MPI_COMM_WORLD);
    double med = r.iters.median(), mx = 0;
    MPI_Allreduce(&med, &mx, 1, MPI_DOUBLE, MPI_MAX, MPI_COMM_WORLD);
    // --overlap: whole steps of both orders, aggregated like the exchange time
    double step_sum[2] = {0, 0}, step_med[2] = {0, 0}, step_err = -1;
    if (overlap) {
      const double mine[2] = {r.step_serial.sum(), r.step_overlap.sum()};
      const double med2[2] = {r.step_serial.median(), r.step_overlap.median()};
      MPI_Reduce(mine, step_sum, 2, MPI_DOUBLE, MPI_SUM, 0, MPI_COMM_WORLD);
      MPI_Reduce(med2, step_med, 2, MPI_DOUBLE, MPI_MAX, 0, MPI_COMM_WORLD);
      MPI_Allreduce(&r.step_err_max, &step_err, 1, MPI_DOUBLE, MPI_MAX, MPI_COMM_WORLD);
      // one stale ghost cell moves an edge value by scale / 12 = n_global / 96
      if (step_err > static_cast<double>(n_global_deriv) / 192) halo_check_failed() = true;
    }
    if (world_rank == 0) {
      std::printf("TEST dim:%d, %s, buf:%d; %0.8f, err=%0.8f%s\n", dim,
                  space == GMT_SPACE_MANAGED ? "managed" : "device ", buf ? 1 : 0, time_sum,
                  err_sum, tags(space, true).c_str());
      if (overlap) {
        char err_field[48] = "";
        if (step_err >= 0) std::snprintf(err_field, sizeof(err_field), ", step_err=%0.8f", step_err);
        std::printf("STEP dim:%d, %s, buf:%d; serial=%0.8f, overlap=%0.8f%s [%s]\n", dim,
                    space == GMT_SPACE_MANAGED ? "managed" : "device ", buf ? 1 : 0, step_sum[0], step_sum[1],
                    err_field, r.transport.c_str());
      }
      JsonRecord j;
      j.add("app", "mpi_stencil2d_gt").add("test", name).add("dim", dim)
          .add("mem", space == GMT_SPACE_MANAGED ? "managed" : "device").add("buf", buf)
          .add("ranks", world_size).add("transport", r.transport).add("n_local_deriv", n_local_deriv)
          .add("n_other", n_global_other).add("iters", n_iter).add("time_sum_s", time_sum)
          .add("err_sum", err_sum).add("exchange_us_median_max_rank", mx * 1e6)
          .add("bytes_per_exchange", r.bytes_per_exchange)
          .add("GBps_per_rank", mx > 0 ? r.bytes_per_exchange / mx / 1e9 : 0.0)
          .add("buffers", alloc_per_call ? "per-call" : "persistent")
          .add("managed_host_resident", space == GMT_SPACE_MANAGED && host_resident_managed);
      if (overlap) {
        j.add("step_serial_us_median_max_rank", step_med[0] * 1e6)
            .add("step_overlap_us_median_max_rank", step_med[1] * 1e6)
            .add("step_err_max", step_err);
      }
      j.append_to(json);
    }
    std::fflush(stdout);
  };

  if (tests.find("deriv") != std::string::npos) {
    for (int dim = 0; dim < 2; ++dim) {
      if (only_dim >= 0 && dim != only_dim) continue;
      for (int m = 0; m < (managed ? 2 : 1); ++m) {
        if (only_mem == "managed" && m == 0) continue;
        for (int buf = 1; buf >= 0; --buf) {
          if (only_buf >= 0 && buf != only_buf) continue;
          DerivConfig c;
          c.dim = dim;
          c.n_local = n_local_deriv;
          c.n_other = n_global_other;
          c.n_iter = n_iter;
          c.n_warmup = n_warmup;
          c.space = m ? GMT_SPACE_MANAGED : GMT_SPACE_DEVICE;
          c.buf = buf;
          c.transport = want;
          c.host_init = cli.flag("host-init");
          c.host_verify = cli.flag("host-verify");
          c.check = cli.flag("check");
          c.overlap = overlap;
          c.realloc_per_call = alloc_per_call;
          DerivResult r = run_deriv(c, b, MPI_COMM_WORLD, pool);
          report("deriv", dim, c.space, buf, r);
        }
      }
    }
  }
  if (tests.find("sum") != std::string::npos) {
    for (int dim = 0; dim < 2; ++dim) {
      if (only_dim >= 0 && dim != only_dim) continue;
      for (int m = 0; m < (managed ? 2 : 1); ++m) {
        if (only_mem == "managed" && m == 0) continue;
        const int space = m ? GMT_SPACE_MANAGED : GMT_SPACE_DEVICE;
        SumResult r = run_sum(dim, space, n_local_deriv, n_global_other, n_iter, n_warmup, want,
                              b, pool);
        if (debug) {  // mpi_stencil2d_gt.cc:635-638
          std::printf("%d/%d allreduce time %0.8f ms\n", world_rank, world_size, r.total_time / n_iter * 1000);
          std::fflush(stdout);
        }
        double time_sum = 0, err = r.max_abs_err, err_max = 0;
        MPI_Reduce(&r.total_time, &time_sum, 1, MPI_DOUBLE, MPI_SUM, 0, MPI_COMM_WORLD);
        MPI_Reduce(&err, &err_max, 1, MPI_DOUBLE, MPI_MAX, 0, MPI_COMM_WORLD);
        if (world_rank == 0) {
          std::printf("TEST dim:%d, %s, buf:0; allreduce=%0.8f%s\n", dim,
                      m ? "managed" : "device ", time_sum, tags(space, false).c_str());
          if (err_max > 1e-9) std::printf("# WARNING allreduce value rel err %g\n", err_max);
          JsonRecord j;
          j.add("app", "mpi_stencil2d_gt").add("test", "sum").add("dim", dim)
              .add("mem", m ? "managed" : "device").add("ranks", world_size)
              .add("transport", r.transport).add("iters", n_iter).add("time_sum_s", time_sum)
              .add("allreduce_us_median", r.iters.median() * 1e6).add("value_rel_err", err_max);
          j.append_to(json);
        }
        std::fflush(stdout);
      }
    }
  }
  pool_owner.reset();
  MPI_Finalize();
  return halo_check_failed() ? 5 : EXIT_SUCCESS;
}
