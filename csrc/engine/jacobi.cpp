// Native distributed Jacobi engine (gmt/jacobi.hpp).
#include "gmt/jacobi.hpp"
#include "gmt/control.hpp"
#include "gmt/kernels.h"
#include "gmt/mg_tab.hpp"
#include "gmt/util.hpp"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

namespace gmt {

namespace {
// un = 1/4 ((W + E) + (S + N)) [+ s]: the source engines (JacobiConfig::source)
// store s itself and pass it as the kernels' f with c1 = 1 — o + 1.0 * s
// rounds the same with or without fma contraction; Laplace engines pass no f
constexpr double kC0 = 0.25;

int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }
}  // namespace

void choose_dims(int world, int64_t ny, int64_t nx, int* py, int* px) {
  double best = -1.0;
  for (int x = 1; x <= world; ++x) {
    if (world % x) continue;
    const int y = world / x;
    const double ly = static_cast<double>(ny) / y, lx = static_cast<double>(nx) / x;
    const double cost = (y > 1 ? 2 * lx : 0.0) + (x > 1 ? 1.5 * 2 * ly : 0.0);
    if (best < 0 || cost < best - 1e-9 || (std::fabs(cost - best) <= 1e-9 && y > *py)) {
      best = cost;
      *py = y;
      *px = x;
    }
  }
}

JacobiSolver::JacobiSolver(comm::Transport& t, const JacobiConfig& c) : t_(t), cfg_(c) {
  const int rank = t.rank(), world = t.size();
  watchdog_kick("jacobi: setup");
  if (c.py * c.px != world) {
    std::printf("JacobiSolver: process grid %dx%d != world size %d\n", c.py, c.px, world);
    abort_job(EXIT_FAILURE);
  }
  const int cy = rank / c.px, cx = rank % c.px;
  block_split(c.ny_global, c.py, cy, &oy_, &ny_);
  block_split(c.nx_global, c.px, cx, &ox_, &nx_);
  if (nx_ < 1 || ny_ < 1) {
    std::printf("JacobiSolver: empty local domain (%lldx%lld over %dx%d)\n",
                static_cast<long long>(c.ny_global), static_cast<long long>(c.nx_global), c.py, c.px);
    abort_job(EXIT_FAILURE);
  }
  auto at = [&](int y, int x) { return y * c.px + x; };
  const bool wx = c.periodic && (c.periodic_axes & 1), wy = c.periodic && (c.periodic_axes & 2);
  nb_.west = cx > 0 ? at(cy, cx - 1) : (wx ? at(cy, c.px - 1) : -1);
  nb_.east = cx < c.px - 1 ? at(cy, cx + 1) : (wx ? at(cy, 0) : -1);
  nb_.south = cy > 0 ? at(cy - 1, cx) : (wy ? at(c.py - 1, cx) : -1);
  nb_.north = cy < c.py - 1 ? at(cy + 1, cx) : (wy ? at(0, cx) : -1);
  // diagonal neighbours: the K-wide corner ghosts travel in the same single
  // exchange phase as the faces (gmt/halo.hpp one-phase corner mode);
  // GMT_HALO_TWO_PHASE=1 restores the two-phase exchange (A/B)
  auto wrap = [&](int v, int n, bool periodic, bool& ok) {
    if (v >= 0 && v < n) return v;
    if (!periodic) ok = false;
    return (v + n) % n;
  };
  auto diag = [&](int dy, int dx) {
    bool ok = true;
    const int y = wrap(cy + dy, c.py, wy, ok), x = wrap(cx + dx, c.px, wx, ok);
    return ok ? at(y, x) : -1;
  };
  const char* tp = std::getenv("GMT_HALO_TWO_PHASE");
  if (!(tp && tp[0] == '1')) {
    nb_.sw = diag(-1, -1);
    nb_.se = diag(-1, 1);
    nb_.nw = diag(1, -1);
    nb_.ne = diag(1, 1);
  }

  ks_ = c.tsteps > 1 ? c.tsteps : (c.tblock ? 2 : 1);
  if (ks_ > GMT_TB_MAX_SWEEPS) ks_ = GMT_TB_MAX_SWEEPS;
  while (ks_ > 1 && !gmt_jacobi5tb_supported(ks_)) --ks_;  // odd counts above 10: the next even one
  if (c.init != 0 && c.init != 1) {
    std::printf("JacobiSolver: init must be 0 (analytic) or 1 (random), got %d\n", c.init);
    abort_job(EXIT_FAILURE);
  }
  if (c.source < 0 || c.source > 3 || c.src_every < 0 || !(c.source_amp >= 0.0) || !std::isfinite(c.source_amp) ||
      (c.source != 0 && ks_ > 1 && c.src_every % ks_ != 0)) {
    std::printf("JacobiSolver: source must be 0..3, source_amp finite and >= 0, src_every 0 or a positive "
                "multiple of tsteps (%d); got %d, %g, %d\n", ks_, c.source, c.source_amp, c.src_every);
    abort_job(EXIT_FAILURE);
  }
  g_ = ks_;
  yo_ = g_;
  xo_ = round_up(g_, 8);  // ghost columns fit left of the interior; 64-B aligned interior
  // one row pitch on every rank (the largest share's): the inline halo
  // exchange addresses a neighbour's cells with this rank's pitch
  const int64_t nx_max = (c.nx_global + c.px - 1) / c.px;
  ld_ = round_up(xo_ + nx_max + g_, 64);
  const size_t elems = static_cast<size_t>(ld_) * (ny_ + 2 * g_);
  GMT_CHECK("stream", gmt_rt_stream_create(&s_, 0));
  // exchange stream priority: high by default; GMT_COMM_PRIORITY=0 for A/B
  const char* cp = std::getenv("GMT_COMM_PRIORITY");
  GMT_CHECK("comm stream", gmt_rt_stream_create(&cs_, cp && cp[0] == '0' ? 0 : 1));
  GMT_CHECK("event", gmt_rt_event_create(&ev_start_, 0));
  GMT_CHECK("event", gmt_rt_event_create(&ev_halo_, 0));

  // deterministic, decomposition-independent initial field and Dirichlet
  // ring: u(x, y) = x^3 + y^2 at global ghost-inclusive coordinates * h
  for (int b = 0; b < 2; ++b) buf_[b] = Buffer<double>(elems, GMT_SPACE_DEVICE);
  init_field();
  // Scaled levels (4^p u_p) are bitwise equal to the exact form while
  // max|u| * 4^K stays finite (and no level value is subnormal).  Every
  // Jacobi sweep averages, so the initial field's max|u| — measured here on
  // the device, max over ranks — bounds every later field.
  watchdog_kick("jacobi: max|u| all-reduce");
  umax_ = measure_max_abs();
  exact_ = c.exact == 1 || !(umax_ * std::ldexp(1.0, 2 * ks_) < 1e300);
  if (c.source != 0) {
    // the source and block fields, before capture_graphs: captured launches
    // hold these pointers.  A source breaks "the initial field bounds every
    // later one": a field grows by at most max|s| a sweep, and an int counts
    // fewer than 2^31 sweeps
    f_ = Buffer<double>(elems, GMT_SPACE_DEVICE);
    gsrc_ = Buffer<double>(elems, GMT_SPACE_DEVICE);
    fill_source();
    smax_ = measure_max_source();
    if (!source_bound_ok(smax_, ks_)) exact_ = true;
  }
  // exact passes stop at the largest K whose kernel fits the register file
  // (the ghost ring keeps its width: wider than a pass needs is harmless)
  if (ks_ > 1 && exact_)
    while (ks_ > gmt_jacobi5tb_max_sweeps(1) || !gmt_jacobi5tb_supported(ks_)) --ks_;
  // sweeps per source block (any count is correct: its passes are plan_passes')
  if (c.source != 0 && ks_ > 1) src_every_ = c.src_every > 0 ? c.src_every : ks_;
  resid_ws_ = Buffer<double>(gmt_jacobi_resid_workspace(nx_, ny_) + 1, GMT_SPACE_DEVICE);
  {
    const char* ce = std::getenv("GMT_CLOCK");
    if (!(ce && ce[0] == '0')) {
      clk_ = Buffer<uint64_t>(3, GMT_SPACE_DEVICE);
      clock_reset();
    }
  }
  // band-first passes: arrival counter, signal, waiter's count, error word
  sig_ = Buffer<uint64_t>(4, GMT_SPACE_FLAGS);
  for (int b = 0; b < 2; ++b) {
    Span2D<double> f(buf_[b].data() + (xo_ - g_), nx_ + 2 * g_, ny_ + 2 * g_, ld_);
    halo_[b] = std::make_unique<Halo2D>(t_, f, g_, g_, nb_, false, GMT_SPACE_DEVICE, ks_ > 1);
  }
  if (const char* e = std::getenv("GMT_PACK_WGS")) beside_pack_wgs_ = std::max(0, std::atoi(e));
  if (c.push && ks_ > 1 && halo_[0]->active()) setup_push();
  if (!push_on_ && ks_ > 1 && halo_[0]->active() && (c.overlap || c.overlap_auto)) split_cus();
  watchdog_kick("jacobi: halo plans ready");
  if (c.overlap_auto && !push_on_) autotune_overlap();
  if (c.source != 0) build_block_field();
  if (c.graph) capture_graphs();
  watchdog_kick("jacobi: ready");
}

// Band-first passes run the pass and the exchange on disjoint compute units.
// A fused pass keeps every CU's wave slots full (2 waves per SIMD, one round
// of resident workgroups on the shares), so exchange kernels on a stream of
// their own — pack, RCCL or staging copies, unpack, 256-thread workgroups —
// could only start as whole CUs drained, i.e. at the end of the pass
// (profiles/r03_shares.md).  GMT_COMM_CUS = 8, 16 or 24 CUs (the same
// number from every XCD) are reserved for the exchange while band-first
// passes run; serial passes keep every CU.  Off by default: measured slower
// on one GPU (profiles/r03_shares.md, "reserved CUs").
void JacobiSolver::split_cus() {
  int cus = 0;
  if (gmt_rt_device_cu_count(&cus) != 0 || cus < 16) return;
  const char* e = std::getenv("GMT_COMM_CUS");
  const int n = e ? std::atoi(e) : 0;
  if (n <= 0 || n > 24 || n % 8 || cus != 256) return;  // MI355X: 8 XCDs x 32 CUs
  const int words = (cus + 31) / 32;
  std::vector<uint32_t> comm(words, 0u), comp(words, 0u);
  // the same number of CUs from every XCD (8 of them, 32 CUs each), whether
  // the runtime numbers CUs XCD by XCD or round-robin over the XCDs: CU
  // 33 x + 8 y is on XCD x either way (x < 8, 8 y + 7 < 32)
  for (int i = 0; i < n; ++i) {
    const int cu = ((i % 8) * 33 + (i / 8) * 8) % cus;
    comm[cu / 32] |= 1u << (cu % 32);
  }
  for (int cu = 0; cu < cus; ++cu)
    if (!(comm[cu / 32] >> (cu % 32) & 1u)) comp[cu / 32] |= 1u << (cu % 32);
  gmt_stream_t cs = nullptr, sb = nullptr;
  if (gmt_rt_stream_create_cumask(&cs, words, comm.data()) != 0) return;
  if (gmt_rt_stream_create_cumask(&sb, words, comp.data()) != 0) {
    gmt_rt_stream_destroy(cs);
    return;
  }
  GMT_CHECK("sync", gmt_rt_stream_synchronize(cs_));
  gmt_rt_stream_destroy(cs_);
  cs_ = cs;
  sb_ = sb;
  comm_cus_ = n;
  GMT_CHECK("event", gmt_rt_event_create(&ev_band_, 0));
}

void JacobiSolver::init_field() {
  const JacobiConfig& c = cfg_;
  const double h = 1.0 / (static_cast<double>(c.ny_global > c.nx_global ? c.ny_global : c.nx_global) + 1);
  for (int b = 0; b < 2; ++b) {
    GMT_CHECK("memset", gmt_rt_memset_async(buf_[b].data(), 0, buf_[b].bytes(), s_));
    // global lattice index of the first ghost column / row: ox_ - g_, oy_ - g_
    if (c.init == 1)
      GMT_CHECK("fill", gmt_fill_poly(5, nx_ + 2 * g_, ny_ + 2 * g_, static_cast<double>(ox_ - g_),
                                      static_cast<double>(c.seed), static_cast<double>(oy_ - g_), 0.0,
                                      buf_[b].data() + (xo_ - g_), ld_, s_));
    else
      GMT_CHECK("fill", gmt_fill_poly(4, nx_ + 2 * g_, ny_ + 2 * g_, static_cast<double>(ox_ - g_), h,
                                      static_cast<double>(oy_ - g_), h, buf_[b].data() + (xo_ - g_), ld_, s_));
  }
  GMT_CHECK("init sync", gmt_rt_stream_synchronize(s_));
  parity_ = 0;
  passes_ = 0;
  advanced_ = false;
  fresh_[0] = fresh_[1] = false;  // periodic / neighbour ghosts come from an exchange
}

// ---- source term (cfg_.source) ----

void JacobiSolver::fill_source() {
  const JacobiConfig& c = cfg_;
  const double h = 1.0 / (static_cast<double>(c.ny_global > c.nx_global ? c.ny_global : c.nx_global) + 1);
  double* fi = f_.data() + xo_ + yo_ * ld_;
  GMT_CHECK("memset", gmt_rt_memset_async(f_.data(), 0, f_.bytes(), s_));
  // interior cell (i, j) is the global lattice point (ox_ + i, oy_ + j), as in init_field
  if (c.source == 1)
    GMT_CHECK("source fill", gmt_fill_poly(7, nx_, ny_, static_cast<double>(ox_), h, static_cast<double>(oy_), h, fi,
                                           ld_, s_));
  else if (c.source == 2)
    GMT_CHECK("source fill", gmt_fill_poly(6, nx_, ny_, static_cast<double>(ox_), static_cast<double>(c.seed + 1),
                                           static_cast<double>(oy_), c.source_amp, fi, ld_, s_));
  GMT_CHECK("source sync", gmt_rt_stream_synchronize(s_));
}

double JacobiSolver::measure_max_source() {
  Buffer<double> ws(static_cast<size_t>(gmt_diff_sq_workspace(nx_, ny_)) + 1, GMT_SPACE_DEVICE);
  GMT_CHECK("abs max", gmt_abs_max(nx_, ny_, f_.data() + xo_ + yo_ * ld_, ld_, ws.data(), ws.data() + 1, s_));
  t_.allreduce_max(ws.data(), 1, s_);
  double m = 0.0;
  GMT_CHECK("abs max D2H", gmt_rt_memcpy_async(&m, ws.data(), sizeof(double), s_));
  GMT_CHECK("abs max sync", gmt_rt_stream_synchronize(s_));
  return m;
}

bool JacobiSolver::source_bound_ok(double smax, int k) const {
  return (umax_ + std::ldexp(smax, 31)) * std::ldexp(1.0, 2 * k) < 1e300;
}

// g = src_every_ single source sweeps from a zero field with a zero ring,
// through the engine's own step (halo exchanges included: a neighbour's or a
// periodic ghost carries that side's g), then the initial field again.
void JacobiSolver::build_block_field() {
  const double t0 = wtime();
  src_setup_sweeps_ = 0;
  if (src_every_ > 0) {
    watchdog_kick("jacobi: source block field");
    if (smax_ == 0.0) {  // a zero source (kind 3 before set_source): a zero block field
      GMT_CHECK("memset", gmt_rt_memset_async(gsrc_.data(), 0, gsrc_.bytes(), s_));
    } else {
      for (int b = 0; b < 2; ++b) GMT_CHECK("memset", gmt_rt_memset_async(buf_[b].data(), 0, buf_[b].bytes(), s_));
      parity_ = 0;
      fresh_[0] = fresh_[1] = false;
      for (int i = 0; i < src_every_; ++i) {
        enqueue_step(parity_);
        parity_ ^= 1;
      }
      GMT_CHECK("block field", gmt_rt_memcpy_async(gsrc_.data(), buf_[parity_].data(), gsrc_.bytes(), s_));
      src_setup_sweeps_ = src_every_;
    }
    synchronize();
  }
  init_field();
  src_setup_ms_ = (wtime() - t0) * 1e3;
}

void JacobiSolver::add_block_field() {
  const int64_t off = xo_ + yo_ * ld_;
  GMT_CHECK("source add", gmt_add2d(nx_, ny_, gsrc_.data() + off, ld_, buf_[parity_].data() + off, ld_, s_));
  fresh_[parity_] = false;  // the ghost ring was not added to
}

int JacobiSolver::set_source(const double* host) {
  if (cfg_.source != 3 || !host) return 1;
  if (advanced_) return 2;
  double m = 0.0;
  for (int64_t i = 0; i < nx_ * ny_; ++i) m = std::max(m, std::isnan(host[i]) ? HUGE_VAL : std::fabs(host[i]));
  {  // max over ranks: one decision for every rank
    Buffer<double> d(1, GMT_SPACE_DEVICE);
    GMT_CHECK("source H2D", gmt_rt_memcpy(d.data(), &m, sizeof(double)));
    t_.allreduce_max(d.data(), 1, s_);
    GMT_CHECK("source D2H", gmt_rt_memcpy_async(&m, d.data(), sizeof(double), s_));
    GMT_CHECK("source sync", gmt_rt_stream_synchronize(s_));
  }
  if (ks_ > 1 && !exact_ && !source_bound_ok(m, ks_)) return 3;
  f_ring_ = 0;
  GMT_CHECK("source H2D", gmt_rt_memcpy2d_async(f_.data() + xo_ + yo_ * ld_, ld_ * sizeof(double), host,
                                                nx_ * sizeof(double), nx_ * sizeof(double), ny_, s_));
  GMT_CHECK("source sync", gmt_rt_stream_synchronize(s_));
  smax_ = m;
  build_block_field();
  return 0;
}

void JacobiSolver::source_plan(int k, int out[3]) const {
  out[0] = out[1] = out[2] = 0;
  if (cfg_.source == 0) return;
  out[1] = src_every_;
  if (k <= 0) return;
  out[0] = src_every_ > 0 ? k / src_every_ : 0;
  out[2] = src_every_ > 0 ? k % src_every_ : k;
}

double JacobiSolver::measure_max_abs() {
  const int64_t w = nx_ + 2 * g_, hgt = ny_ + 2 * g_;
  Buffer<double> ws(static_cast<size_t>(gmt_diff_sq_workspace(w, hgt)) + 1, GMT_SPACE_DEVICE);
  GMT_CHECK("abs max", gmt_abs_max(w, hgt, buf_[parity_].data() + (xo_ - g_), ld_, ws.data(), ws.data() + 1, s_));
  t_.allreduce_max(ws.data(), 1, s_);
  double m = 0.0;
  GMT_CHECK("abs max D2H", gmt_rt_memcpy_async(&m, ws.data(), sizeof(double), s_));
  GMT_CHECK("abs max sync", gmt_rt_stream_synchronize(s_));
  return m;
}

// One timed pass of every size the planner may use, on this rank's share
// with its real neighbours (a serial pass includes its exchange), max over
// ranks: the job's pass takes as long as its slowest rank.  The clock falls
// by about a quarter over the first few ms of sustained passes
// (profiles/r03_shares.md), so every pass type is launched once first (code
// object, occupancy query, clock settling), then the sizes are timed in two
// round-robin sweeps and each keeps its faster one: no size is measured only
// cold or only hot.
void JacobiSolver::calibrate_costs() {
  if (ks_ < 2) return;
  watchdog_kick("jacobi: pass-cost calibration");
  std::vector<int> ks;
  for (int K = 1; K <= ks_; ++K)
    if (K == 1 || (push_on_ ? gmt_jacobi5tb_push_supported(K) : gmt_jacobi5tb_supported(K))) ks.push_back(K);
  Buffer<double> d(ks.size(), GMT_SPACE_DEVICE);
  std::vector<double> host(ks.size(), 1e300);
  constexpr int kSweeps = 2;
  auto one = [&](int K) {
    if (K == 1) {
      step();
    } else {
      enqueue_block(parity_, K);
      parity_ ^= 1;
    }
  };
  for (int K : ks) one(K);
  synchronize();
  // enough passes per measurement for ~4 ms of GPU work: on small shares
  // (8192^2: 0.3 ms a pass) two passes were within the launch and sync
  // overhead of each other and the plan flipped between 18- and 20-sweep
  // passes from run to run (profiles/r04_shares.md)
  double t1 = wtime();
  one(ks_);
  synchronize();
  t1 = (wtime() - t1) * 1e3;
  {  // one pass count for every rank: the passes carry the exchanges
    GMT_CHECK("calib H2D", gmt_rt_memcpy(d.data(), &t1, sizeof(double)));
    t_.allreduce_max(d.data(), 1, s_);
    GMT_CHECK("calib D2H", gmt_rt_memcpy_async(&t1, d.data(), sizeof(double), s_));
    GMT_CHECK("calib sync", gmt_rt_stream_synchronize(s_));
  }
  const int kPasses = std::max(2, std::min(32, static_cast<int>(std::ceil(4.0 / std::max(t1, 1e-3)))));
  for (int sweep = 0; sweep < kSweeps; ++sweep)
    for (size_t i = 0; i < ks.size(); ++i) {
      const double t0 = wtime();
      for (int r = 0; r < kPasses; ++r) one(ks[i]);
      synchronize();
      host[i] = std::min(host[i], (wtime() - t0) / kPasses * 1e3);
    }
  GMT_CHECK("calib H2D", gmt_rt_memcpy(d.data(), host.data(), host.size() * sizeof(double)));
  t_.allreduce_max(d.data(), host.size(), s_);
  GMT_CHECK("calib D2H", gmt_rt_memcpy_async(host.data(), d.data(), host.size() * sizeof(double), s_));
  GMT_CHECK("calib sync", gmt_rt_stream_synchronize(s_));
  for (size_t i = 0; i < ks.size(); ++i) meas_ms_[ks[i]] = host[i];
  calibrated_ = true;
  // the built-in table was measured on one box for one kernel revision: say
  // so when this share disagrees with it by more than 10 %
  const double tab = table_pass_ms(ks_), got = meas_ms_[ks_];
  if (t_.rank() == 0 && tab > 0 && std::fabs(got - tab) > 0.1 * tab)
    std::fprintf(stderr, "# jacobi: measured %d-sweep pass %.3f ms vs the cost table's %.3f ms (%+.0f%%); "
                         "planning with the measured costs\n", ks_, got, tab, 100.0 * (got - tab) / tab);
  init_field();  // the timed passes advanced the solution: start over
}

void JacobiSolver::autotune_overlap() {
  if (ks_ < 2 || !halo_[0]->active()) return;  // nothing to hide
  watchdog_kick("jacobi: overlap autotune");
  Buffer<double> t(2, GMT_SPACE_DEVICE);
  double host[2] = {0.0, 0.0};
  constexpr int kPasses = 2;
  // first use of each mode's streams, untimed; then the modes in the order
  // A B B A, so the clock's fall over sustained passes (profiles/
  // r03_shares.md) does not favour the mode timed first
  for (int mode = 0; mode < 2; ++mode) {
    cfg_.overlap = mode == 0;
    enqueue_block(parity_, ks_);
    parity_ ^= 1;
  }
  synchronize();
  for (int mode : {0, 1, 1, 0}) {
    cfg_.overlap = mode == 0;
    const double t0 = wtime();
    for (int i = 0; i < kPasses; ++i) {
      enqueue_block(parity_, ks_);
      parity_ ^= 1;
    }
    synchronize();
    host[mode] += (wtime() - t0) / (2 * kPasses);
  }
  // one decision for every rank: the mode with the smaller summed time
  GMT_CHECK("tune H2D", gmt_rt_memcpy(t.data(), host, sizeof(host)));
  t_.allreduce_sum(t.data(), 2, s_);
  GMT_CHECK("tune D2H", gmt_rt_memcpy_async(host, t.data(), sizeof(host), s_));
  GMT_CHECK("tune sync", gmt_rt_stream_synchronize(s_));
  tune_s_[0] = host[0] / t_.size();
  tune_s_[1] = host[1] / t_.size();
  cfg_.overlap = host[0] <= host[1];
  init_field();  // the timed passes advanced the solution: start over
}

JacobiSolver::~JacobiSolver() {
  if (s_) gmt_rt_stream_synchronize(s_);
  for (void* b : push_opened_) GMT_WARN("ipc close", gmt_rt_ipc_close(b));
  if (cs_) gmt_rt_stream_synchronize(cs_);
  if (sb_) gmt_rt_stream_synchronize(sb_);
  for (auto& g : graph_) gmt_rt_graph_destroy(g);
  for (auto& g : graph2_) gmt_rt_graph_destroy(g);
  gmt_rt_event_destroy(ev_start_);
  gmt_rt_event_destroy(ev_halo_);
  if (ev_band_) gmt_rt_event_destroy(ev_band_);
  halo_[0].reset();
  halo_[1].reset();
  for (auto e : rn_ev_)
    if (e) gmt_rt_event_destroy(e);
  gmt_rt_stream_destroy(cs_);
  if (sb_) gmt_rt_stream_destroy(sb_);
  gmt_rt_stream_destroy(s_);
}

void JacobiSolver::sweep_full(int parity, double* resid) {
  const double* u = buf_[parity].data();
  double* un = buf_[parity ^ 1].data();
  GMT_CHECK("jacobi sweep", gmt_jacobi5(xo_, nx_, yo_, ny_, u, un, ld_, src_f(), src_ld(), kC0, src_c1(), resid, s_));
}

void JacobiSolver::enqueue_step(int parity) {
  Halo2D& h = *halo_[parity];
  fresh_[parity ^ 1] = false;
  if (!h.active()) {
    sweep_full(parity, nullptr);
    return;
  }
  if (!cfg_.overlap || nx_ < 6 || ny_ < 3) {
    h.start(s_);
    h.finish(s_);
    sweep_full(parity, nullptr);
    return;
  }
  const double* u = buf_[parity].data();
  double* un = buf_[parity ^ 1].data();
  // core: every cell whose 5-point stencil stays inside the interior; it
  // starts at an even column so the sweep keeps its 16-B vector path
  GMT_CHECK("event", gmt_rt_event_record(ev_start_, s_));
  GMT_CHECK("core sweep", gmt_jacobi5(xo_ + 2, nx_ - 4, yo_ + 1, ny_ - 2, u, un, ld_, src_f(), src_ld(),
                                      kC0, src_c1(), nullptr, s_));
  // halo on the high-priority stream, concurrent with the core sweep
  GMT_CHECK("wait", gmt_rt_stream_wait_event(cs_, ev_start_));
  h.start(cs_);
  h.finish(cs_);
  GMT_CHECK("event", gmt_rt_event_record(ev_halo_, cs_));
  GMT_CHECK("wait", gmt_rt_stream_wait_event(s_, ev_halo_));
  // boundary frame: first/last row, first/last two columns
  const int64_t y0 = yo_, y1 = yo_ + 1;
  const int64_t rects[16] = {xo_, nx_, y0,            1,       xo_,           nx_, yo_ + ny_ - 1, 1,
                             xo_, 2,   y1,            ny_ - 2, xo_ + nx_ - 2, 2,   y1,            ny_ - 2};
  GMT_CHECK("frame sweep", gmt_jacobi5_rects(4, rects, u, un, ld_, src_f(), src_ld(), kC0, src_c1(), s_));
}

int JacobiSolver::halo_mask() const {
  static_assert(GMT_MG_HALO_W == 1 && GMT_MG_HALO_E == 2 && GMT_MG_HALO_S == 4 && GMT_MG_HALO_N == 8,
                "the gmt_mg_* calls take this mask too");
  return (nb_.west >= 0 ? 1 : 0) | (nb_.east >= 0 ? 2 : 0) | (nb_.south >= 0 ? 4 : 0) |
         (nb_.north >= 0 ? 8 : 0);
}

void JacobiSolver::xk_launch(int K, int n, const int64_t* rects, int parity, int sig_rects, int sig_rows,
                             gmt_stream_t st, int sig_cols) {
  const double* u = buf_[parity].data();
  double* un = buf_[parity ^ 1].data();
  const int64_t dom[4] = {xo_, nx_, yo_, ny_};
  const int mask = halo_mask();
  unsigned* count = reinterpret_cast<unsigned*>(sig_.data());
  const bool sig = sig_rects > 0 || sig_rows > 0 || sig_cols != 0;
  gmt_tb_opts o{K,   cfg_.wg_waves, cfg_.seg_rows, exact_ ? 1 : 0, sig_rects, sig ? count : nullptr,
                sig ? sig_.data() + 1 : nullptr, sig_rows, st == sb_ && sb_ ? comm_cus_ : 0, sig_cols};
  o.clock = clk_.data();
  o.shared = cfg_.tb_shared;
  GMT_CHECK("jacobi tb", gmt_jacobi5tb(&o, n, rects, dom, mask, u, un, ld_, ny_ + 2 * g_, st ? st : s_));
}

// The bands of a band-first pass, all inside the one output rect (the
// interior): no band rects, no extra strips, segments or warm-ups.
// W/E halo sides: the rect's first / last strip group, every segment at
// full length, dispatched first; each of their workgroups signals when done
// (gmt_tb_opts.signal_cols) — with the pass's later rounds still to run.
// S/N halo sides: the other groups' segments next to those sides are row
// bands (gmt_tb_opts.signal_rows = g_: dispatched next, N ones walked
// bottom-up, each output wave signals once its first g_ rows are stored).
// (Round 3 took the W/E bands as separate rects with 3/4-length segments:
// 1.05-1.08x the serial pass on the N = 8 shares, profiles/r03_shares.md.)
// False when the domain is too small for the bands.
bool JacobiSolver::band_rects(int K, int64_t* rects, int* sig_cols, int* sig_rows) const {
  const int mask = halo_mask();
  const bool hw = mask & 1, he = mask & 2, hs = mask & 4, hn = mask & 8;
  const int64_t wb = std::max<int64_t>(gmt_jacobi5tb_group_cols(K, cfg_.wg_waves), g_);
  const int rb = (hs ? 1 : 0) + (hn ? 1 : 0);
  if (wb <= 0 || (rb > 0 && ny_ < rb * std::max<int64_t>(32, g_)) || ny_ < 64) return false;
  const int64_t r[4] = {xo_, nx_, yo_, ny_};
  std::copy(r, r + 4, rects);
  *sig_cols = (hw ? 1 : 0) | (he ? 2 : 0);
  *sig_rows = rb > 0 ? g_ : 0;
  return *sig_cols != 0 || rb > 0;
}

void JacobiSolver::exchange_now(int parity) {
  Halo2D& h = *halo_[parity];
  h.start(s_);
  h.finish(s_);
  fresh_[parity] = true;
}

// ks_ (or fewer) sweeps u(t) -> u(t+K) in one pass.
//   serial:     exchange the halo of u, then one fused launch;
//   overlap:    band-first — one launch whose boundary bands are dispatched
//               first and raise a completion signal; the comm stream waits
//               for it (gmt_signal_wait) and exchanges the halo of u(t+K)
//               while the interior workgroups still run.  The pass leaves
//               its output's halo current (fresh_), so the next pass starts
//               without an exchange.
// Every workgroup is one the serial pass would run too (plus short band
// segments): no frame pass, no redundant work (the core/frame scheme of
// round 1 cost 2-11 % per pass, profiles/r02_shares.md).
void JacobiSolver::enqueue_block(int parity, int K) {
  if (push_on_) {
    push_block(parity, K);
    return;
  }
  Halo2D& h = *halo_[parity];
  const int64_t dom[4] = {xo_, nx_, yo_, ny_};
  if (!h.active()) {
    maybe_corrupt(parity);
    xk_launch(K, 1, dom, parity, 0, 0);
    return;
  }
  if (!fresh_[parity]) exchange_now(parity);
  maybe_corrupt(parity);
  int64_t rects[4];
  int cols = 0, rows = 0;
  if (!cfg_.overlap || !band_rects(K, rects, &cols, &rows)) {
    xk_launch(K, 1, dom, parity, 0, 0);
    fresh_[parity ^ 1] = false;
    return;
  }
  // the comm stream forks before the launch (so it never waits for the whole
  // pass), and its wait kernel is enqueued after it
  band_ran_ = true;
  GMT_CHECK("event", gmt_rt_event_record(ev_start_, s_));
  GMT_CHECK("wait", gmt_rt_stream_wait_event(cs_, ev_start_));
  if (sb_) {  // the pass on the compute CUs, joined back into s_ below
    GMT_CHECK("wait", gmt_rt_stream_wait_event(sb_, ev_start_));
    xk_launch(K, 1, rects, parity, 0, rows, sb_, cols);
    GMT_CHECK("event", gmt_rt_event_record(ev_band_, sb_));
    GMT_CHECK("wait", gmt_rt_stream_wait_event(s_, ev_band_));
  } else {
    xk_launch(K, 1, rects, parity, 0, rows, nullptr, cols);
  }
  GMT_CHECK("signal wait", gmt_signal_wait(sig_.data() + 1, sig_.data() + 2,
                                           reinterpret_cast<unsigned*>(sig_.data() + 3), cs_));
  Halo2D& hn = *halo_[parity ^ 1];
  hn.set_pack_wgs(beside_pack_wgs_);  // beside the pass: few resident pack workgroups
  hn.start(cs_);
  hn.finish(cs_);
  hn.set_pack_wgs(0);
  GMT_CHECK("event", gmt_rt_event_record(ev_halo_, cs_));
  GMT_CHECK("wait", gmt_rt_stream_wait_event(s_, ev_halo_));
  fresh_[parity ^ 1] = true;
}

// ---- inline halo exchange (cfg_.push) ----
//
// Each fused pass stores its output's face cells a second time, straight
// into the ghost cells of the neighbours' next input buffer
// (gmt_tb_opts.push, csrc/kernels/jacobi5tb.hpp): the S / N faces (the
// first / last g_ rows of the interior), W / E faces (the first / last g_
// columns) and the g_ x g_ corners for the diagonal neighbours.  No pack,
// exchange or unpack launch: one hand-over launch after the pass
// (gmt_push_sync) tells every neighbour "my pass is done" and waits for
// theirs, so the next pass reads complete ghost cells and no rank writes a
// buffer its neighbour still reads (a neighbour pushes into this rank's
// buffer b^1 only during its pass p, which starts after this rank's pass
// p - 1 — the last reader of b^1 — handed over).  The round-4 traces showed
// why an exchange cannot hide beside a pass that holds every CU: its
// kernels only get registers as the pass drains (profiles/r04_overlap.md).
// Written by the pass itself, the faces cost a few store instructions per
// step of the boundary strips and segments.
namespace {
constexpr int kPushOpp[8] = {GMT_PUSH_N, GMT_PUSH_S, GMT_PUSH_E, GMT_PUSH_W,
                             GMT_PUSH_NE, GMT_PUSH_NW, GMT_PUSH_SE, GMT_PUSH_SW};
constexpr int kPushTag = 40000;  // + the direction, seen from the sender
struct PushWire {
  gmt_ipc_handle h[3];  // buf_[0], buf_[1], the flag slots
  uint64_t off[3];
  int64_t nx, ny, ld;
};
}  // namespace

void JacobiSolver::setup_push() {
  const JacobiConfig& c = cfg_;
  const int me = t_.rank();
  const int nbr[8] = {nb_.south, nb_.north, nb_.west, nb_.east, nb_.sw, nb_.se, nb_.nw, nb_.ne};
  // The kernel's rules (gmt_tb_opts.push) on the smallest share, so every
  // rank takes the same decision: an even face width, two segments clear of
  // each other's face, two strips (wider than any pass's strip output).
  const int64_t ny_min = c.ny_global / c.py, nx_min = c.nx_global / c.px;
  if ((g_ & 1) || g_ > 64 || ny_min < 2 * g_ + 2 || nx_min <= 256 || !gmt_jacobi5tb_push_supported(ks_)) return;
  bool remote = false;
  for (int d = 0; d < 8; ++d) remote = remote || (nbr[d] >= 0 && nbr[d] != me);
  comm::Control* ctl = t_.control();
  // no control plane for the mappings (rccl): the transport's exchange (the
  // same on every rank: one transport kind per job)
  if (remote && !ctl) return;
  push_flags_ = Buffer<uint64_t>(8, GMT_SPACE_FLAGS);
  GMT_CHECK("push flags", gmt_rt_memset_async(push_flags_.data(), 0, push_flags_.bytes(), s_));
  GMT_CHECK("push flags", gmt_rt_stream_synchronize(s_));
  push_err_ = Buffer<unsigned>(1, GMT_SPACE_PINNED);
  *push_err_.data() = 0;
  push_stop_ = Buffer<unsigned>(1, GMT_SPACE_DEVICE);
  GMT_CHECK("push stop", gmt_rt_memset_async(push_stop_.data(), 0, push_stop_.bytes(), s_));
  // the hand-over's epoch lives on the device (gmt_push_sync_dev): a captured
  // hand-over replays with the epoch of its pass, not of its capture
  push_ctl_ = Buffer<uint64_t>(2, GMT_SPACE_DEVICE);
  GMT_CHECK("push epoch", gmt_rt_memset_async(push_ctl_.data(), 0, push_ctl_.bytes(), s_));
  GMT_CHECK("push stop", gmt_rt_stream_synchronize(s_));
  PushWire mine;
  std::memset(&mine, 0, sizeof(mine));
  void* own[3] = {buf_[0].data(), buf_[1].data(), push_flags_.data()};
  if (remote)
    for (int i = 0; i < 3; ++i) {
      size_t off = 0;
      GMT_CHECK("ipc handle", gmt_rt_ipc_get_handle(&mine.h[i], &off, own[i]));
      mine.off[i] = off;
    }
  mine.nx = nx_;
  mine.ny = ny_;
  mine.ld = ld_;
  std::vector<PushWire> in(8);
  std::vector<comm::HostMsg> rs, ss;
  for (int d = 0; d < 8; ++d) {
    if (nbr[d] < 0 || nbr[d] == me) continue;
    rs.push_back({&in[d], sizeof(PushWire), nbr[d], kPushTag + kPushOpp[d]});
    ss.push_back({&mine, sizeof(PushWire), nbr[d], kPushTag + d});
  }
  if (!rs.empty()) ctl->exchange(rs, ss);
  std::map<std::string, void*> opened;  // a handle maps once per process
  auto open = [&](const gmt_ipc_handle& h, uint64_t off) -> char* {
    const std::string k(reinterpret_cast<const char*>(h.bytes), sizeof(h.bytes));
    auto it = opened.find(k);
    if (it == opened.end()) {
      void* base = nullptr;
      GMT_CHECK("ipc open", gmt_rt_ipc_open(&base, &h));
      push_opened_.push_back(base);
      it = opened.emplace(k, base).first;
    }
    return static_cast<char*>(it->second) + off;
  };
  for (int d = 0; d < 8; ++d) {
    if (nbr[d] < 0) continue;
    const bool self = nbr[d] == me;
    if (!self && in[d].ld != ld_) {
      std::printf("JacobiSolver: rank %d's row pitch %lld differs from rank %d's %lld\n", nbr[d],
                  static_cast<long long>(in[d].ld), me, static_cast<long long>(ld_));
      abort_job(EXIT_FAILURE);
    }
    const int64_t onx = self ? nx_ : in[d].nx, ony = self ? ny_ : in[d].ny;
    // this rank's face cell (x, y) -> the neighbour's ghost cell (x + tx, y + ty)
    const bool wside = d == GMT_PUSH_W || d == GMT_PUSH_SW || d == GMT_PUSH_NW;
    const bool eside = d == GMT_PUSH_E || d == GMT_PUSH_SE || d == GMT_PUSH_NE;
    const bool sside = d == GMT_PUSH_S || d == GMT_PUSH_SW || d == GMT_PUSH_SE;
    const bool nside = d == GMT_PUSH_N || d == GMT_PUSH_NW || d == GMT_PUSH_NE;
    const int64_t tx = wside ? onx : (eside ? -nx_ : 0);
    const int64_t ty = sside ? ony : (nside ? -ny_ : 0);
    for (int b = 0; b < 2; ++b) {
      // a pass reading buffer b writes b ^ 1: its faces go to the
      // neighbour's b ^ 1, the neighbour's input of the next pass
      const char* t = self ? reinterpret_cast<const char*>(buf_[b ^ 1].data()) : open(in[d].h[b ^ 1], in[d].off[b ^ 1]);
      push_base_[b][d] = reinterpret_cast<const double*>(
          reinterpret_cast<uintptr_t>(t) + static_cast<uintptr_t>((ty * ld_ + tx) * static_cast<int64_t>(sizeof(double))));
    }
    if (!self) {
      push_remote_[d] = reinterpret_cast<uint64_t*>(open(in[d].h[2], in[d].off[2])) + kPushOpp[d];
      push_mask_ |= 1 << d;
    }
  }
  push_on_ = true;
  cfg_.overlap = false;  // no band-first passes: the exchange is inline
}

void JacobiSolver::push_block(int parity, int K) {
  if (!fresh_[parity]) exchange_now(parity);
  maybe_corrupt(parity);
  push_pass(parity, K);
  if (push_mask_) {
    fault_point_exchange(t_.rank());  // GMT_INJECT_HANG: the hand-over is this pass's exchange
    push_handover();
  }
  fresh_[parity ^ 1] = true;
}

// The stream work of one inline-halo block is a plain chain on the compute
// stream: push_pass, then push_handover.  Every argument of both is fixed per
// parity (the epoch is a device word), so capture_graphs records exactly
// these two launches and a replay is the block of whichever pass comes next.
void JacobiSolver::push_handover() {
  unsigned* arrivals = reinterpret_cast<unsigned*>(push_ctl_.data() + 1);
  GMT_CHECK("push hand-over", gmt_push_sync_dev(push_flags_.data(), push_remote_, push_mask_, push_ctl_.data(),
                                                arrivals, push_err_.data(), push_stop_.data(), s_));
}

void JacobiSolver::push_pass(int parity, int K) {
  const int64_t dom[4] = {xo_, nx_, yo_, ny_};
  gmt_tb_opts o{};
  o.sweeps = K;
  o.wg_waves = cfg_.wg_waves;
  o.exact = exact_ ? 1 : 0;
  for (int d = 0; d < 8; ++d) o.push[d] = push_base_[parity][d];
  o.push_w = g_;
  o.stop = push_stop_.data();
  o.clock = clk_.data();
  o.shared = cfg_.tb_shared;
  GMT_CHECK("jacobi tb (inline halo)", gmt_jacobi5tb(&o, 1, dom, dom, halo_mask(), buf_[parity].data(),
                                                     buf_[parity ^ 1].data(), ld_, ny_ + 2 * g_, s_));
}

int JacobiSolver::tb_launch_info(int K, int64_t out[6]) const {
  const int64_t dom[4] = {xo_, nx_, yo_, ny_};
  gmt_tb_opts o{};
  o.sweeps = K;
  o.wg_waves = cfg_.wg_waves;
  o.seg_rows = cfg_.seg_rows;
  o.exact = exact_ ? 1 : 0;
  if (push_on_) {
    for (int d = 0; d < 8; ++d) o.push[d] = push_base_[parity_][d];
    o.push_w = g_;
  }
  o.shared = cfg_.tb_shared;
  return gmt_jacobi5tb_plan(&o, 1, dom, dom, halo_mask(), ld_, ny_ + 2 * g_, out);
}

int JacobiSolver::tb_shared_strips(int K) const {
  const int64_t dom[4] = {xo_, nx_, yo_, ny_};
  gmt_tb_opts o{};
  o.sweeps = K;
  o.wg_waves = cfg_.wg_waves;
  o.seg_rows = cfg_.seg_rows;
  o.push_w = push_on_ ? g_ : 0;
  o.shared = cfg_.tb_shared;
  return gmt_jacobi5tb_shared_path(&o, 1, dom, halo_mask());
}

bool JacobiSolver::band_mode(int K) const {
  int64_t rects[4];
  int cols = 0, rows = 0;
  return cfg_.overlap && halo_[0] && halo_[0]->active() && band_rects(K, rects, &cols, &rows);
}

void JacobiSolver::step_block() {
  if (graph2_[parity_] && push_on_) {
    // an inline-halo graph is the pass and its hand-over, captured from a
    // current halo; the per-pass host hooks of the eager path run here, so
    // GMT_CORRUPT_PASS and GMT_INJECT_HANG keep counting passes
    if (!fresh_[parity_]) exchange_now(parity_);
    maybe_corrupt(parity_);
    if (push_mask_) fault_point_exchange(t_.rank());
    GMT_CHECK("graph launch", gmt_rt_graph_launch(graph2_[parity_], s_));
    fresh_[parity_ ^ 1] = true;
  } else if (graph2_[parity_]) {
    // a band-first graph starts from a current halo (it was captured so)
    const bool band = band_mode(ks_);
    if (band && !fresh_[parity_]) exchange_now(parity_);
    band_ran_ = band_ran_ || band;
    GMT_CHECK("graph launch", gmt_rt_graph_launch(graph2_[parity_], s_));
    fresh_[parity_ ^ 1] = band;
  } else {
    enqueue_block(parity_, ks_);
  }
  parity_ ^= 1;  // u(t+ks) lives in the other buffer
}

// Measured cost of one fused pass of K sweeps (ms; gmt_kernel_bench
// --only=tb --sustained=1: back-to-back launches with the default launch
// shape and segment plan, Dirichlet sides, MI355X, profiles/r02_tb4c.md, the
// 4-column kernel) on two domain sizes.  One-wave strips (K <= 8) run at
// ~3.7-4.1 ms at 32768^2 (K = 9, 10 sit at 253-255 VGPRs); two-stage strips
// (K >= 12) are VALU bound from K ~ 16 (K = 22, 24 would exceed the register
// file at 2 waves per SIMD and spill: not built).  0 = no kernel for that K
// (odd K > 10).
namespace {
struct PassCosts {
  double points;  // lattice points of the measured domain
  double ms[GMT_TB_MAX_SWEEPS + 1];
};
constexpr PassCosts kCostLarge = {32768.0 * 32768.0,
                                  {0,    3.98, 4.13, 3.79, 3.86, 3.85, 3.68, 3.85, 3.91, 4.58, 4.57, 0,    3.63,
                                   0,    3.76, 0,    3.89, 0,    4.30, 0,    4.68}};
constexpr PassCosts kCostSmall = {8192.0 * 8192.0,
                                  {0,     0.311, 0.300, 0.294, 0.292, 0.292, 0.302, 0.287, 0.289,
                                   0.317, 0.322, 0,     0.264, 0,     0.284, 0,     0.289, 0,
                                   0.319, 0,     0.349}};
constexpr double kLaunchMs = 0.015;    // host launch + dispatch per pass
constexpr double kExchangeMs = 0.035;  // a halo exchange not hidden by the overlap
}  // namespace

double JacobiSolver::table_pass_ms(int K) const {
  if (K < 1 || K > GMT_TB_MAX_SWEEPS) return 0.0;
  // The table measured on the closer domain size, scaled to the LARGEST
  // share of the job (ceil of the global extents over the grid): every rank
  // must compute the same plan — ranks whose shares differ by a row would
  // otherwise pick different pass sequences and exchange at different sweeps
  // — and the job's pass takes as long as its largest share.
  const JacobiConfig& c = cfg_;
  const double pts = static_cast<double>((c.nx_global + c.px - 1) / c.px) *
                     static_cast<double>((c.ny_global + c.py - 1) / c.py);
  const PassCosts& tab = std::fabs(std::log(pts / kCostLarge.points)) < std::fabs(std::log(pts / kCostSmall.points))
                             ? kCostLarge
                             : kCostSmall;
  if (tab.ms[K] <= 0 || (push_on_ && K > 1 && !gmt_jacobi5tb_push_supported(K))) return 0.0;
  const bool exchanges = t_.size() > 1 || c.periodic;  // the same on every rank
  // a push pass exchanges inline (its face stores are in the table's
  // measured push costs, its hand-over is a launch): no serial exchange
  const double over = kLaunchMs + (exchanges && !c.overlap && !push_on_ ? kExchangeMs : 0.0);
  return tab.ms[K] * pts / tab.points + over;
}

std::vector<int> JacobiSolver::plan_passes(int k) const {
  if (k <= 0) return {};
  if (ks_ <= 1) return std::vector<int>(k, 1);
  // pass costs: measured on this share (prepare with calibrate; launches and
  // serial exchanges included; max over ranks), else the built-in table for
  // the job's largest share — the same costs, hence the same plan, on every rank
  std::vector<double> cost(ks_ + 1, 0.0);
  for (int K = 1; K <= ks_; ++K) cost[K] = calibrated_ ? meas_ms_[K] : table_pass_ms(K);
  return plan_pass_sequence(k, ks_, cost, calibrated_);
}

std::vector<int> plan_pass_sequence(int k, int ks, std::vector<double> cost, bool measured) {
  std::vector<int> plan;
  if (k <= 0) return plan;
  if (ks <= 1 || static_cast<int>(cost.size()) <= ks) return std::vector<int>(k, 1);
  const int ks_ = ks;
  // measured costs carry ~1-2% of clock noise: a pass shorter than ks must
  // win by more than that to displace full passes (a 1000-sweep 8192^2 plan
  // flipped between 50x20 and 5x20+50x18, the latter 1.5% slower:
  // profiles/r05_final/bench_2.json)
  if (measured)
    for (int K = 2; K < ks_; ++K) cost[K] *= 1.02;
  std::vector<double> best(k + 1, 1e300);
  std::vector<int> pick(k + 1, 0);
  best[0] = 0.0;
  for (int s = 1; s <= k; ++s)
    for (int K = 1; K <= ks_ && K <= s; ++K) {
      if (cost[K] <= 0) continue;
      const double c = best[s - K] + cost[K];
      if (c < best[s]) {
        best[s] = c;
        pick[s] = K;
      }
    }
  for (int s = k; s > 0; s -= pick[s]) plan.push_back(pick[s]);
  // full ks_ passes first (graph replays), then the rest, largest first
  std::sort(plan.begin(), plan.end(), [&](int a, int b) {
    return (a == ks_) != (b == ks_) ? a == ks_ : a > b;
  });
  return plan;
}

void JacobiSolver::run(int k) {
  in_run_ = true;
  if (k > 0) advanced_ = true;
  if (src_every_ > 0) {
    // a source engine with fused passes: blocks of src_every_ sweeps — the
    // Laplace passes as they are (graphs and inline halo included), then
    // the block field added — and single source sweeps for the rest
    for (int b = 0; b < k / src_every_; ++b) {
      run_laplace(src_every_);
      add_block_field();
    }
    for (int i = 0; i < k % src_every_; ++i) step();
  } else {
    run_laplace(k);  // single sweeps carry their source themselves
  }
  in_run_ = false;
  watchdog_kick("jacobi steps enqueued");
}

void JacobiSolver::run_laplace(int k) {
  for (int K : plan_passes(k)) {
    if (K == 1) {
      step();
    } else if (K == ks_) {
      step_block();
    } else {
      enqueue_block(parity_, K);  // eager; the ks-wide halo covers it
      parity_ ^= 1;
    }
  }
}

void JacobiSolver::prepare(int k) {
  if (cfg_.calibrate && !calibrated_) calibrate_costs();
  std::vector<int> kinds;
  // a source engine's run(k): the passes of a block, the add, the single source sweep
  for (int K : plan_passes(src_every_ > 0 ? src_every_ : k))
    if (std::find(kinds.begin(), kinds.end(), K) == kinds.end()) kinds.push_back(K);
  if (src_every_ > 0 && std::find(kinds.begin(), kinds.end(), 1) == kinds.end()) kinds.push_back(1);
  for (int K : kinds) {
    if (K == 1) {
      enqueue_step(parity_);
    } else {
      enqueue_block(parity_, K);
    }
    parity_ ^= 1;
  }
  if (src_every_ > 0) add_block_field();
  synchronize();
  init_field();
}

void JacobiSolver::capture_graphs() {
  if (gmt_rt_backend() == GMT_BACKEND_HOST) return;  // no graphs on the CPU backend
  for (int b = 0; b < 2; ++b)
    if (halo_[b]->active() && !halo_[b]->capturable()) {
      std::printf("# jacobi: transport %s is not stream-ordered; running without hipGraphs\n",
                  t_.name());
      return;
    }
  // the first send/recv to each peer sets up connections: do that eagerly
  for (int b = 0; b < 2; ++b) {
    halo_[b]->start(cs_);
    halo_[b]->finish(cs_);
  }
  GMT_CHECK("sync", gmt_rt_stream_synchronize(cs_));
  const bool saved[2] = {fresh_[0], fresh_[1]};
  for (int p = 0; p < 4; ++p) {
    if (p >= 2 && ks_ < 2) break;  // no fused passes
    // serial passes capture their exchange; band-first and inline-halo ones
    // start from a current halo (step_block makes sure of it)
    fresh_[0] = fresh_[1] = p >= 2 && band_mode(ks_);
    int e = gmt_rt_stream_begin_capture(s_);
    if (e == 0) {
      if (p < 2) {
        enqueue_step(p);
      } else if (push_on_) {
        // the pass and its hand-over, a chain on s_ with no side stream; the
        // hand-over reads its epoch from device memory (gmt_push_sync_dev),
        // so the recorded launch is right for every later pass.  One rank
        // that is its own neighbour everywhere has no hand-over: the pass alone.
        // (the host hooks of push_block are step_block's on the replay path)
        push_pass(p - 2, ks_);
        if (push_mask_) push_handover();
      } else {
        enqueue_block(p - 2, ks_);
      }
      e = gmt_rt_stream_end_capture(s_, p < 2 ? &graph_[p] : &graph2_[p - 2]);
    }
    fresh_[0] = saved[0];
    fresh_[1] = saved[1];
    if (e != 0) {
      std::printf("# jacobi: hipGraph capture unavailable (%s); running eagerly\n",
                  gmt_rt_error_string(e));
      for (auto* arr : {graph_, graph2_})
        for (int i = 0; i < 2; ++i) {
          gmt_rt_graph_destroy(arr[i]);
          arr[i] = nullptr;
        }
      return;
    }
  }
}

void JacobiSolver::step() {
  if (graph_[parity_])
    GMT_CHECK("graph launch", gmt_rt_graph_launch(graph_[parity_], s_));
  else
    enqueue_step(parity_);
  fresh_[parity_ ^ 1] = false;
  parity_ ^= 1;
  advanced_ = true;
}

void JacobiSolver::synchronize() {
  GMT_CHECK("sync", gmt_rt_stream_synchronize(s_));
  // band-first passes fork to the side streams and join back into s_ (and
  // graph replays of them run on s_), so s_ covers them; the side streams
  // are synchronised and the band signal's error word read only after an
  // eager band-first pass (serial passes use neither)
  if (band_ran_) {
    GMT_CHECK("sync", gmt_rt_stream_synchronize(cs_));
    if (sb_) GMT_CHECK("sync", gmt_rt_stream_synchronize(sb_));
    uint64_t err = 0;
    GMT_CHECK("signal D2H", gmt_rt_memcpy(&err, sig_.data() + 3, sizeof(err)));
    if (err != 0) {
      std::printf("JacobiSolver: a band-first pass timed out waiting for its boundary bands (error %llu)\n",
                  static_cast<unsigned long long>(err));
      abort_job(EXIT_FAILURE);
    }
    band_ran_ = false;
  }
  if (push_on_ && push_mask_ && *push_err_.data() != 0) {
    std::printf("JacobiSolver: an inline-halo hand-over timed out waiting for the neighbours in directions "
                "0x%x (GMT_WAIT_TIMEOUT_MS); ghost cells are stale\n", *push_err_.data());
    abort_job(EXIT_FAILURE);
  }
  // a halo exchange that timed out (IPC) left stale ghost cells: fail loudly
  for (auto& h : halo_)
    if (h) h->check();
  std::string why;
  if (!t_.ok(&why)) {
    std::printf("JacobiSolver: %s\n", why.c_str());
    abort_job(EXIT_FAILURE);
  }
  watchdog_kick("jacobi synchronize");
}

double JacobiSolver::residual() {
  if (!fresh_[parity_]) exchange_now(parity_);
  sweep_full(parity_, resid_ws_.data());
  fresh_[parity_ ^ 1] = false;
  t_.allreduce_sum(resid_ws_.data(), 1, s_);
  double r = 0.0;
  GMT_CHECK("resid D2H", gmt_rt_memcpy_async(&r, resid_ws_.data(), sizeof(double), s_));
  GMT_CHECK("resid sync", gmt_rt_stream_synchronize(s_));
  parity_ ^= 1;
  advanced_ = true;
  return std::sqrt(r);
}

// The read-only residual of the current field, all-reduced, left in rn_dev_:
// everything stream-ordered on s_, nothing waits.
void JacobiSolver::rn_setup() {
  if (rn_dev_.data()) return;
  rn_ws_ = Buffer<double>(static_cast<size_t>(gmt_jacobi5_resid_workspace(nx_, ny_)), GMT_SPACE_DEVICE);
  rn_dev_ = Buffer<double>(2, GMT_SPACE_DEVICE);
  rn_ring_ = Buffer<double>(2 * (kMaxLag + 1), GMT_SPACE_PINNED);
  for (auto& e : rn_ev_) GMT_CHECK("event", gmt_rt_event_create(&e, 0));
}

// The sum of pair[0], then a max over both values: whatever order a transport
// adds in, every rank then holds the same two doubles and takes the same
// decision.
void JacobiSolver::allreduce_sum_max(double* pair) {
  t_.allreduce_sum(pair, 1, s_);
  t_.allreduce_max(pair, 2, s_);
}

void JacobiSolver::enqueue_residual(bool ring_current) {
  rn_setup();
  if (!ring_current && !fresh_[parity_]) exchange_now(parity_);
  GMT_CHECK("jacobi residual", gmt_jacobi5_resid(xo_, nx_, yo_, ny_, buf_[parity_].data(), ld_, src_f(), src_ld(), kC0,
                                                 src_c1(), rn_dev_.data(), rn_ws_.data(), s_));
  allreduce_sum_max(rn_dev_.data());
}

void JacobiSolver::residual_norm(double out[2]) {
  enqueue_residual();
  GMT_CHECK("resid D2H", gmt_rt_memcpy_async(rn_ring_.data(), rn_dev_.data(), 2 * sizeof(double), s_));
  GMT_CHECK("resid sync", gmt_rt_stream_synchronize(s_));
  out[0] = std::sqrt(rn_ring_[0]);
  out[1] = rn_ring_[1];
}

// The 1-wide ring around the interior of a field in the engine's layout:
// faces only, the plus-shaped stencil reads no corner.
std::unique_ptr<Halo2D> JacobiSolver::faces_halo(double* field) {
  Neighbors nb = nb_;
  nb.sw = nb.se = nb.nw = nb.ne = -2;
  Span2D<double> f(field + (yo_ - 1) * ld_ + (xo_ - 1), nx_ + 2, ny_ + 2, ld_);
  return std::make_unique<Halo2D>(t_, f, 1, 1, nb, false, GMT_SPACE_DEVICE, false);
}

// ---- the lagged check loop of solve(), cg() and cheby() ----

// What the three share of their options, and the names their texts use.
struct JacobiSolver::CheckLoop {
  const char* method;    // "solve", "cg", "cheby"
  const char* cap_name;  // the option `cap` is
  const char* phase;     // the watchdog phase of a decided check
  double tol, rtol;
  int norm, cap, every, lag;
  bool need_tol;         // solve(): tol or rtol must be positive (the others then run exactly `cap` iterations)
  // extra_ok: the method's own options hold; extra_rule: how the message words them
  void validate(bool extra_ok = true, const char* extra_rule = "") const {
    const bool tol_ok = tol >= 0.0 && rtol >= 0.0 && std::isfinite(tol) && std::isfinite(rtol) &&
                        (!need_tol || tol > 0.0 || rtol > 0.0);
    if (every < 1 || cap < 1 || cap % every != 0 || lag < 0 || lag > kMaxLag || (norm != 0 && norm != 1) || !tol_ok ||
        !extra_ok)
      throw std::invalid_argument(std::string("JacobiSolver::") + method + ": " + cap_name +
                                  " must be a positive multiple of check_every >= 1, 0 <= lag <= 8, norm 0 or 1, " +
                                  (need_tol ? "and tol or rtol positive" : "tol and rtol finite and >= 0") + extra_rule);
  }
};

// check(i) enqueues check i (after i * every iterations) and names the device
// pair {sum, max} it leaves, all-reduced; the pair is copied into slot
// i % (lag + 1) of the page-locked ring and decided `lag` checks later, when
// the host waits for its event only.  advance() enqueues `every` iterations.
void JacobiSolver::run_checks(const CheckLoop& c, CheckResult& res, const std::function<void()>& advance,
                              const std::function<const double*(int)>& check) {
  const int slots = c.lag + 1, last = c.cap / c.every;   // checks 0..last
  const bool fixed = !(c.tol > 0.0) && !(c.rtol > 0.0);  // run exactly `cap` iterations
  int decided = 0;  // checks decided so far
  bool stop = false;
  // decide on check i (its event has been recorded): every rank reads the
  // same all-reduced pair, so every rank stops at the same check
  auto decide = [&](int i) {
    GMT_CHECK(c.phase, gmt_rt_event_synchronize(rn_ev_[i % slots]));
    watchdog_kick(c.phase);
    const double sum = rn_ring_[2 * (i % slots)], mx = rn_ring_[2 * (i % slots) + 1];
    const double r = c.norm == 0 ? std::sqrt(sum) : mx;
    res.residual_iters = i * c.every;
    res.residual = r;
    res.residual_max = mx;
    if (i == 0) res.r0 = r;
    if (!std::isfinite(sum) || !std::isfinite(mx)) {
      res.failed = 1;
      stop = true;
    } else if (!fixed && r <= std::max(c.tol, c.rtol * res.r0)) {
      res.converged = 1;
      stop = true;
    }
  };
  for (int i = 0; i <= last && !stop; ++i) {
    if (i > 0) {
      advance();
      res.iters += c.every;
    }
    const double* pair = check(i);
    GMT_CHECK("check D2H", gmt_rt_memcpy_async(rn_ring_.data() + 2 * (i % slots), pair, 2 * sizeof(double), s_));
    GMT_CHECK("event", gmt_rt_event_record(rn_ev_[i % slots], s_));
    res.checks = i + 1;
    if (i >= c.lag) decide(decided++);
  }
  // drain the outstanding checks in order (the cap, or a stop with lag > 0:
  // the later checks' iterations have run, an earlier check still decides)
  while (!stop && decided < res.checks) decide(decided++);
}

SolveResult JacobiSolver::solve(const SolveOpts& o) {
  const CheckLoop loop{"solve", "max_sweeps", "jacobi solve check", o.tol, o.rtol, o.norm, o.max_sweeps,
                       o.check_every == 0 ? ks_ : o.check_every, o.lag, true};
  loop.validate();
  SolveResult res;
  run_checks(loop, res, [&] { run(loop.every); },
             [&](int) {
               enqueue_residual();
               return rn_dev_.data();
             });
  synchronize();
  return res;
}

// ---- conjugate gradients (gmt/jacobi.hpp CgOpts) ----

void JacobiSolver::cg_setup() {
  if (cg_sc_.data()) return;
  watchdog_kick("jacobi: cg set-up");
  const size_t elems = static_cast<size_t>(ld_) * (ny_ + 2 * g_);
  Buffer<double>* fields[3] = {&cg_r_, &cg_p_, &cg_q_};
  for (auto* b : fields) {
    *b = Buffer<double>(elems, GMT_SPACE_DEVICE);
    GMT_CHECK("memset", gmt_rt_memset_async(b->data(), 0, b->bytes(), s_));
  }
  cg_ws_ = Buffer<double>(static_cast<size_t>(gmt_cg_workspace(nx_, ny_)), GMT_SPACE_DEVICE);
  cg_sc_ = Buffer<double>(6, GMT_SPACE_DEVICE);
  GMT_CHECK("memset", gmt_rt_memset_async(cg_sc_.data(), 0, cg_sc_.bytes(), s_));
  GMT_CHECK("cg set-up sync", gmt_rt_stream_synchronize(s_));
  cg_halo_ = faces_halo(cg_p_.data());
  rn_setup();
  watchdog_kick("jacobi: cg ready");
}

CgResult JacobiSolver::cg(const CgOpts& o) {
  const CheckLoop loop{"cg", "max_iters", "jacobi cg check", o.tol, o.rtol, o.norm, o.max_iters,
                       o.check_every == 0 ? 10 : o.check_every, o.lag, false};
  loop.validate();
  if (periodic())
    throw std::invalid_argument("JacobiSolver::cg: I - J is singular on a periodic axis");
  cg_setup();
  double* u = buf_[parity_].data();
  double* sc = cg_sc_.data();
  CgResult res;
  // iteration k reads rr from parity k & 1 and leaves rr' in the other slot
  auto iterate = [&](int k) {
    double* rr = sc + 2 * (k & 1);
    double* rn = sc + 2 * ((k & 1) ^ 1);
    double* pq = sc + 4;
    cg_halo_->enqueue(s_);
    GMT_CHECK("cg apply", gmt_cg_apply(0, xo_, nx_, yo_, ny_, cg_p_.data(), ld_, nullptr, 0, kC0, 0.0, cg_q_.data(),
                                       ld_, pq, cg_ws_.data(), s_));
    allreduce_sum_max(pq);
    GMT_CHECK("cg update", gmt_cg_update(xo_, nx_, yo_, ny_, rr, pq, cg_p_.data(), ld_, cg_q_.data(), ld_, u, ld_,
                                         cg_r_.data(), ld_, rn, cg_ws_.data(), s_));
    allreduce_sum_max(rn);
    GMT_CHECK("cg direction", gmt_cg_dir(xo_, nx_, yo_, ny_, rn, rr, cg_r_.data(), ld_, cg_p_.data(), ld_, s_));
  };
  int k = 0;
  run_checks(loop, res,
             [&] {
               for (int j = 0; j < loop.every; ++j) iterate(k++);
               watchdog_kick("jacobi cg iterations enqueued");
             },
             [&](int i) {
               if (i == 0) {
                 // r = b - A u = the residual d of the current field; p = r on the interior
                 if (!fresh_[parity_]) exchange_now(parity_);
                 GMT_CHECK("cg residual", gmt_cg_apply(1, xo_, nx_, yo_, ny_, u, ld_, src_f(), src_ld(), kC0, src_c1(),
                                                       cg_r_.data(), ld_, sc, cg_ws_.data(), s_));
                 allreduce_sum_max(sc);
                 const int64_t off = xo_ + yo_ * ld_;
                 const gmt_copy2d_desc d = {cg_r_.data() + off, cg_p_.data() + off, ld_, ld_, nx_, ny_};
                 GMT_CHECK("cg p = r", gmt_copy2d_batched(1, &d, sizeof(double), s_));
               }
               return sc + 2 * (k & 1);  // the recursive rr of iteration k
             });
  if (res.iters > 0) {
    fresh_[parity_] = false;  // the ghost ring was not updated
    advanced_ = true;
  }
  // the true residual of the final field beside the recursive one
  enqueue_residual();
  GMT_CHECK("resid D2H", gmt_rt_memcpy_async(rn_ring_.data(), rn_dev_.data(), 2 * sizeof(double), s_));
  synchronize();
  res.true_residual = std::sqrt(rn_ring_[0]);
  res.true_residual_max = rn_ring_[1];
  return res;
}

// ---- Chebyshev semi-iteration (gmt/jacobi.hpp ChebyOpts) ----

double cheby_rho(int64_t nx_global, int64_t ny_global) {
  const double pi = 3.14159265358979323846;
  return 0.5 * (std::cos(pi / static_cast<double>(nx_global + 1)) + std::cos(pi / static_cast<double>(ny_global + 1)));
}

double cheby_next_weight(double rho2, double w, int k) {
  // volatile: the product is rounded before the subtraction on any target
  volatile double t = k == 1 ? 0.5 * rho2 : 0.25 * rho2;
  if (k != 1) t = t * w;
  return 1.0 / (1.0 - t);
}

void JacobiSolver::cheby_setup() {
  if (cheby_halo_[0]) return;
  watchdog_kick("jacobi: cheby set-up");
  for (int b = 0; b < 2; ++b) cheby_halo_[b] = faces_halo(buf_[b].data());
  rn_setup();
  watchdog_kick("jacobi: cheby ready");
}

ChebyResult JacobiSolver::cheby(const ChebyOpts& o) {
  const CheckLoop loop{"cheby", "max_iters", "jacobi cheby check", o.tol, o.rtol, o.norm, o.max_iters,
                       o.check_every == 0 ? 10 : o.check_every, o.lag, false};
  loop.validate(o.rho == 0.0 || (std::isfinite(o.rho) && o.rho > 0.0 && o.rho < 1.0), ", rho 0 or in (0, 1)");
  if (periodic())
    throw std::invalid_argument("JacobiSolver::cheby: the spectral radius is 1 on a periodic axis");
  cheby_setup();
  ChebyResult res;
  res.rho = o.rho == 0.0 ? cheby_rho(cfg_.nx_global, cfg_.ny_global) : o.rho;
  const double rho2 = res.rho * res.rho;
  double w = 1.0;  // the weight of the last iteration
  bool ring = false;  // the current buffer's 1-wide faces hold the neighbours' current values
  auto exchange = [&] {
    if (ring || fresh_[parity_]) return;
    cheby_halo_[parity_]->enqueue(s_);
    ring = true;
  };
  // iteration k + 1 of this call (k = 0: the plain sweep, w_1 = 1)
  auto iterate = [&](int k) {
    exchange();
    if (k == 0) {
      sweep_full(parity_, nullptr);
    } else {
      w = cheby_next_weight(rho2, w, k);
      GMT_CHECK("cheby step", gmt_cheby_step(xo_, nx_, yo_, ny_, buf_[parity_].data(), ld_, src_f(), src_ld(), kC0,
                                             src_c1(), w, buf_[parity_ ^ 1].data(), ld_, s_));
    }
    fresh_[parity_ ^ 1] = false;
    parity_ ^= 1;
    ring = false;
  };
  int k = 0;
  run_checks(loop, res,
             [&] {
               for (int j = 0; j < loop.every; ++j) iterate(k++);
               advanced_ = true;
               watchdog_kick("jacobi cheby iterations enqueued");
             },
             [&](int) {
               exchange();
               enqueue_residual(true);
               return rn_dev_.data();
             });
  if (res.iters > 0) fresh_[0] = fresh_[1] = false;  // only the faces of one buffer were exchanged
  synchronize();
  return res;
}

// ---- geometric multigrid (gmt/jacobi.hpp MgOpts) ----

int mg_coarse_iters(double rho) {
  if (!(rho > 0.0)) return 1;
  const double sigma = (1.0 - std::sqrt(1.0 - rho * rho)) / rho;
  // volatile: every product is rounded before it is used, as in Python
  volatile double t = sigma, t2 = 0.0;
  int k = 1;
  for (;;) {
    t2 = t * t;
    if (2.0 * t / (1.0 + t2) <= 0.1 || k >= 1 << 20) return k;
    t = t * sigma;
    ++k;
  }
}

namespace {

// One level of a hierarchy: the global extents and the share boundaries of
// either axis (rank k of the axis owns cells b[k] .. b[k+1] - 1, 0-based).
struct MgShape {
  int64_t ny = 0, nx = 0;
  std::vector<int64_t> by, bx;
  // an even extent: no nested coarser level, the transfers to the next one go by tables
  bool tab() const { return ny % 2 == 0 || nx % 2 == 0; }
};

std::vector<int64_t> mg_bounds(int64_t n, int p) {
  std::vector<int64_t> b(static_cast<size_t>(p) + 1, n);
  for (int i = 0; i < p; ++i) {
    int64_t len = 0;
    block_split(n, p, i, &b[i], &len);
  }
  return b;
}

// One axis of a coarsen = any level: the coarse share boundaries by the anchor
// rule of gmt/mg_tab.hpp; false when a rank would own no coarse point, or,
// on a level with table-driven transfers, when a rank's tables fail their
// checks (tap count, tap halo, coarse ring) or a rank with a neighbour has
// fewer than kMgTapHalo cells to send.
bool mg_any_axis(int64_t n, int64_t m, const std::vector<int64_t>& b, bool tables, std::vector<int64_t>* cb) {
  const size_t p = b.size() - 1;
  cb->resize(p + 1);
  for (size_t k = 0; k <= p; ++k) (*cb)[k] = mg_coarse_bound(n, m, b[k]);
  for (size_t k = 0; k < p; ++k) {
    if ((*cb)[k + 1] <= (*cb)[k]) return false;
    if (!tables) continue;
    if (p > 1 && b[k + 1] - b[k] < kMgTapHalo) return false;
    MgAxisTab tab;
    if (mg_axis_tab_build(n, m, b[k], b[k + 1] - b[k], (*cb)[k], (*cb)[k + 1] - (*cb)[k], &tab) != 0) return false;
  }
  return true;
}

std::vector<MgShape> mg_hierarchy(int64_t ny, int64_t nx, int py, int px, int max_levels, int coarsen) {
  std::vector<MgShape> out(1);
  out[0].ny = ny, out[0].nx = nx;
  out[0].by = mg_bounds(ny, py), out[0].bx = mg_bounds(nx, px);
  // nested: a coarser level halves the share boundaries
  auto halve = [](std::vector<int64_t>& b) {
    for (auto& v : b) v /= 2;
    for (size_t i = 0; i + 1 < b.size(); ++i)
      if (b[i + 1] <= b[i]) return false;  // a rank without a coarse row / column
    return true;
  };
  while (max_levels == 0 || static_cast<int>(out.size()) < max_levels) {
    const MgShape& f = out.back();
    MgShape c;
    if (coarsen == 0) {
      if (f.tab()) break;
      c.by = f.by, c.bx = f.bx;
      if (!halve(c.by) || !halve(c.bx)) break;
      c.ny = (f.ny - 1) / 2, c.nx = (f.nx - 1) / 2;
    } else {
      c.ny = mg_coarse_extent(f.ny), c.nx = mg_coarse_extent(f.nx);
      if (c.ny < 1 || c.nx < 1) break;
      if (!mg_any_axis(f.ny, c.ny, f.by, f.tab(), &c.by) || !mg_any_axis(f.nx, c.nx, f.bx, f.tab(), &c.bx)) break;
    }
    out.push_back(std::move(c));
  }
  return out;
}

}  // namespace

std::vector<std::pair<int64_t, int64_t>> mg_level_table(int64_t ny, int64_t nx, int py, int px, int max_levels,
                                                        int coarsen) {
  std::vector<std::pair<int64_t, int64_t>> out;
  for (const MgShape& l : mg_hierarchy(ny, nx, py, px, max_levels, coarsen)) out.emplace_back(l.ny, l.nx);
  return out;
}

std::vector<std::pair<int64_t, int64_t>> mg_level_table(int64_t ny, int64_t nx, int py, int px, int max_levels) {
  return mg_level_table(ny, nx, py, px, max_levels, 0);
}

namespace {
// the depth of one level from the smallest shares of its axes (0: the axis has one rank)
int mg_fuse_depth(int fuse, int64_t min_ny, int64_t min_nx, bool fine, int ranks, int ghost) {
  int64_t d = fuse < 1 ? 1 : fuse;
  if (min_ny > 0) d = std::min(d, min_ny);
  if (min_nx > 0) d = std::min(d, min_nx);
  if (fine && ranks > 1) d = std::min<int64_t>(d, ghost);
  return static_cast<int>(std::max<int64_t>(d, 1));
}
int64_t mg_min_share(const std::vector<int64_t>& b) {
  if (b.size() <= 2) return 0;
  int64_t m = b[1] - b[0];
  for (size_t k = 1; k + 1 < b.size(); ++k) m = std::min(m, b[k + 1] - b[k]);
  return m;
}
// a restricting level runs gmt_mg_resid_restrict (min shares as above)
bool mg_resid_level(bool tab, int64_t min_ny, int64_t min_nx, bool fine, int ranks, int ghost) {
  if (tab) return false;
  if (ranks == 1) return true;
  if ((min_ny > 0 && min_ny < 2) || (min_nx > 0 && min_nx < 2)) return false;
  return !fine || ghost >= 2;
}
// a level runs gmt_mg_prolong_smooth with c sweeps or half-sweeps (the min shares of the next coarser level)
bool mg_prolong_level(bool tab, int nu2, int c, int64_t cmin_ny, int64_t cmin_nx, int ranks) {
  if (nu2 < 1 || tab) return false;
  if (ranks == 1) return true;
  const int64_t w = c / 2 + 1;
  return !((cmin_ny > 0 && cmin_ny < w) || (cmin_nx > 0 && cmin_nx < w));
}
// the sweeps or half-sweeps of the first chunk of a post-smoothing run
int mg_prolong_chunk(int nu2, int smoother, int depth) { return std::min(smoother == 1 ? 2 * nu2 : nu2, depth); }
}  // namespace

std::vector<int> mg_prolong_levels(int64_t ny, int64_t nx, int py, int px, int ghost, int fuse, int nu2, int smoother,
                                   int max_levels, int coarsen) {
  const auto shapes = mg_hierarchy(ny, nx, py, px, max_levels, coarsen);
  std::vector<int> out;
  for (size_t l = 0; l + 1 < shapes.size(); ++l) {
    const int d = mg_fuse_depth(fuse, mg_min_share(shapes[l].by), mg_min_share(shapes[l].bx), l == 0, py * px, ghost);
    out.push_back(mg_prolong_level(shapes[l].tab(), nu2,
                                   mg_prolong_chunk(nu2, smoother, d), mg_min_share(shapes[l + 1].by),
                                   mg_min_share(shapes[l + 1].bx), py * px));
  }
  return out;
}

std::vector<int> mg_resid_levels(int64_t ny, int64_t nx, int py, int px, int ghost, int max_levels, int coarsen) {
  const auto shapes = mg_hierarchy(ny, nx, py, px, max_levels, coarsen);
  std::vector<int> out;
  for (size_t l = 0; l + 1 < shapes.size(); ++l)
    out.push_back(mg_resid_level(shapes[l].tab(), mg_min_share(shapes[l].by), mg_min_share(shapes[l].bx), l == 0,
                                 py * px, ghost));
  return out;
}

std::vector<int> mg_fuse_depths(int64_t ny, int64_t nx, int py, int px, int fuse, int ghost, int max_levels,
                                int coarsen) {
  const auto shapes = mg_hierarchy(ny, nx, py, px, max_levels, coarsen);
  std::vector<int> out;
  for (size_t l = 0; l + 1 < shapes.size(); ++l)
    out.push_back(mg_fuse_depth(fuse, mg_min_share(shapes[l].by), mg_min_share(shapes[l].bx), l == 0, py * px, ghost));
  return out;
}

std::unique_ptr<Halo2D> JacobiSolver::ring_halo(double* field, int64_t xo, int64_t yo, int64_t nx, int64_t ny,
                                                int64_t ld, bool corners, int width) {
  Neighbors nb = nb_;
  if (!corners) nb.sw = nb.se = nb.nw = nb.ne = -2;
  Span2D<double> f(field + (yo - width) * ld + (xo - width), nx + 2 * width, ny + 2 * width, ld);
  return std::make_unique<Halo2D>(t_, f, width, width, nb, false, GMT_SPACE_DEVICE, corners);
}

// Every level the problem has under mgc_ (mg_hierarchy without a limit); a
// call with max_levels uses the first of them.  The hierarchy of fused calls
// (mgh_ >= 2) gives its coarse levels GMT_MG_MAX_FUSE ghost rows and columns.
void JacobiSolver::mg_setup() {
  std::vector<MgLevel>& mg = mg_[mgh_];
  const bool wide = mgh_ >= 2;
  if (!mg.empty()) return;
  watchdog_kick("jacobi: mg set-up");
  cheby_setup();
  const auto shapes = mg_hierarchy(cfg_.ny_global, cfg_.nx_global, cfg_.py, cfg_.px, 0, mgc_);
  const int cy = t_.rank() / cfg_.px, cx = t_.rank() % cfg_.px;
  mg.resize(shapes.size());
  auto zeroed = [&](size_t elems) {
    Buffer<double> b(elems, GMT_SPACE_DEVICE);
    GMT_CHECK("memset", gmt_rt_memset_async(b.data(), 0, b.bytes(), s_));
    return b;
  };
  for (size_t l = 0; l < mg.size(); ++l) {
    MgLevel& L = mg[l];
    L.ny_g = shapes[l].ny;
    L.nx_g = shapes[l].nx;
    L.min_ny = mg_min_share(shapes[l].by), L.min_nx = mg_min_share(shapes[l].bx);
    size_t elems = static_cast<size_t>(ld_) * (ny_ + 2 * g_);
    if (l == 0) {
      L.nx = nx_, L.ny = ny_, L.ox = ox_, L.oy = oy_;
      L.xo = xo_, L.yo = yo_, L.ld = ld_;
    } else {
      L.ox = shapes[l].bx[cx], L.nx = shapes[l].bx[cx + 1] - L.ox;
      L.oy = shapes[l].by[cy], L.ny = shapes[l].by[cy + 1] - L.oy;
      const int64_t gh = wide ? GMT_MG_MAX_FUSE : 1;
      L.xo = 8, L.yo = gh, L.ld = round_up(L.xo + L.nx + gh, 64);
      elems = static_cast<size_t>(L.ld) * (L.ny + 2 * gh);
      for (int b = 0; b < 2; ++b) {
        L.u[b] = zeroed(elems);
        L.up[b] = L.u[b].data();
      }
      L.s = zeroed(elems);
      L.sp = L.s.data();
    }
    L.dyo = L.yo, L.dld = L.ld;
    if (l + 1 == mg.size()) continue;
    L.tab = shapes[l].tab();
    if (L.tab) {  // room for the 2-wide ring of d, whatever the engine's ghost depth
      L.dyo = std::max<int64_t>(L.yo, kMgTapHalo);
      L.dld = std::max(L.ld, round_up(L.xo + L.nx + kMgTapHalo, 64));
      elems = static_cast<size_t>(L.dld) * (L.dyo + L.ny + kMgTapHalo);
    }
    L.delems = elems;  // d itself when a call first runs the level's residual unfused (mg_fuse_setup)
  }
  if (!mg_ws_.data())
    mg_ws_ = Buffer<double>(static_cast<size_t>(gmt_cg_workspace(nx_, ny_)) + 2, GMT_SPACE_DEVICE);
  GMT_CHECK("mg set-up sync", gmt_rt_stream_synchronize(s_));
  for (size_t l = 0; l < mg.size(); ++l) {
    MgLevel& L = mg[l];
    if (l > 0)
      for (int b = 0; b < 2; ++b) L.hu[b] = ring_halo(L.up[b], L.xo, L.yo, L.nx, L.ny, L.ld, true);
    if (!L.tab) continue;
    // the tables of this rank's share, checked on the host before they reach the device
    const MgLevel& C = mg[l + 1];
    const gmt_mg_xfer_desc desc{{L.nx_g, L.ny_g}, {C.nx_g, C.ny_g}, {L.ox, L.oy},
                                {L.nx, L.ny},     {C.ox, C.oy},     {C.nx, C.ny}};
    void* plan = nullptr;
    GMT_CHECK("mg transfer plan", gmt_mg_xfer_plan_create(&desc, &plan));
    L.plan.reset(plan);
  }
  watchdog_kick("jacobi: mg ready");
}

void JacobiSolver::mg_ring(int l) {
  MgLevel& L = mg_[mgh_][l];
  if (L.ring) return;
  (l == 0 ? *cheby_halo_[L.cur] : *L.hu[L.cur]).enqueue(s_);
  L.ring = true;
}

// The depth of every smoothing level of this call (mg_fuse_depths' rule on the
// shares mg_setup kept), whether a restricting level fuses its residual into
// the restriction (mg_resid_levels' rule) and, on first use, what the level
// needs: the wide halo plans of either buffer (at the level's depth, 2-wide
// for the fused transfer) and of the source (one cell narrower), or the
// residual field d and its ring's plan where the transfer runs unfused.  A
// level that interpolates inside its post-smoothing pass (mg_prolong_levels'
// rule) needs the next coarser level's plans c/2 + 1 wide.  Level 0's source
// ring is exchanged here, once per source.
void JacobiSolver::mg_fuse_setup(int levels, const MgOpts& o) {
  std::vector<MgLevel>& mg = mg_[mgh_];
  for (int l = 0; l < static_cast<int>(mg.size()); ++l) {
    MgLevel& L = mg[l];
    L.depth = l + 1 < levels ? mg_fuse_depth(o.fuse, L.min_ny, L.min_nx, l == 0, t_.size(), g_) : 1;
    L.resid = l + 1 < levels && o.fuse_resid != 0 &&
              mg_resid_level(L.tab, L.min_ny, L.min_nx, l == 0, t_.size(), g_);
    L.sw = std::max(L.depth >= 2 ? L.depth - 1 : 0, L.resid ? 1 : 0);
    L.pc = mg_prolong_chunk(o.nu2, o.smoother, L.depth);
    L.prolong = l + 1 < levels && o.fuse_prolong != 0 &&
                mg_prolong_level(L.tab, o.nu2, L.pc, mg[l + 1].min_ny, mg[l + 1].min_nx, t_.size());
    // the width at which the finer level reads this one's field when it interpolates
    const int ew = l > 0 && l < levels && mg[l - 1].prolong ? mg[l - 1].pc / 2 + 1 : 1;
    if (l + 1 < levels && !L.resid && !L.d.data()) {
      L.d = Buffer<double>(L.delems, GMT_SPACE_DEVICE);
      GMT_CHECK("memset", gmt_rt_memset_async(L.d.data(), 0, L.d.bytes(), s_));
      GMT_CHECK("mg set-up sync", gmt_rt_stream_synchronize(s_));
      L.hd = ring_halo(L.d.data(), L.xo, L.dyo, L.nx, L.ny, L.dld, true, L.tab ? kMgTapHalo : 1);
    }
    if (t_.size() == 1) continue;
    for (int b = 0; b < 2; ++b) {
      if (L.hk_field[b] != L.up[b])  // plans of a buffer that is gone
        for (auto& h : L.hk[b]) h.reset();
      L.hk_field[b] = L.up[b];
      for (const int w : {L.depth, L.resid ? 2 : 1, ew, L.prolong ? L.pc : 1})
        if (w >= 2 && !L.hk[b][w]) L.hk[b][w] = ring_halo(L.up[b], L.xo, L.yo, L.nx, L.ny, L.ld, true, w);
    }
    if (L.sw > 0 && L.sp && !L.hs[L.sw])
      L.hs[L.sw] = ring_halo(const_cast<double*>(L.sp), L.xo, L.yo, L.nx, L.ny, L.ld, true, L.sw);
  }
  MgLevel& F = mg[0];
  if (F.sw > 0 && F.sp && t_.size() > 1 && f_ring_ < F.sw) {
    F.hs[F.sw]->enqueue(s_);
    f_ring_ = F.sw;
  }
}

// n sweeps of the smoother on level l: chunks of min(n, depth); a chunk of two
// or more is one depth-wide exchange with corners and one gmt_mg_smooth_k.
// Red-black: 2n half-sweeps in the same chunks, through gmt_mg_smooth_rb.
void JacobiSolver::mg_smooth_run(int l, int n, const MgOpts& o, int done) {
  MgLevel& L = mg_[mgh_][l];
  const int64_t ldf = L.sp ? L.ld : 0;
  const double c1 = L.sp ? 1.0 : 0.0;
  const int mask = halo_mask();
  const bool rb = o.smoother == 1;
  // cell (xo, yo) has the 1-based global indices (ox + 1, oy + 1): red, due first, iff ox + oy is even
  int par = static_cast<int>((L.ox + L.oy) & 1);
  if (rb) n *= 2;
  n -= done;
  par ^= done & 1;
  while (n > 0) {
    const int c = std::min(n, L.depth);
    // a rank without neighbours reads its fixed ring only: its ring plan exchanges nothing
    if (c >= 2 && mask != 0)
      L.hk[L.cur][L.depth]->enqueue(s_);
    else
      mg_ring(l);
    if (rb) {
      GMT_CHECK("mg red-black smooth", gmt_mg_smooth_rb(c, par, L.xo, L.nx, L.yo, L.ny, mask, L.up[L.cur], L.ld, L.sp,
                                                        ldf, kC0, c1, o.omega, L.up[L.cur ^ 1], L.ld, s_));
      par ^= c & 1;
    } else if (c >= 2) {
      GMT_CHECK("mg fused smooth", gmt_mg_smooth_k(c, L.xo, L.nx, L.yo, L.ny, mask, L.up[L.cur], L.ld, L.sp, ldf, kC0,
                                                   c1, o.omega, L.up[L.cur ^ 1], L.ld, s_));
    } else {
      GMT_CHECK("mg smooth", gmt_mg_smooth(L.xo, L.nx, L.yo, L.ny, L.up[L.cur], L.ld, L.sp, ldf, kC0, c1, o.omega,
                                           L.up[L.cur ^ 1], L.ld, s_));
    }
    L.cur ^= 1;
    L.ring = false;
    n -= c;
  }
}

void JacobiSolver::mg_cycle(int l, int levels, const MgOpts& o, int coarse_iters, double coarse_rho) {
  MgLevel& L = mg_[mgh_][l];
  const int64_t ldf = L.sp ? L.ld : 0;
  const double c1 = L.sp ? 1.0 : 0.0;
  if (l == levels - 1) {
    // the Chebyshev iteration of cheby() from u = 0 (the caller zeroed it)
    const double rho2 = coarse_rho * coarse_rho;
    double w = 1.0;
    for (int k = 0; k < coarse_iters; ++k) {
      mg_ring(l);
      if (k == 0) {
        GMT_CHECK("mg coarse sweep", gmt_jacobi5(L.xo, L.nx, L.yo, L.ny, L.up[L.cur], L.up[L.cur ^ 1], L.ld, L.sp, ldf,
                                                 kC0, c1, nullptr, s_));
      } else {
        w = cheby_next_weight(rho2, w, k);
        GMT_CHECK("mg coarse step", gmt_cheby_step(L.xo, L.nx, L.yo, L.ny, L.up[L.cur], L.ld, L.sp, ldf, kC0, c1, w,
                                                   L.up[L.cur ^ 1], L.ld, s_));
      }
      L.cur ^= 1;
      L.ring = false;
    }
    return;
  }
  auto smooth = [&](int n) { mg_smooth_run(l, n, o); };
  MgLevel& C = mg_[mgh_][l + 1];
  const int px = L.ox % 2 == 0 ? 1 : 0, py = L.oy % 2 == 0 ? 1 : 0;
  const int mask = halo_mask();  // a rank without neighbours reads its fixed rings only
  smooth(o.nu1);
  if (L.resid) {
    // the residual on the ring of d comes from the neighbours' cells two deep
    if (mask != 0) {
      // a level that interpolates inside its post-smoothing pass reads this halo again, c deep: max(2, c) wide
      L.hk[L.cur][L.prolong && L.pc >= 2 ? L.pc : 2]->enqueue(s_);
      L.ring = true;
    }
    GMT_CHECK("mg fused residual and restrict",
              gmt_mg_resid_restrict(L.xo, L.nx, L.yo, L.ny, px, py, mask, L.up[L.cur], L.ld, L.sp, ldf, kC0, c1, kC0,
                                    C.s.data(), C.xo, C.yo, C.ld, s_));
  } else {
    mg_ring(l);
    // d in its own layout: row yo of u is row dyo of d
    double* dv = L.d.data() + (L.dyo - L.yo) * L.dld;
    GMT_CHECK("mg residual", gmt_cg_apply(1, L.xo, L.nx, L.yo, L.ny, L.up[L.cur], L.ld, L.sp, ldf, kC0, c1, dv, L.dld,
                                          mg_ws_.data(), mg_ws_.data() + 2, s_));
    L.hd->enqueue(s_);
    if (L.tab)
      GMT_CHECK("mg restrict", gmt_mg_restrict_tab(L.plan.get(), L.xo, L.dyo, L.d.data(), L.dld, C.s.data(), C.xo,
                                                   C.yo, C.ld, s_));
    else
      GMT_CHECK("mg restrict", gmt_mg_restrict(L.xo, L.nx, L.yo, L.ny, px, py, L.d.data(), L.ld, kC0, C.s.data(), C.xo,
                                               C.yo, C.ld, s_));
  }
  // a coarser level with fused smoothing or a fused transfer reads the ring of its source too
  if (C.sw > 0 && C.hs[C.sw]) C.hs[C.sw]->enqueue(s_);
  // u = 0 on the coarser level, ring included: current on every rank
  GMT_CHECK("memset", gmt_rt_memset_async(C.up[0], 0, C.u[0].bytes(), s_));
  C.cur = 0;
  C.ring = true;
  mg_cycle(l + 1, levels, o, coarse_iters, coarse_rho);
  if (L.prolong) {
    // u + P e inside the first chunk of the post-smoothing run: the halo cells of u are corrected here as
    // their owners would, from the coarser field c/2 + 1 beyond this rank's cells
    const int c = L.pc, cw = c / 2 + 1;
    if (mask != 0) {
      (cw >= 2 ? *C.hk[C.cur][cw] : *C.hu[C.cur]).enqueue(s_);  // either with corners
      C.ring = true;
      if (c >= 2 && !L.resid) L.hk[L.cur][c]->enqueue(s_);  // the fused residual left the halo this deep already
    }
    // c = 1: the faces are current since the residual.  Level 0's ring plan has no corners: the kernel corrects
    // the four corner cells of B0 from stale values, and one sweep's plus-shaped stencil never reads them
    if (c == 1) mg_ring(l);
    const bool rb = o.smoother == 1;
    GMT_CHECK("mg fused prolong and smooth",
              gmt_mg_prolong_smooth(c, rb ? 1 : 0, rb ? static_cast<int>((L.ox + L.oy) & 1) : 0, L.xo, L.nx, L.yo, L.ny,
                                    px, py, mask, C.up[C.cur], C.xo, C.yo, C.ld, L.up[L.cur], L.ld, L.sp, ldf, kC0, c1,
                                    o.omega, L.up[L.cur ^ 1], L.ld, s_));
    L.cur ^= 1;
    L.ring = false;
    mg_smooth_run(l, o.nu2, o, c);
    return;
  }
  C.hu[C.cur]->enqueue(s_);
  C.ring = true;
  if (L.tab)
    GMT_CHECK("mg prolong", gmt_mg_prolong_add_tab(L.plan.get(), L.xo, L.yo, C.up[C.cur], C.xo, C.yo, C.ld,
                                                   L.up[L.cur], L.ld, s_));
  else
    GMT_CHECK("mg prolong", gmt_mg_prolong_add(L.xo, L.nx, L.yo, L.ny, px, py, C.up[C.cur], C.xo, C.yo, C.ld,
                                               L.up[L.cur], L.ld, s_));
  L.ring = false;
  smooth(o.nu2);
}

MgResult JacobiSolver::mg(const MgOpts& o) {
  const CheckLoop loop{"mg", "max_cycles", "jacobi mg check", o.tol, o.rtol, o.norm, o.max_cycles,
                       o.check_every == 0 ? 1 : o.check_every, o.lag, false};
  loop.validate(o.nu1 >= 0 && o.nu2 >= 0 && o.nu1 + o.nu2 > 0 && o.omega > 0.0 && o.omega <= 1.0 &&
                    o.max_levels >= 0 && o.max_levels != 1 && o.coarse_iters >= 0 && (o.coarsen == 0 || o.coarsen == 1) &&
                    (o.fuse == 0 || (o.fuse >= 2 && o.fuse <= GMT_MG_MAX_FUSE)) &&
                    (o.smoother == 0 || o.smoother == 1) && (o.fuse_resid == 0 || o.fuse_resid == 1) &&
                    (o.fuse_prolong == 0 || o.fuse_prolong == 1),
                ", nu1 and nu2 >= 0 with nu1 + nu2 > 0, omega in (0, 1], max_levels 0 or >= 2, coarse_iters >= 0, "
                "coarsen 0 or 1, fuse 0 or 2..4, smoother 0 or 1, fuse_resid 0 or 1, fuse_prolong 0 or 1");
  if (periodic())
    throw std::invalid_argument("JacobiSolver::mg: I - J is singular on a periodic axis");
  const auto table = mg_level_table(cfg_.ny_global, cfg_.nx_global, cfg_.py, cfg_.px, o.max_levels, o.coarsen);
  if (table.size() < 2)
    throw std::invalid_argument(
        std::string("JacobiSolver::mg: no coarse level: ") +
        (o.coarsen == 0 && (cfg_.ny_global % 2 == 0 || cfg_.nx_global % 2 == 0)
             ? "nx + 1 and ny + 1 must be even"
             : o.coarsen == 0 ? "a rank of the process grid would own no coarse point"
                              : "the extents are too small or a rank of the process grid would own no coarse point"));
  mgc_ = o.coarsen;
  mgh_ = o.coarsen + (o.fuse > 0 || o.fuse_resid || o.fuse_prolong ? 2 : 0);
  mg_setup();
  const int levels = static_cast<int>(table.size());
  MgResult res;
  res.levels = levels;
  res.coarse_ny = table.back().first;
  res.coarse_nx = table.back().second;
  res.coarse_rho = cheby_rho(res.coarse_nx, res.coarse_ny);
  res.coarse_iters = o.coarse_iters > 0 ? o.coarse_iters : mg_coarse_iters(res.coarse_rho);
  MgLevel& F = mg_[mgh_][0];
  for (int b = 0; b < 2; ++b) F.up[b] = buf_[b].data();
  F.sp = src_f();
  mg_fuse_setup(levels, o);
  res.fuse = o.fuse;
  res.smoother = o.smoother;
  res.fuse_fine = F.depth;
  res.fuse_resid = o.fuse_resid;
  res.fuse_prolong = o.fuse_prolong;
  for (int l = 0; l + 1 < levels; ++l) {
    const MgLevel& L = mg_[mgh_][l];
    res.fuse_levels += L.depth >= 2;
    if (L.resid) ++res.resid_levels, res.resid_mask |= 1 << l;
    if (L.prolong) ++res.prolong_levels, res.prolong_mask |= 1 << l;
  }
  F.cur = parity_;
  F.ring = fresh_[parity_];
  run_checks(loop, res,
             [&] {
               for (int j = 0; j < loop.every; ++j) mg_cycle(0, levels, o, res.coarse_iters, res.coarse_rho);
               fresh_[0] = fresh_[1] = false;  // at most the faces of one buffer are current
               parity_ = F.cur;
               advanced_ = true;
               watchdog_kick("jacobi mg cycles enqueued");
             },
             [&](int) {
               mg_ring(0);
               enqueue_residual(true);
               return rn_dev_.data();
             });
  synchronize();
  return res;
}

void JacobiSolver::exchange_only() {
  Halo2D& h = *halo_[parity_];
  // the exchange packs the current field and writes its ghost ring: order it
  // after every pass already enqueued on the compute stream (on the compute
  // stream itself when the comm stream is held to a few CUs: this is the
  // blocking exchange bench.py times, and it has the GPU to itself)
  gmt_stream_t st = sb_ ? s_ : cs_;
  GMT_CHECK("event", gmt_rt_event_record(ev_start_, s_));
  GMT_CHECK("wait", gmt_rt_stream_wait_event(st, ev_start_));
  h.start(st);
  h.finish(st);
  GMT_CHECK("sync", gmt_rt_stream_synchronize(st));
  fresh_[parity_] = true;
}

// Fault injection for the check of the timed run: GMT_CORRUPT_PASS=R:P makes
// rank R, at the P-th fused pass that run() enqueued since the field was last
// initialised (bench.py: the warm-up's passes, then the timed ones), overwrite one ghost
// cell of the pass's input — after its exchange, or after the neighbour's
// inline push landed — with a wrong value, as a stale or corrupt pushed face
// cell would leave it.  The check (compare against single sweeps) must fire.
void JacobiSolver::maybe_corrupt(int parity) {
  if (!in_run_) return;  // calibration, prepare() and tuning passes do not count
  ++passes_;
  static const std::pair<int, int> spec = [] {
    const char* e = std::getenv("GMT_CORRUPT_PASS");
    int r = -1, p = -1;
    if (!e || std::sscanf(e, "%d:%d", &r, &p) != 2) r = p = -1;
    return std::make_pair(r, p);
  }();
  if (spec.first != t_.rank() || spec.second != passes_) return;
  // mid-face of the first side that has a neighbour (its ghost cells came
  // from that neighbour's exchange or push), else the west Dirichlet ring
  int64_t x = -1, y = ny_ / 2;
  if (nb_.west < 0 && nb_.east >= 0) {
    x = nx_;
  } else if (nb_.west < 0 && nb_.south >= 0) {
    x = nx_ / 2;
    y = -1;
  } else if (nb_.west < 0 && nb_.north >= 0) {
    x = nx_ / 2;
    y = ny_;
  }
  double* cell = buf_[parity].data() + (xo_ + x) + (yo_ + y) * ld_;
  GMT_CHECK("fault injection", gmt_fill_poly(3, 1, 1, 12345.0, 0.0, 0.0, 0.0, cell, ld_, s_));
  std::fprintf(stderr, "GMT FAULT INJECTION: rank %d corrupts ghost cell (x = %lld, y = %lld) of fused pass %d\n",
               t_.rank(), static_cast<long long>(x), static_cast<long long>(y), passes_);
}

void JacobiSolver::compare(JacobiSolver& o, double out[2]) {
  if (o.nx_ != nx_ || o.ny_ != ny_ || o.ox_ != ox_ || o.oy_ != oy_) {
    std::printf("JacobiSolver::compare: shares differ (%lldx%lld at %lld,%lld vs %lldx%lld at %lld,%lld)\n",
                static_cast<long long>(ny_), static_cast<long long>(nx_), static_cast<long long>(oy_),
                static_cast<long long>(ox_), static_cast<long long>(o.ny_), static_cast<long long>(o.nx_),
                static_cast<long long>(o.oy_), static_cast<long long>(o.ox_));
    abort_job(EXIT_FAILURE);
  }
  o.synchronize();
  Buffer<double> ws(2 * static_cast<size_t>(gmt_diff_sq_workspace(nx_, ny_)) + 2, GMT_SPACE_DEVICE);
  double* res = ws.data() + ws.size() - 2;
  GMT_CHECK("diff bits", gmt_diff_bits(nx_, ny_, buf_[parity_].data() + xo_ + yo_ * ld_, ld_,
                                       o.buf_[o.parity_].data() + o.xo_ + o.yo_ * o.ld_, o.ld_, res, ws.data(), s_));
  t_.allreduce_max(res, 1, s_);
  t_.allreduce_sum(res + 1, 1, s_);
  GMT_CHECK("diff bits D2H", gmt_rt_memcpy_async(out, res, 2 * sizeof(double), s_));
  GMT_CHECK("diff bits sync", gmt_rt_stream_synchronize(s_));
}

void JacobiSolver::clock_reset() {
  if (clk_.data()) GMT_CHECK("clock reset", gmt_rt_memset_async(clk_.data(), 0, clk_.bytes(), s_));
}

void JacobiSolver::clock_read(double out[3]) {
  out[0] = out[1] = out[2] = 0.0;
  if (!clk_.data()) return;
  uint64_t c[3] = {0, 0, 0};
  GMT_CHECK("clock D2H", gmt_rt_memcpy_async(c, clk_.data(), sizeof(c), s_));
  GMT_CHECK("clock sync", gmt_rt_stream_synchronize(s_));
  constexpr double kRealtimeMHz = 100.0;  // s_memrealtime: the CDNA constant 100 MHz clock
  out[0] = c[1] > 0 ? static_cast<double>(c[0]) / static_cast<double>(c[1]) * kRealtimeMHz : 0.0;
  out[1] = static_cast<double>(c[2]);
  out[2] = static_cast<double>(c[1]) / (kRealtimeMHz * 1e6);
}

void JacobiSolver::copy_interior(double* host) const {
  const double* src = buf_[parity_].data() + xo_ + yo_ * ld_;
  GMT_CHECK("interior D2H", gmt_rt_memcpy2d_async(host, nx_ * sizeof(double), src,
                                                  ld_ * sizeof(double), nx_ * sizeof(double), ny_, s_));
  GMT_CHECK("interior sync", gmt_rt_stream_synchronize(s_));
}

}  // namespace gmt
