// gmt/mg_tab.hpp — the per-axis tables of the table-driven multigrid transfers
// (gmt_mg_restrict_tab / gmt_mg_prolong_add_tab, gmt/kernels.h), host code
// only.  Both backends, the engine's level table and the apps' serial checks
// build their tables here, from integers, so every rank and every backend
// holds the same bits (engine.mg_axis_table is the Python definition).
//
// An axis has n fine and m coarse interior points on the same interval, rings
// at 0 and n + 1 (fine) and at 0 and m + 1 (coarse); all indices 1-based and
// global.  Fine point i lies between coarse points q and q + 1 with
//   q, r = divmod(i*(m+1), n+1),  t = r/(n+1)  (one fp64 division),
// and interpolates with the weights 1.0 - t and t.  Coarse point J gathers
// from the fine points with q(i) = J (weight 1.0 - t(i)) or with q(i) + 1 = J
// and r(i) != 0 (weight t(i)): the transpose, bit for bit.  Coarse point J is
// owned by the rank that owns fine cell floor(J*(n+1)/(m+1)).
#pragma once

#include <cstdint>
#include <vector>

namespace gmt {

// coarse points of an axis of n fine ones: (n-1)/2 for odd n (the nested
// rule, spacing 2), n/2 - 1 for even n
inline int64_t mg_coarse_extent(int64_t n) { return n % 2 == 1 ? (n - 1) / 2 : n / 2 - 1; }

inline void mg_axis_point(int64_t n, int64_t m, int64_t i, int64_t* q, int64_t* r, double* t) {
  const int64_t a = i * (m + 1);
  *q = a / (n + 1);
  *r = a % (n + 1);
  *t = static_cast<double>(*r) / static_cast<double>(n + 1);
}

// the taps of coarse point J: fine points first .. last, every i with
// (J-1)*(n+1) < i*(m+1) < (J+1)*(n+1)
inline void mg_axis_taps(int64_t n, int64_t m, int64_t J, int64_t* first, int64_t* last) {
  *first = (J - 1) * (n + 1) / (m + 1) + 1;
  *last = ((J + 1) * (n + 1) + m) / (m + 1) - 1;
}

// coarse points owned by the ranks that own fine cells 1 .. b: the J with
// floor(J*(n+1)/(m+1)) <= b.  b/2 on an odd axis.
inline int64_t mg_coarse_bound(int64_t n, int64_t m, int64_t b) {
  const int64_t c = ((b + 1) * (m + 1) - 1) / (n + 1);
  return c < m ? c : m;
}

constexpr int kMgMinTaps = 3;   // taps a coarse point has on an axis: the kernels read three
constexpr int kMgMaxTaps = 4;   // and a fourth where the count says so
constexpr int kMgTapHalo = 2;   // fine cells outside a region its coarse points may gather from
constexpr int kMgRingHalo = 1;  // coarse cells outside a region its fine points may interpolate from

// One axis of one region: fine cells fo+1 .. fo+fn, coarse cells co+1 .. co+cn
// (global, 1-based), every index below relative to the region's first cell.
struct MgAxisTab {
  std::vector<int32_t> pq;   // [fn] the coarse cell below fine cell i: -1 .. cn-1 (the other one is pq + 1)
  std::vector<double> pt;    // [fn] t
  std::vector<int32_t> rf;   // [2*cn] first tap (>= -kMgTapHalo), tap count (3 or 4)
  std::vector<double> rw;    // [4*cn] the taps' weights, 0 beyond the count
  int taps = 0;              // the largest tap count
  int lo = 0, hi = 0;        // fine cells tapped below / above the region
  int ring_lo = 0, ring_hi = 0;  // coarse cells read below / above the coarse region
};

// Fills tab; 0, or non-zero (tab then holds the needs found so far and must
// not reach a kernel): 1 a bad description, 2 a coarse point with fewer than
// kMgMinTaps or more than kMgMaxTaps taps, 3 a tap more than kMgTapHalo cells outside the region,
// 4 a coarse cell more than kMgRingHalo outside the coarse region.
inline int mg_axis_tab_build(int64_t n, int64_t m, int64_t fo, int64_t fn, int64_t co, int64_t cn, MgAxisTab* tab) {
  *tab = MgAxisTab();
  if (n < 1 || m < 1 || m > n || fo < 0 || fn < 0 || co < 0 || cn < 0 || fo + fn > n || co + cn > m ||
      n > (int64_t{1} << 31) - 8)
    return 1;
  tab->pq.resize(static_cast<size_t>(fn));
  tab->pt.resize(static_cast<size_t>(fn));
  tab->rf.resize(static_cast<size_t>(2 * cn));
  tab->rw.assign(static_cast<size_t>(4 * cn), 0.0);
  for (int64_t k = 0; k < fn; ++k) {
    int64_t q, r;
    mg_axis_point(n, m, fo + 1 + k, &q, &r, &tab->pt[k]);
    const int64_t rel = q - (co + 1);
    if (rel < -kMgRingHalo || rel + 1 > cn - 1 + kMgRingHalo) return 4;
    if (rel < 0) tab->ring_lo = 1;
    if (rel + 1 > cn - 1) tab->ring_hi = 1;
    tab->pq[k] = static_cast<int32_t>(rel);
  }
  for (int64_t k = 0; k < cn; ++k) {
    const int64_t J = co + 1 + k;
    int64_t first, last;
    mg_axis_taps(n, m, J, &first, &last);
    const int64_t cnt = last - first + 1;
    if (cnt > tab->taps) tab->taps = static_cast<int>(cnt);
    if (cnt < kMgMinTaps || cnt > kMgMaxTaps) return 2;
    const int64_t below = fo + 1 - first, above = last - (fo + fn);
    if (below > tab->lo) tab->lo = static_cast<int>(below < 1000 ? below : 1000);
    if (above > tab->hi) tab->hi = static_cast<int>(above < 1000 ? above : 1000);
    if (below > kMgTapHalo || above > kMgTapHalo) return 3;
    tab->rf[2 * k] = static_cast<int32_t>(first - (fo + 1));
    tab->rf[2 * k + 1] = static_cast<int32_t>(cnt);
    for (int64_t i = first; i <= last; ++i) {
      int64_t q, r;
      double t;
      mg_axis_point(n, m, i, &q, &r, &t);
      tab->rw[4 * k + (i - first)] = q == J ? 1.0 - t : t;
    }
  }
  return 0;
}

}  // namespace gmt
