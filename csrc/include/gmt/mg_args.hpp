// gmt/mg_args.hpp — what every gmt_mg_* call (gmt/kernels.h) accepts, host
// code only.  The gfx950 kernels (csrc/kernels/mg.hip) and the CPU backend
// (csrc/host/kernels_host.cpp) run these checks and no others, so a refusal
// list that passes on one backend holds on the other.
//
// A check answers kRun, kNothing (the call returns 0 without touching memory)
// or kRefuse (hipErrorInvalidValue on the GPU, 1 on the host), in the order
// the entry point documents, and hands back what its caller derives from the
// arguments.  A field's address is formed only after the origins and pitches
// that place it inside the caller's rows were accepted.
#pragma once

#include <cstdint>

#include "gmt/kernels.h"
#include "gmt/mg_tab.hpp"

namespace gmt {

// ---- the fused walk's column geometry (mg.hip asserts both against the row walk's) ----
constexpr int kMgWaveCols = 128;  // columns a wave loads
constexpr int kMgBlockWaves = 4;  // waves per workgroup
constexpr int mg_fuse_shift(int k) { return k / 2 * 2; }  // k - 1 rounded up to even
constexpr int mg_fuse_wave_cols(int k) { return k == 1 ? kMgWaveCols : kMgWaveCols - 2 * mg_fuse_shift(k); }
constexpr int64_t mg_fuse_block_cols(int k) { return static_cast<int64_t>(mg_fuse_wave_cols(k)) * kMgBlockWaves; }

enum class MgCheck { kRun, kNothing, kRefuse };
inline int mg_check_code(MgCheck c, int refuse) { return c == MgCheck::kRefuse ? refuse : 0; }

inline bool mg_bit_ok(int v) { return v == 0 || v == 1; }  // rb, par, px, py
inline bool mg_mask_ok(int mask) { return mask >= 0 && mask <= 15; }
inline bool mg_depth_ok(int k) { return k >= 1 && k <= GMT_MG_MAX_FUSE; }
// coarse points on n fine cells, the first on cell p
inline int64_t mg_coarse_cells(int64_t n, int p) { return (n - p + 1) / 2; }

// ghost cells beyond a region per side: `halo` where the mask has the side, `ring` elsewhere.  u: k or 1;
// f: one less; the coarse field of gmt_mg_prolong_smooth: h / 2 + 1 or 1.
struct MgSides {
  int64_t w = 0, e = 0, s = 0, n = 0;
};
inline MgSides mg_sides(int mask, int64_t halo, int64_t ring) {
  return {mask & GMT_MG_HALO_W ? halo : ring, mask & GMT_MG_HALO_E ? halo : ring,
          mask & GMT_MG_HALO_S ? halo : ring, mask & GMT_MG_HALO_N ? halo : ring};
}

// the cells of a region grown by g, as an address range
struct MgRange {
  const double *a, *e;
  bool overlaps(const MgRange& o) const { return a < o.e && o.a < e; }
};
inline MgRange mg_range(const double* p, int64_t ld, int64_t x0, int64_t nx, int64_t y0, int64_t ny,
                        const MgSides& g = {}) {
  return {p + (y0 - g.s) * ld + (x0 - g.w), p + (y0 + ny + g.n - 1) * ld + (x0 + nx + g.e)};
}

// room for u's read set (g beyond the region), f's (one less) and out's region
inline bool mg_smooth_fields_ok(const MgSides& g, int64_t x0, int64_t nx, int64_t y0, const double* u, int64_t ld,
                                const double* f, int64_t ldf, const double* out, int64_t ldo) {
  return u && out && x0 >= g.w && y0 >= g.s && ld >= x0 + nx + g.e && ldo >= x0 + nx &&
         (!f || ldf >= x0 + nx + (g.e - 1));
}

inline MgCheck mg_smooth_check(int64_t x0, int64_t nx, int64_t y0, int64_t ny, const double* u, int64_t ld,
                               const double* f, int64_t ldf, const double* out, int64_t ldo) {
  if (nx < 0 || ny < 0) return MgCheck::kRefuse;
  if (nx == 0 || ny == 0) return MgCheck::kNothing;
  return mg_smooth_fields_ok({1, 1, 1, 1}, x0, nx, y0, u, ld, f, ldf, out, ldo) ? MgCheck::kRun : MgCheck::kRefuse;
}

// gmt_mg_smooth_k (par = 0) and gmt_mg_smooth_rb: k sweeps or half-sweeps
inline MgCheck mg_fuse_check(int k, int par, int64_t x0, int64_t nx, int64_t y0, int64_t ny, int mask,
                             const double* u, int64_t ld, const double* f, int64_t ldf, const double* out,
                             int64_t ldo) {
  if (!mg_depth_ok(k) || !mg_bit_ok(par) || !mg_mask_ok(mask) || nx < 0 || ny < 0) return MgCheck::kRefuse;
  if (nx == 0 || ny == 0) return MgCheck::kNothing;
  const MgSides g = mg_sides(mask, k, 1);
  if (!mg_smooth_fields_ok(g, x0, nx, y0, u, ld, f, ldf, out, ldo)) return MgCheck::kRefuse;
  // u's read set against out[R]
  return mg_range(u, ld, x0, nx, y0, ny, g).overlaps(mg_range(out, ldo, x0, nx, y0, ny)) ? MgCheck::kRefuse
                                                                                         : MgCheck::kRun;
}

// the coarse columns and rows gmt_mg_prolong_smooth may read, region-relative, inclusive
struct MgCoarseWin {
  int64_t ilo, ihi, jlo, jhi;
};

inline MgCheck mg_prolong_smooth_check(int h, int rb, int par, int64_t x0, int64_t nx, int64_t y0, int64_t ny, int px,
                                       int py, int mask, const double* e, int64_t cx0, int64_t cy0, int64_t lde,
                                       const double* u, int64_t ld, const double* f, int64_t ldf, const double* out,
                                       int64_t ldo, MgCoarseWin* win) {
  if (!mg_bit_ok(rb) || !mg_bit_ok(px) || !mg_bit_ok(py)) return MgCheck::kRefuse;
  const MgCheck c = mg_fuse_check(h, par, x0, nx, y0, ny, mask, u, ld, f, ldf, out, ldo);
  if (c != MgCheck::kRun) return c;
  const MgSides cg = mg_sides(mask, h / 2 + 1, 1);
  const int64_t mx = mg_coarse_cells(nx, px), my = mg_coarse_cells(ny, py);
  if (!e || cx0 < cg.w || cy0 < cg.s || lde < cx0 + mx + cg.e) return MgCheck::kRefuse;
  // out[R] against the read sets of e and f (u's: mg_fuse_check)
  const MgRange o = mg_range(out, ldo, x0, nx, y0, ny);
  if (mg_range(e, lde, cx0, mx, cy0, my, cg).overlaps(o)) return MgCheck::kRefuse;
  if (f && mg_range(f, ldf, x0, nx, y0, ny, mg_sides(mask, h - 1, 0)).overlaps(o)) return MgCheck::kRefuse;
  if (win) *win = {-cg.w, mx - 1 + cg.e, -cg.s, my - 1 + cg.n};
  return MgCheck::kRun;
}

// an empty region returns 0 before px and py are looked at; kNothing too where no coarse point lies on it
inline MgCheck mg_restrict_check(int64_t x0, int64_t nx, int64_t y0, int64_t ny, int px, int py, const double* d,
                                 int64_t ldd, const double* sc, int64_t cx0, int64_t cy0, int64_t ldc, int64_t* mx,
                                 int64_t* my) {
  if (nx < 0 || ny < 0) return MgCheck::kRefuse;
  if (nx == 0 || ny == 0) return MgCheck::kNothing;
  if (!mg_bit_ok(px) || !mg_bit_ok(py)) return MgCheck::kRefuse;
  *mx = mg_coarse_cells(nx, px), *my = mg_coarse_cells(ny, py);
  if (!d || !sc || x0 < 1 || y0 < 1 || cx0 < 0 || cy0 < 0 || ldd < x0 + nx + 1 || ldc < cx0 + *mx)
    return MgCheck::kRefuse;
  return *mx == 0 || *my == 0 ? MgCheck::kNothing : MgCheck::kRun;
}

inline MgCheck mg_resid_restrict_check(int64_t x0, int64_t nx, int64_t y0, int64_t ny, int px, int py, int mask,
                                       const double* u, int64_t ld, const double* f, int64_t ldf, const double* sc,
                                       int64_t cx0, int64_t cy0, int64_t ldc, int64_t* mx, int64_t* my) {
  if (!mg_mask_ok(mask) || nx < 0 || ny < 0) return MgCheck::kRefuse;
  if (nx == 0 || ny == 0) return MgCheck::kNothing;
  if (!mg_bit_ok(px) || !mg_bit_ok(py)) return MgCheck::kRefuse;
  const MgSides g = mg_sides(mask, 2, 1);
  *mx = mg_coarse_cells(nx, px), *my = mg_coarse_cells(ny, py);
  if (!u || !sc || x0 < g.w || y0 < g.s || cx0 < 0 || cy0 < 0 || ld < x0 + nx + g.e || ldc < cx0 + *mx ||
      (f && ldf < x0 + nx + (g.e - 1)))
    return MgCheck::kRefuse;
  if (*mx == 0 || *my == 0) return MgCheck::kNothing;
  // the read sets of u and f against sc's cells
  const MgRange o = mg_range(sc, ldc, cx0, *mx, cy0, *my);
  if (mg_range(u, ld, x0, nx, y0, ny, g).overlaps(o)) return MgCheck::kRefuse;
  if (f && mg_range(f, ldf, x0, nx, y0, ny, mg_sides(mask, 1, 0)).overlaps(o)) return MgCheck::kRefuse;
  return MgCheck::kRun;
}

inline MgCheck mg_prolong_add_check(int64_t x0, int64_t nx, int64_t y0, int64_t ny, int px, int py, const double* e,
                                    int64_t cx0, int64_t cy0, int64_t lde, const double* u, int64_t ld) {
  if (nx < 0 || ny < 0) return MgCheck::kRefuse;
  if (nx == 0 || ny == 0) return MgCheck::kNothing;
  if (!mg_bit_ok(px) || !mg_bit_ok(py)) return MgCheck::kRefuse;
  const int64_t mx = mg_coarse_cells(nx, px);
  return e && u && x0 >= 1 && y0 >= 1 && cx0 >= 1 && cy0 >= 1 && lde >= cx0 + mx + 1 && ld >= x0 + nx
             ? MgCheck::kRun
             : MgCheck::kRefuse;
}

// the table-driven transfers: nx, ny, mx, my are the plan's extents
inline MgCheck mg_restrict_tab_check(int64_t nx, int64_t ny, int64_t mx, int64_t my, int64_t x0, int64_t y0,
                                     const double* d, int64_t ldd, const double* sc, int64_t cx0, int64_t cy0,
                                     int64_t ldc) {
  if (nx == 0 || ny == 0 || mx == 0 || my == 0) return MgCheck::kNothing;
  return d && sc && x0 >= kMgTapHalo && y0 >= kMgTapHalo && cx0 >= 0 && cy0 >= 0 && ldd >= x0 + nx + kMgTapHalo &&
                 ldc >= cx0 + mx
             ? MgCheck::kRun
             : MgCheck::kRefuse;
}

inline MgCheck mg_prolong_add_tab_check(int64_t nx, int64_t ny, int64_t mx, int64_t x0, int64_t y0, const double* e,
                                        int64_t cx0, int64_t cy0, int64_t lde, const double* u, int64_t ld) {
  if (nx == 0 || ny == 0) return MgCheck::kNothing;
  return e && u && x0 >= 1 && y0 >= 1 && cx0 >= kMgRingHalo && cy0 >= kMgRingHalo &&
                 lde >= cx0 + mx + kMgRingHalo && ld >= x0 + nx
             ? MgCheck::kRun
             : MgCheck::kRefuse;
}

}  // namespace gmt
