// Strip geometry of the temporal-blocking Jacobi kernel
// (csrc/kernels/jacobi5tb.hpp), shared by the gfx950 launcher, the CPU
// backend (csrc/host/kernels_host.cpp) and the engine's planners, so the
// column counts every layer reasons with are the kernel's own.
//
//   4 columns per lane = 256 columns; one wave per strip up to K = 10, two
//   waves (levels split) for even K = 12..20.
// The left margin KL is the number of window columns left of the first
// output column: K rounded up so the output starts on a lane boundary; the
// right margin mirrors it.  (The round-4 wide K = 20 strip, six columns per
// lane over four stages, is in git history: profiles/r04_wide.md.)
#pragma once

#include <cstdint>

namespace gmt {
namespace tb {

constexpr int kMaxK1 = 10;  // largest single-wave K

constexpr int tb_nc(int) { return 4; }
constexpr int tb_stages(int K) { return K <= kMaxK1 ? 1 : 2; }
constexpr int tb_cols(int K) { return tb_nc(K) * 64; }
constexpr int tb_left(int K) { return (K + 3) / 4 * 4; }
constexpr int tb_strip_out(int K) { return tb_cols(K) - 2 * tb_left(K); }
// strips per workgroup: at most 512 threads; default one strip per
// workgroup for multi-stage strips, four single-wave strips otherwise
constexpr int tb_max_strips(int K) { return 8 / tb_stages(K); }
constexpr int tb_default_strips(int K) { return tb_stages(K) == 1 ? 4 : 1; }
// Sweep counts with an inline-halo (push) kernel: the face stores' two
// per-lane offsets and three descriptors spill the K = 6-10 one-wave strips
// (253-255 VGPRs without them; K = 10 since the exec-masked Dirichlet keep's
// column masks took 8 SGPRs, K = 6 since the push body is chosen per wave)
// and K = 14; the engine plans around them
constexpr bool tb_push_built(int K) { return (K < 6 || K > 10) && K != 14; }

// Shared hand-off groups (csrc/kernels/jacobi5tb.hpp Sh<K, NW>): NW adjacent
// two-stage strips whose stage-1 waves read 256-column windows of one shared
// level-K/2 row.  A group kernel exists for two or four strips of a two-stage
// K whose stages hold an even number of levels (K = 12, 16, 20).
constexpr int sh_nl(int K) { return K / 2; }                   // levels per stage
constexpr bool sh_ok(int K, int NW = 4) { return tb_stages(K) == 2 && sh_nl(K) % 2 == 0 && (NW == 2 || NW == 4); }
constexpr int sh_s0(int K) { return 256 - 2 * sh_nl(K); }      // stage-0 window spacing
constexpr int sh_o(int K) { return (sh_nl(K) + 3) / 4 * 4; }   // first stage-1 window, from the group's
constexpr int sh_s1(int K, int NW) {                           // stage-1 window spacing
  return (sh_s0(K) * (NW - 1) - sh_nl(K) - sh_o(K)) / (NW - 1) / 4 * 4;
}
constexpr int sh_gout(int K, int NW) { return sh_s1(K, NW) * (NW - 1) + 256 - 2 * sh_nl(K); }  // output columns of a group
constexpr int sh_ml(int K) { return sh_o(K) + sh_nl(K); }      // group window start -> output start
// column slot (0..3 of a lane) of the W / E ghost column in the first / last
// strip's windows of a pass whose rect is the interior
constexpr int sh_jw(int K) { return (sh_ml(K) - 1) % 4; }
constexpr int sh_je(int K, int NW) { return (sh_gout(K, NW) + sh_ml(K)) % 4; }
// {GOUT, ML, NL, O, S0, S1, kJW, kJE} (gmt_jacobi5tb_shared_geom); false when
// no group kernel exists for (K, NW)
constexpr bool sh_geom(int K, int NW, std::int64_t out[8]) {
  if (!sh_ok(K, NW)) return false;
  out[0] = sh_gout(K, NW);
  out[1] = sh_ml(K);
  out[2] = sh_nl(K);
  out[3] = sh_o(K);
  out[4] = sh_s0(K);
  out[5] = sh_s1(K, NW);
  out[6] = sh_jw(K);
  out[7] = sh_je(K, NW);
  return true;
}

// (K, NW) with an inline-halo (push) group kernel: a K with both a group
// kernel and a push kernel whose push-group body fits 2 waves per SIMD
// without scratch or VGPR spills (tests/test_kernel_resources.py)
constexpr bool tb_push_sh_built(int K, int NW) { return sh_ok(K, NW) && tb_push_built(K); }

}  // namespace tb
}  // namespace gmt
