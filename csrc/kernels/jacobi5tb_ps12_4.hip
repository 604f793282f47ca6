// Instantiations of the temporal-blocking kernel (jacobi5tb.hpp): the inline-halo
// (push) pass in shared hand-off groups of 4 strips, K = 12.
#include "jacobi5tb.hpp"

namespace gmt {
namespace tb {
GMT_TB_PUSH_SH(, 12, 4);
}  // namespace tb
}  // namespace gmt
