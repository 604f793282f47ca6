// Instantiations of the temporal-blocking kernel (jacobi5tb.hpp): the inline-halo
// (push) pass in shared hand-off groups of 2 strips, K = 16.
#include "jacobi5tb.hpp"

namespace gmt {
namespace tb {
GMT_TB_PUSH_SH(, 16, 2);
}  // namespace tb
}  // namespace gmt
