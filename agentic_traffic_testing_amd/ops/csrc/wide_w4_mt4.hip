// Wide small-M GEMM, MXFP4 (W4) builds for 64-row blocks (MT = 4): see wide.h.
#include "wide.h"

namespace atta {
namespace wide {
ATTA_WIDE_W4_MT_TU(4)
}  // namespace wide
}  // namespace atta
