// Wide small-M GEMM, MXFP4 (W4) builds for 128-row blocks (MT = 8): see wide.h.
#include "wide.h"

namespace atta {
namespace wide {
ATTA_WIDE_W4_MT_TU(8)
}  // namespace wide
}  // namespace atta
