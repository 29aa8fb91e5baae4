// Wide small-M GEMM, MXFP4 (W4) builds for 48-row blocks (MT = 3): see wide.h.
#include "wide.h"

namespace atta {
namespace wide {
ATTA_WIDE_W4_MT_TU(3)
}  // namespace wide
}  // namespace atta
