// Decode paged attention, one query token per sequence: the MQ = false instantiations of
// attention_decode_core.h (the kernel is described there), the timeline probe and the
// ATTA_ATTN128_WAVES switch.
#include <cstdlib>

#include "attention_decode_core.h"
#include "kernels.h"

namespace atta {
namespace dec {

template <typename T, int G, int WAVES, int TPW>
__global__ __launch_bounds__(WAVES * 64) void decode_attention_kernel(DecParams p) {
  unsigned long long tr[3] = {0, 0, 0};
  decode_attention_body<T, G, WAVES, TPW, false>(p, blockIdx.x, blockIdx.y, blockIdx.z, tr);
  // timeline probe (set_attention_trace): [past round trip 1, computed, published, end]
  if (p.wg_trace != nullptr && threadIdx.x == 0) {
    const int64_t b = blockIdx.x + static_cast<int64_t>(gridDim.x) *
                                       (blockIdx.y + static_cast<int64_t>(gridDim.y) * blockIdx.z);
    p.wg_trace[4 * b] = tr[0];
    p.wg_trace[4 * b + 1] = tr[1];
    p.wg_trace[4 * b + 2] = tr[2];
    p.wg_trace[4 * b + 3] = wall_clock64();
  }
}

// 128-token partitions (the decode batches <= 8 of the headline) run as 8 waves x 1 tile:
// half the serial QK / softmax / PV chain per wave and twice the waves in flight against
// 4 waves x 2 tiles - bench 767.9 / 769.2 vs 762.4 / 764.0 tok/s interleaved on one box
// (profiles/r5_attention_8wave.txt).  ATTA_ATTN128_WAVES=4 restores 4 x 2 (read once).
static int attn128_waves() {
  static const int w = [] {
    const char* v = std::getenv("ATTA_ATTN128_WAVES");
    return v != nullptr && std::atoi(v) == 4 ? 4 : 8;
  }();
  return w;
}

}  // namespace dec
}  // namespace atta

using namespace atta;

static unsigned long long* g_attn_trace = nullptr;

// Timeline probe for the decode attention launches that follow (nullptr: off).
void atta_set_attention_trace(void* trace) {
  g_attn_trace = static_cast<unsigned long long*>(trace);
}

int atta_attention_decode_v2(void* out, float* part_out, float* part_lse, int* counters,
                             const void* q, const void* k_cache, const void* v_cache,
                             const int* block_tables, const int* seq_kvlen, const int* seq_qstart,
                             int num_seqs, int max_parts, int part_tokens, int n_q_heads,
                             int n_kv_heads, int head_dim, int block_size, int bt_stride,
                             int64_t q_stride, int64_t out_stride, float scale, int dtype,
                             hipStream_t stream) {
  return dec::decode_attention<false>(out, part_out, part_lse, counters, q, k_cache, v_cache,
                                      block_tables, seq_kvlen, seq_qstart, num_seqs, max_parts,
                                      part_tokens, n_q_heads, n_kv_heads, head_dim, block_size,
                                      bt_stride, q_stride, out_stride, scale, dtype, stream,
                                      dec::attn128_waves(), g_attn_trace);
}
