// Multi-query decode paged attention, the verify step of speculative decoding: the MQ = true
// instantiations of attention_decode_core.h (the kernel is described there).
//
// A column of a one-token sequence goes through the one-token kernel's operations in the
// same order here, but the two instantiations are not held to the same last bit (the
// compiler is free to contract the combine's folds into different FMA forms), so
// ops.attention_decode_mq sends one-token sequences to that kernel itself and this one sees
// kvlen = 0 for them (as each skips the other's sequences).
#include "attention_decode_core.h"
#include "kernels.h"

namespace atta {
namespace dec {

template <typename T, int G, int WAVES, int TPW>
__global__ __launch_bounds__(WAVES * 64) void decode_attention_mq_kernel(DecParams p) {
  unsigned long long tr[3];  // the timeline probe is the one-token kernel's
  decode_attention_body<T, G, WAVES, TPW, true>(p, blockIdx.x, blockIdx.y, blockIdx.z, tr);
}

}  // namespace dec
}  // namespace atta

using namespace atta;

int atta_attention_decode_mq(void* out, float* part_out, float* part_lse, int* counters,
                             const void* q, const void* k_cache, const void* v_cache,
                             const int* block_tables, const int* seq_kvlen, const int* seq_qstart,
                             int num_seqs, int max_parts, int part_tokens, int n_q_heads,
                             int n_kv_heads, int head_dim, int block_size, int bt_stride,
                             int64_t q_stride, int64_t out_stride, float scale, int dtype,
                             hipStream_t stream) {
  // the 16-wave 512-token shape of the one-token kernel has no multi-query twin
  if (part_tokens != 64 && part_tokens != 128 && part_tokens != 256) return -1;
  return dec::decode_attention<true>(out, part_out, part_lse, counters, q, k_cache, v_cache,
                                     block_tables, seq_kvlen, seq_qstart, num_seqs, max_parts,
                                     part_tokens, n_q_heads, n_kv_heads, head_dim, block_size,
                                     bt_stride, q_stride, out_stride, scale, dtype, stream, 8,
                                     nullptr);
}
