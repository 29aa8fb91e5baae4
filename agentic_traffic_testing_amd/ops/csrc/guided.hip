// Guided decoding: token masks from a device-resident automaton table.
//
// A guide (regex, choice list or JSON schema, compiled on the host by engine/guided.py) is a
// DFA over tokens.  All live guides share one pool:
//   next   int16 [pool_states, vocab]   next[s][v] = the pool state after token v in state s,
//                                       or -1: token v is not allowed in state s
//   state  int32 [slots]                the current pool state of each guided running sequence
// State 0 of the pool is the shared "done" state: it allows the end tokens only and each of
// them leads back to 0, so a look-ahead step launched behind an end token stays harmless.
//
// Two entry points on the decode path, every parameter in device memory (graph-capturable):
//   guide_apply    out[r][v] = next[state[slot[r]]][v] < 0 ? -inf : float(logits[r][v]); a row
//                  with slot < 0 (an unguided row of a mixed step, a padded row of a graph
//                  bucket) or slot >= slots is the raw logits converted to fp32.  The mask is
//                  -inf, not a large finite number: the samplers' Gumbel draw is +inf for one
//                  mantissa value in 2^24, a finite mask plus that draw would win the argmax,
//                  while -inf + inf is NaN, which the samplers' comparison never selects.
//   guide_advance  state[slot[r]] = max(next[state[slot[r]]][tokens[r]], 0) after the sampler
// `logits` may be `out` itself (fp32, same strides): the in-place form behind penalty_apply,
// where every element is read and written by the same lane.
#include "common.h"
#include "kernels.h"

namespace atta {

constexpr int kGuideThreads = 256;
constexpr int kGuideVec = 8;  // elements per lane: 16 B of table, 16 B of bf16 logits
constexpr int kGuideMaxBlocksPerRow = 64;

template <typename LT>
__device__ __forceinline__ float guide_load(const LT* p, int64_t i);
template <>
__device__ __forceinline__ float guide_load<float>(const float* p, int64_t i) {
  return p[i];
}
template <>
__device__ __forceinline__ float guide_load<__bf16>(const __bf16* p, int64_t i) {
  return to_f32<__bf16>(reinterpret_cast<const uint16_t*>(p)[i]);
}
template <>
__device__ __forceinline__ float guide_load<_Float16>(const _Float16* p, int64_t i) {
  return static_cast<float>(p[i]);
}

// eight consecutive logits from a 16-byte aligned address
template <typename LT>
__device__ __forceinline__ void guide_load8(const LT* p, float (&l)[8]) {
  const Pack8 k = *reinterpret_cast<const Pack8*>(p);
#pragma unroll
  for (int j = 0; j < 8; ++j) l[j] = to_f32<LT>(k.v[j]);
}
template <>
__device__ __forceinline__ void guide_load8<float>(const float* p, float (&l)[8]) {
  const f32x4 a = *reinterpret_cast<const f32x4*>(p);
  const f32x4 b = *reinterpret_cast<const f32x4*>(p + 4);
  l[0] = a.x, l[1] = a.y, l[2] = a.z, l[3] = a.w;
  l[4] = b.x, l[5] = b.y, l[6] = b.z, l[7] = b.w;
}

// grid (blocks per row, rows).  No __restrict__ on out / logits: they may be one buffer.
template <typename LT>
__global__ __launch_bounds__(kGuideThreads) void guide_apply_kernel(
    float* out, int64_t out_stride, const LT* logits, int64_t logits_stride,
    const int16_t* __restrict__ next, int vocab, int pool_states,
    const int* __restrict__ state, int num_slots, const int* __restrict__ row_slot) {
  const int row = blockIdx.y;
  const int slot = row_slot[row];
  const bool on = slot >= 0 && slot < num_slots;
  int st = on ? state[slot] : 0;
  st = st < 0 ? 0 : (st >= pool_states ? pool_states - 1 : st);  // never index past the pool
  const LT* lr = logits + static_cast<int64_t>(row) * logits_stride;
  float* orow = out + static_cast<int64_t>(row) * out_stride;
  const int16_t* nr = next + static_cast<int64_t>(st) * vocab;
  const float ninf = -__builtin_huge_valf();

  const bool vec = vocab % kGuideVec == 0 && reinterpret_cast<uintptr_t>(lr) % 16 == 0 &&
                   reinterpret_cast<uintptr_t>(orow) % 16 == 0 &&
                   reinterpret_cast<uintptr_t>(nr) % 16 == 0;
  const int tid = blockIdx.x * kGuideThreads + threadIdx.x;
  const int nthr = gridDim.x * kGuideThreads;
  if (vec) {
    const int nvec = vocab / kGuideVec;
    for (int i = tid; i < nvec; i += nthr) {
      const int64_t e = static_cast<int64_t>(i) * kGuideVec;
      float l[8];
      guide_load8<LT>(lr + e, l);
      if (on) {
        const Pack8 n = *reinterpret_cast<const Pack8*>(nr + e);
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (n.v[j] & 0x8000u) l[j] = ninf;
      }
      *reinterpret_cast<f32x4*>(orow + e) = f32x4{l[0], l[1], l[2], l[3]};
      *reinterpret_cast<f32x4*>(orow + e + 4) = f32x4{l[4], l[5], l[6], l[7]};
    }
    return;
  }
  for (int i = tid; i < vocab; i += nthr) {
    float l = guide_load<LT>(lr, i);
    if (on && nr[i] < 0) l = ninf;
    orow[i] = l;
  }
}

// one lane per row; two rows of a step never share a slot
__global__ __launch_bounds__(kGuideThreads) void guide_advance_kernel(
    int* __restrict__ state, const int16_t* __restrict__ next, int vocab, int pool_states,
    int num_slots, const int* __restrict__ row_slot, const int64_t* __restrict__ tokens,
    int rows) {
  const int row = blockIdx.x * kGuideThreads + threadIdx.x;
  if (row >= rows) return;
  const int slot = row_slot[row];
  if (slot < 0 || slot >= num_slots) return;
  int st = state[slot];
  st = st < 0 ? 0 : (st >= pool_states ? pool_states - 1 : st);
  const int64_t tok = tokens[row];
  int n = -1;
  if (tok >= 0 && tok < vocab) n = next[static_cast<int64_t>(st) * vocab + tok];
  state[slot] = (n >= 0 && n < pool_states) ? n : 0;
}

}  // namespace atta

using namespace atta;

template <typename LT>
static void launch_guide_apply(float* out, int64_t out_stride, const void* logits,
                               int64_t logits_stride, const int16_t* next, int rows, int vocab,
                               int pool_states, const int* state, int num_slots,
                               const int* row_slot, hipStream_t stream) {
  int bx = (vocab + kGuideThreads * kGuideVec - 1) / (kGuideThreads * kGuideVec);
  bx = bx < 1 ? 1 : (bx > kGuideMaxBlocksPerRow ? kGuideMaxBlocksPerRow : bx);
  guide_apply_kernel<LT><<<dim3(bx, rows), kGuideThreads, 0, stream>>>(
      out, out_stride, static_cast<const LT*>(logits), logits_stride, next, vocab, pool_states,
      state, num_slots, row_slot);
}

int atta_guide_apply(float* out, int64_t out_stride, const void* logits, int64_t logits_stride,
                     int logits_dtype, const int16_t* next, int rows, int vocab, int pool_states,
                     const int* state, int num_slots, const int* row_slot, hipStream_t stream) {
  if (rows == 0 || vocab == 0) return 0;
  if (rows > 65535 || pool_states < 1) return static_cast<int>(hipErrorInvalidValue);
  if (logits_dtype == 2)
    launch_guide_apply<float>(out, out_stride, logits, logits_stride, next, rows, vocab,
                              pool_states, state, num_slots, row_slot, stream);
  else if (logits_dtype == 1)
    launch_guide_apply<_Float16>(out, out_stride, logits, logits_stride, next, rows, vocab,
                                 pool_states, state, num_slots, row_slot, stream);
  else
    launch_guide_apply<__bf16>(out, out_stride, logits, logits_stride, next, rows, vocab,
                               pool_states, state, num_slots, row_slot, stream);
  return static_cast<int>(hipGetLastError());
}

int atta_guide_advance(int* state, const int16_t* next, int vocab, int pool_states,
                       int num_slots, const int* row_slot, const int64_t* tokens, int rows,
                       hipStream_t stream) {
  if (rows == 0) return 0;
  if (pool_states < 1) return static_cast<int>(hipErrorInvalidValue);
  guide_advance_kernel<<<(rows + kGuideThreads - 1) / kGuideThreads, kGuideThreads, 0, stream>>>(
      state, next, vocab, pool_states, num_slots, row_slot, tokens, rows);
  return static_cast<int>(hipGetLastError());
}
