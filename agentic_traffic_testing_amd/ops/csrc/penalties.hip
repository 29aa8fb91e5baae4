// Sampling penalties and logit bias over device-resident token counts.
//
// A penalised sequence owns one row ("slot") of an int32 state tensor [slots, vocab]; word v:
//   bit 31     token v occurs in the prompt
//   bits 0-30  times token v was generated
// so the hot kernel takes ONE load per element for both facts.  Next to it each slot has a
// 300-entry logit-bias table: int32 ids (-1 padded, unique) and fp32 values.
//
// For a sampled row with slot s >= 0, per token v, from the raw logit l in fp32:
//   1. seen = word != 0 (prompt flag or count):  l = l > 0 ? l / rep : l * rep
//   2. c = count:                                l -= freq * c;  l -= pres * (c > 0)
//   3.                                           l += bias[v] if present
// The fp32 result feeds ops.sample / ops.sample_topkp unrounded.  A row with slot < 0 (an
// unpenalised row of a mixed step, a padded row of a graph bucket) is copied through converted
// to fp32 and reads no state.
//
// Three entry points, all parameters in device memory (graph-capturable):
//   penalty_seed    zero a slot's row, set prompt flags, add output counts, write its bias table
//                   (admission / re-admission after a preemption; not on the decode path)
//   penalty_apply   the dense pass (kernel 1) followed by the bias entries (kernel 2): two
//                   launches on one stream, so every bias read-modify-write comes after the
//                   dense store of its element and no element is touched by two threads
//   penalty_update  count[slot[r], tokens[r]] += 1 after the sampler
#include "common.h"
#include "kernels.h"

namespace atta {

constexpr int kPenThreads = 256;
constexpr int kPenVec = 4;            // elements per lane and access: 16 B of state and of out
constexpr int kPenMaxBlocksPerRow = 64;
constexpr int kPenBias = 300;         // bias entries per slot (OpenAI's logit_bias limit)
constexpr uint32_t kPromptBit = 0x80000000u;
constexpr uint32_t kCountMask = 0x7fffffffu;

template <typename LT>
__device__ __forceinline__ float pen_load(const LT* p, int64_t i);
template <>
__device__ __forceinline__ float pen_load<float>(const float* p, int64_t i) {
  return p[i];
}
template <>
__device__ __forceinline__ float pen_load<__bf16>(const __bf16* p, int64_t i) {
  return to_f32<__bf16>(reinterpret_cast<const uint16_t*>(p)[i]);
}
template <>
__device__ __forceinline__ float pen_load<_Float16>(const _Float16* p, int64_t i) {
  return static_cast<float>(p[i]);
}

// four consecutive logits from an address aligned to 4 elements
template <typename LT>
__device__ __forceinline__ f32x4 pen_load4(const LT* p);
template <>
__device__ __forceinline__ f32x4 pen_load4<float>(const float* p) {
  return *reinterpret_cast<const f32x4*>(p);
}
template <>
__device__ __forceinline__ f32x4 pen_load4<__bf16>(const __bf16* p) {
  const Pack4 k = *reinterpret_cast<const Pack4*>(p);
  return f32x4{to_f32<__bf16>(k.v[0]), to_f32<__bf16>(k.v[1]), to_f32<__bf16>(k.v[2]),
               to_f32<__bf16>(k.v[3])};
}
template <>
__device__ __forceinline__ f32x4 pen_load4<_Float16>(const _Float16* p) {
  const Pack4 k = *reinterpret_cast<const Pack4*>(p);
  return f32x4{to_f32<_Float16>(k.v[0]), to_f32<_Float16>(k.v[1]), to_f32<_Float16>(k.v[2]),
               to_f32<_Float16>(k.v[3])};
}

__device__ __forceinline__ float penalise(float l, uint32_t w, float rep, float inv_rep,
                                          float freq, float pres) {
  if (w != 0u) l = l > 0.f ? l * inv_rep : l * rep;
  const uint32_t c = w & kCountMask;
  l -= freq * static_cast<float>(c);
  if (c != 0u) l -= pres;
  return l;
}

// grid (blocks per row, rows); a row whose three row pointers are 16-byte (logits: 4-element)
// aligned goes 4 elements a lane with a scalar tail, any other row element by element
template <typename LT>
__global__ __launch_bounds__(kPenThreads) void penalty_apply_kernel(
    float* __restrict__ out, int64_t out_stride, const LT* __restrict__ logits,
    int64_t logits_stride, const uint32_t* __restrict__ state, int vocab, int num_slots,
    const int* __restrict__ row_slot, const float* __restrict__ rep,
    const float* __restrict__ freq, const float* __restrict__ pres) {
  const int row = blockIdx.y;
  int slot = row_slot[row];
  if (slot >= num_slots) slot = -1;  // never index past the state
  const bool on = slot >= 0;
  const LT* lr = logits + static_cast<int64_t>(row) * logits_stride;
  float* orow = out + static_cast<int64_t>(row) * out_stride;
  const uint32_t* sr = state + static_cast<int64_t>(on ? slot : 0) * vocab;
  const float r = on ? rep[row] : 1.f;
  const float inv_r = 1.f / r;
  const float f = on ? freq[row] : 0.f;
  const float p = on ? pres[row] : 0.f;

  const bool vec = reinterpret_cast<uintptr_t>(lr) % (kPenVec * sizeof(LT)) == 0 &&
                   reinterpret_cast<uintptr_t>(orow) % 16 == 0 &&
                   (!on || reinterpret_cast<uintptr_t>(sr) % 16 == 0);
  const int tid = blockIdx.x * kPenThreads + threadIdx.x;
  const int nthr = gridDim.x * kPenThreads;
  const int nvec = vec ? vocab / kPenVec : 0;
  for (int i = tid; i < nvec; i += nthr) {
    f32x4 l = pen_load4<LT>(lr + static_cast<int64_t>(i) * kPenVec);
    if (on) {
      const u32x4 w = *reinterpret_cast<const u32x4*>(sr + static_cast<int64_t>(i) * kPenVec);
      l.x = penalise(l.x, w.x, r, inv_r, f, p);
      l.y = penalise(l.y, w.y, r, inv_r, f, p);
      l.z = penalise(l.z, w.z, r, inv_r, f, p);
      l.w = penalise(l.w, w.w, r, inv_r, f, p);
    }
    *reinterpret_cast<f32x4*>(orow + static_cast<int64_t>(i) * kPenVec) = l;
  }
  for (int i = nvec * kPenVec + tid; i < vocab; i += nthr) {
    float l = pen_load<LT>(lr, i);
    if (on) l = penalise(l, sr[i], r, inv_r, f, p);
    orow[i] = l;
  }
}

// one workgroup per row, one lane per bias entry; ids of a slot's table are unique, so every
// element has one writer
__global__ __launch_bounds__(320) void penalty_bias_kernel(
    float* __restrict__ out, int64_t out_stride, int vocab, int num_slots,
    const int* __restrict__ row_slot, const int* __restrict__ bias_ids,
    const float* __restrict__ bias_vals) {
  const int row = blockIdx.x;
  const int slot = row_slot[row];
  if (slot < 0 || slot >= num_slots || threadIdx.x >= kPenBias) return;
  const int id = bias_ids[static_cast<int64_t>(slot) * kPenBias + threadIdx.x];
  if (id < 0 || id >= vocab) return;
  out[static_cast<int64_t>(row) * out_stride + id] +=
      bias_vals[static_cast<int64_t>(slot) * kPenBias + threadIdx.x];
}

__global__ __launch_bounds__(kPenThreads) void penalty_update_kernel(
    uint32_t* __restrict__ state, int vocab, int num_slots, const int* __restrict__ row_slot,
    const int64_t* __restrict__ tokens, int rows) {
  const int row = blockIdx.x * kPenThreads + threadIdx.x;
  if (row >= rows) return;
  const int slot = row_slot[row];
  const int64_t tok = tokens[row];
  if (slot < 0 || slot >= num_slots || tok < 0 || tok >= vocab) return;
  atomicAdd(state + static_cast<int64_t>(slot) * vocab + tok, 1u);
}

// after the row was zeroed (stream order): prompt flags, output counts (duplicates in either
// list meet in the atomics) and the slot's bias table, padded with -1
__global__ __launch_bounds__(kPenThreads) void penalty_seed_kernel(
    uint32_t* __restrict__ state_row, int vocab, const int* __restrict__ prompt_ids, int n_prompt,
    const int* __restrict__ output_ids, int n_output, int* __restrict__ bias_ids_row,
    float* __restrict__ bias_vals_row, const int* __restrict__ bias_ids,
    const float* __restrict__ bias_vals, int n_bias) {
  const int tid = blockIdx.x * kPenThreads + threadIdx.x;
  const int nthr = gridDim.x * kPenThreads;
  for (int i = tid; i < n_prompt; i += nthr) {
    const int id = prompt_ids[i];
    if (id >= 0 && id < vocab) atomicOr(state_row + id, kPromptBit);
  }
  for (int i = tid; i < n_output; i += nthr) {
    const int id = output_ids[i];
    if (id >= 0 && id < vocab) atomicAdd(state_row + id, 1u);
  }
  for (int i = tid; i < kPenBias; i += nthr) {
    const bool have = i < n_bias;
    bias_ids_row[i] = have ? bias_ids[i] : -1;
    bias_vals_row[i] = have ? bias_vals[i] : 0.f;
  }
}

}  // namespace atta

using namespace atta;

int atta_penalty_seed(int* state_row, int vocab, const int* prompt_ids, int n_prompt,
                      const int* output_ids, int n_output, int* bias_ids_row,
                      float* bias_vals_row, const int* bias_ids, const float* bias_vals,
                      int n_bias, hipStream_t stream) {
  if (n_bias > kPenBias) return static_cast<int>(hipErrorInvalidValue);
  hipError_t e = hipMemsetAsync(state_row, 0, static_cast<size_t>(vocab) * sizeof(int), stream);
  if (e != hipSuccess) return static_cast<int>(e);
  const int n = n_prompt > n_output ? n_prompt : n_output;
  int blocks = (n + kPenThreads - 1) / kPenThreads;
  blocks = blocks < 2 ? 2 : (blocks > 256 ? 256 : blocks);  // >= 300 lanes for the bias table
  penalty_seed_kernel<<<blocks, kPenThreads, 0, stream>>>(
      reinterpret_cast<uint32_t*>(state_row), vocab, prompt_ids, n_prompt, output_ids, n_output,
      bias_ids_row, bias_vals_row, bias_ids, bias_vals, n_bias);
  return static_cast<int>(hipGetLastError());
}

template <typename LT>
static void launch_apply(float* out, int64_t out_stride, const void* logits,
                         int64_t logits_stride, const int* state, int rows, int vocab,
                         int num_slots, const int* row_slot, const float* rep, const float* freq,
                         const float* pres, hipStream_t stream) {
  int bx = (vocab + kPenThreads * kPenVec * 2 - 1) / (kPenThreads * kPenVec * 2);
  bx = bx < 1 ? 1 : (bx > kPenMaxBlocksPerRow ? kPenMaxBlocksPerRow : bx);
  penalty_apply_kernel<LT><<<dim3(bx, rows), kPenThreads, 0, stream>>>(
      out, out_stride, static_cast<const LT*>(logits), logits_stride,
      reinterpret_cast<const uint32_t*>(state), vocab, num_slots, row_slot, rep, freq, pres);
}

int atta_penalty_apply(float* out, int64_t out_stride, const void* logits, int64_t logits_stride,
                       int logits_dtype, const int* state, int rows, int vocab, int num_slots,
                       const int* row_slot, const float* rep, const float* freq,
                       const float* pres, const int* bias_ids, const float* bias_vals,
                       hipStream_t stream) {
  if (rows == 0 || vocab == 0) return 0;
  if (rows > 65535) return static_cast<int>(hipErrorInvalidValue);
  if (logits_dtype == 2)
    launch_apply<float>(out, out_stride, logits, logits_stride, state, rows, vocab, num_slots,
                        row_slot, rep, freq, pres, stream);
  else if (logits_dtype == 1)
    launch_apply<_Float16>(out, out_stride, logits, logits_stride, state, rows, vocab, num_slots,
                           row_slot, rep, freq, pres, stream);
  else
    launch_apply<__bf16>(out, out_stride, logits, logits_stride, state, rows, vocab, num_slots,
                         row_slot, rep, freq, pres, stream);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return static_cast<int>(e);
  penalty_bias_kernel<<<rows, 320, 0, stream>>>(out, out_stride, vocab, num_slots, row_slot,
                                                bias_ids, bias_vals);
  return static_cast<int>(hipGetLastError());
}

int atta_penalty_update(int* state, int vocab, int num_slots, const int* row_slot,
                        const int64_t* tokens, int rows, hipStream_t stream) {
  if (rows == 0) return 0;
  penalty_update_kernel<<<(rows + kPenThreads - 1) / kPenThreads, kPenThreads, 0, stream>>>(
      reinterpret_cast<uint32_t*>(state), vocab, num_slots, row_slot, tokens, rows);
  return static_cast<int>(hipGetLastError());
}
