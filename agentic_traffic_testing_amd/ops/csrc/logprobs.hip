// Per-token log-probabilities over a materialised logits row (docs/kernels.md, "Logprobs").
//
// One 1024-thread workgroup per row of a [rows, vocab] logits tensor (bf16 or fp32):
//   lp[row]          = l[token[row]] - logZ,  logZ = max + log(sum exp(l - max)), all fp32
//   top_ids/top_lp   = the n_top most likely tokens of the row and their logprobs, higher logit
//                      first, equal logits by lower id first
// The raw logits are what the samplers see (sampling.hip): before temperature, Gumbel noise and
// top-k / top-p.
//
// Top-N is n_top passes of a key-ordered block max over the row: key = (ordered bits of the
// logit) << 32 | (0xFFFFFFFF - id), the sampler's (score, -id) packing, and pass p takes the
// largest key below pass p - 1's.  Keys are distinct (they carry the id), so the order is
// exact, ties included.  A row of 128 256 bf16 logits is 250 KB: the n_top + 2 sweeps are
// served by L2.  Token ids and logits are read from device memory and n_top is a launch
// constant, so a captured launch replays as is.
#include "common.h"
#include "kernels.h"

namespace atta {

constexpr int kLpThreads = 1024;
constexpr int kLpWaves = kLpThreads / kWave;

// Order-preserving uint32 image of a float (-0 is folded into +0 first: the two compare equal
// as logits, so only the id may order them) and its inverse.
__device__ __forceinline__ uint32_t lp_ordered(float v) {
  const uint32_t b = __float_as_uint(v + 0.f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float lp_unordered(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// f(logit, index) over one row, 16 B per lane per load where the row allows (base 16-B aligned;
// the host passes `vec` = 0 otherwise), elements past the last full packet one by one.
template <typename F>
__device__ __forceinline__ void lp_for_each(const uint16_t* lr, int vocab, bool vec, F f) {
  const int nv = vec ? (vocab & ~7) : 0;
  for (int i = threadIdx.x * 8; i < nv; i += kLpThreads * 8) {
    const Pack8 p = *reinterpret_cast<const Pack8*>(lr + i);
#pragma unroll
    for (int j = 0; j < 8; ++j) f(to_f32<__bf16>(p.v[j]), i + j);
  }
  for (int i = nv + threadIdx.x; i < vocab; i += kLpThreads) f(to_f32<__bf16>(lr[i]), i);
}
template <typename F>
__device__ __forceinline__ void lp_for_each(const float* lr, int vocab, bool vec, F f) {
  const int nv = vec ? (vocab & ~3) : 0;
  for (int i = threadIdx.x * 4; i < nv; i += kLpThreads * 4) {
    const f32x4 p = *reinterpret_cast<const f32x4*>(lr + i);
#pragma unroll
    for (int j = 0; j < 4; ++j) f(p[j], i + j);
  }
  for (int i = nv + threadIdx.x; i < vocab; i += kLpThreads) f(lr[i], i);
}

__device__ __forceinline__ float load_row_logit(const uint16_t* lr, int i) {
  return to_f32<__bf16>(lr[i]);
}
__device__ __forceinline__ float load_row_logit(const float* lr, int i) { return lr[i]; }

template <typename LT>
__global__ __launch_bounds__(kLpThreads) void token_logprobs_kernel(
    float* __restrict__ lp, int* __restrict__ top_ids, float* __restrict__ top_lp,
    const LT* __restrict__ logits, const int64_t* __restrict__ tokens, int vocab,
    int64_t stride, int n_top, int vec) {
  __shared__ float sf[kLpWaves];
  __shared__ unsigned long long sk[2][kLpWaves];
  const int row = blockIdx.x;
  const LT* lr = logits + static_cast<int64_t>(row) * stride;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;

  // row max, then sum exp(l - max)
  float mx = -__builtin_huge_valf();
  lp_for_each(lr, vocab, vec != 0, [&](float v, int) { mx = fmaxf(mx, v); });
  mx = wave_max(mx);
  if (lane == 0) sf[wid] = mx;
  __syncthreads();
  mx = sf[0];
#pragma unroll
  for (int w = 1; w < kLpWaves; ++w) mx = fmaxf(mx, sf[w]);
  __syncthreads();
  float sum = 0.f;
  lp_for_each(lr, vocab, vec != 0, [&](float v, int) { sum += expf(v - mx); });
  sum = block_sum(sum, sf);
  const float log_z = mx + logf(sum);

  if (threadIdx.x == 0) {
    const int64_t t = tokens[row];
    // an id outside the row has no logit: NaN, never a read past the row
    lp[row] = (t >= 0 && t < vocab) ? load_row_logit(lr, static_cast<int>(t)) - log_z
                                    : __builtin_nanf("");
  }

  unsigned long long prev = ~0ull;  // above every key: the id field of a key is >= 1
  for (int p = 0; p < n_top; ++p) {
    unsigned long long best = 0;  // below every key: ordered bits of a float are >= 1
    lp_for_each(lr, vocab, vec != 0, [&](float v, int i) {
      const unsigned long long k = (static_cast<unsigned long long>(lp_ordered(v)) << 32) |
                                   (0xFFFFFFFFu - static_cast<uint32_t>(i));
      if (k < prev && k > best) best = k;
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long ok = __shfl_xor(best, o, kWave);
      best = ok > best ? ok : best;
    }
    // two LDS rows, by pass parity: a wave may write pass p + 1's row while another still
    // reads pass p's; the barrier of pass p + 1 orders pass p's reads before pass p + 2's writes
    unsigned long long* s = sk[p & 1];
    if (lane == 0) s[wid] = best;
    __syncthreads();
    best = s[0];
#pragma unroll
    for (int w = 1; w < kLpWaves; ++w) best = s[w] > best ? s[w] : best;
    if (threadIdx.x == 0) {
      const bool found = best != 0;  // n_top > vocab: the row has run out
      const int64_t o = static_cast<int64_t>(row) * n_top + p;
      top_ids[o] = found ? static_cast<int>(0xFFFFFFFFu - static_cast<uint32_t>(best)) : -1;
      top_lp[o] = found ? lp_unordered(static_cast<uint32_t>(best >> 32)) - log_z
                        : -__builtin_huge_valf();
    }
    prev = best;
  }
}

}  // namespace atta

using namespace atta;

int atta_token_logprobs(float* lp, int* top_ids, float* top_lp, const void* logits,
                        const int64_t* tokens, int rows, int vocab, int64_t stride,
                        int logits_is_fp32, int n_top, hipStream_t stream) {
  if (rows == 0) return 0;
  const int esize = logits_is_fp32 ? 4 : 2;
  const int vec = reinterpret_cast<uintptr_t>(logits) % 16 == 0 && (stride * esize) % 16 == 0;
  if (logits_is_fp32)
    token_logprobs_kernel<float><<<rows, kLpThreads, 0, stream>>>(
        lp, top_ids, top_lp, static_cast<const float*>(logits), tokens, vocab, stride, n_top,
        vec);
  else
    token_logprobs_kernel<uint16_t><<<rows, kLpThreads, 0, stream>>>(
        lp, top_ids, top_lp, static_cast<const uint16_t*>(logits), tokens, vocab, stride, n_top,
        vec);
  return static_cast<int>(hipGetLastError());
}
