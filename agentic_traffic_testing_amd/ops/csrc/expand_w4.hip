// MXFP4 -> 16-bit expansion (ops.expand_mxfp4): one projection's pre-shuffled 4-bit codes and
// e8m0 block scales (the layout of ops.preshuffle_mxfp4, skinny_w4.h) into a row-major [N, K]
// bf16 / fp16 matrix, the tile row map undone.  The weights-only MXFP4 mode runs it into one
// shared scratch in front of every GEMM that has no 4-bit kernel; the values are those the
// 4-bit GEMV and wide builds compute with (the same convert, fp4x8_to_frag).
//
// A pure stream: 0.53 B in, 2 B out per weight.  One wave per (16-row tile, 128-wide K chunk):
// one 1 KiB code load + one scale dword per lane, four converts.  A lane's four 16-byte results
// are row (lane & 15), k = 32 j + 8 (lane >> 4): stored directly, the 64 lanes of a store would
// touch 16 rows in 64-byte pieces - half a 128-B line each.  So the wave transposes through its
// own 4 KiB of LDS (rows padded by one 16-B slot) and every store instruction writes four rows'
// whole 256-byte chunk segments, two full lines per row.
#include "common.h"
#include "kernels.h"
#include "skinny_w4.h"

namespace atta {

constexpr int kExpWaves = 4;
constexpr int kExpRowB = 256 + 16;  // staged row: 128 values + one slot of padding

// weight row of column c of a tile under a row map (skinny.h tile_row)
__device__ __forceinline__ int expand_row(int rowmap, int tile, int c, int inter) {
  if (rowmap == 1) return (tile >> 3) * 128 + (tile & 7) * 8 + (c & 7) + ((c & 8) ? 64 : 0);
  if (rowmap == 2) return c < 8 ? tile * 8 + c : inter + tile * 8 + c - 8;
  return tile * 16 + c;
}

template <typename T>
__global__ __launch_bounds__(kExpWaves * 64) void expand_mxfp4_kernel(
    uint16_t* __restrict__ out, const uint8_t* __restrict__ codes,
    const uint8_t* __restrict__ bscale, int nch, int ncg, int64_t out_stride, int rowmap,
    int inter) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[kExpWaves][16 * kExpRowB];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int col = lane & 15, grp = lane >> 4;
  const int tile = blockIdx.x / ncg;
  const int c = (blockIdx.x % ncg) * kExpWaves + wid;
  const bool live = c < nch;  // wave-uniform; a dead wave re-reads the last chunk, stores nothing
  const int64_t blk = static_cast<int64_t>(tile) * nch + (live ? c : nch - 1);
  const u32x4 w = __builtin_nontemporal_load(
      reinterpret_cast<const u32x4*>(codes + blk * 1024 + lane * 16));
  const uint32_t s = *reinterpret_cast<const uint32_t*>(bscale + blk * 64 + col * 4);
  unsigned char* my = lds[wid];
#pragma unroll
  for (int j = 0; j < 4; ++j)
    *reinterpret_cast<u32x4*>(my + col * kExpRowB + j * 64 + grp * 16) =
        __builtin_bit_cast(u32x4, fp4x8_to_frag<T>(w[j], (s >> (8 * j)) & 0xffu));
  __syncthreads();
  if (!live) return;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = grp + 4 * i;
    const u32x4 v = *reinterpret_cast<const u32x4*>(my + r * kExpRowB + col * 16);
    uint16_t* dst = out + static_cast<int64_t>(expand_row(rowmap, tile, r, inter)) * out_stride +
                    c * 128 + col * 8;
    *reinterpret_cast<u32x4*>(dst) = v;
  }
}

}  // namespace atta

using namespace atta;

int atta_expand_mxfp4(void* out, const void* codes, const uint8_t* bscale, int N, int K,
                      int64_t out_stride, int rowmap, int dtype, hipStream_t stream) {
  if (out == nullptr || codes == nullptr || bscale == nullptr || N < 16 || N % 16 != 0 ||
      K < 128 || K % 128 != 0 || out_stride < K || out_stride % 8 != 0 || rowmap < 0 ||
      rowmap > 2 || (rowmap == 1 && N % 128 != 0) || (dtype != 0 && dtype != 1))
    return -1;
  const int nch = K / 128;
  const int ncg = (nch + kExpWaves - 1) / kExpWaves;
  const int64_t blocks = static_cast<int64_t>(N / 16) * ncg;
  if (blocks > 0x7fffffff) return -1;
  const dim3 grid(static_cast<unsigned>(blocks)), blk(kExpWaves * 64);
  uint8_t const* c8 = static_cast<const uint8_t*>(codes);
  if (dtype == 0)
    expand_mxfp4_kernel<__bf16><<<grid, blk, 0, stream>>>(static_cast<uint16_t*>(out), c8, bscale,
                                                         nch, ncg, out_stride, rowmap, N / 2);
  else
    expand_mxfp4_kernel<_Float16><<<grid, blk, 0, stream>>>(static_cast<uint16_t*>(out), c8, bscale,
                                                           nch, ncg, out_stride, rowmap, N / 2);
  return static_cast<int>(hipGetLastError());
}
