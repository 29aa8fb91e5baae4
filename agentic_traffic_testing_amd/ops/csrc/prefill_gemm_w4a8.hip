// MXFP4 W4A8 prefill GEMM for CDNA4 (gfx950), ops.gemm_w4a8:
//   y[m, n] = xs[m] * sum_k e4m3(xq[m, k]) * e2m1(code[n, k]) * 2^(scale[n, k / 32] - 127)
// fp32 accumulation, one rounding to bf16.  The weights are the resident 4-bit copy exactly as
// ops.preshuffle_mxfp4 lays it out (skinny_w4.h): no second copy, no expansion to 16 bits.
//
// MFMA: v_mfma_scale_f32_32x32x64_f8f6f4, A = weights (format 4 = e2m1, the lane's 32 codes in
// the first four operand dwords, the lane's e8m0 block scale in byte 0 of the scale operand),
// B = activations (format 0 = e4m3, scale byte 127 = 2^0).  Lane maps, settled with exact data
// (tests/test_w4a8_gpu.py::test_layout_probe): lane (r = lane & 31, h = lane >> 5) of the e2m1
// operand holds row r, k = 32 h + 0..31 of the instruction's 64 - one MX block, its scale the
// lane's; the same lane of the e4m3 operand holds row r, k = 16 h + 0..15 in dwords 0-3 and
// k = 32 + 16 h + 0..15 in dwords 4-7 - NOT 32 consecutive k: each half of its 32 bytes meets
// one half of a different e2m1 lane's block.
//
// Fragment gather.  In the resident layout the 32-k block j of row r of a 16-row tile and
// 128-wide K chunk is four dwords at byte (16 g + r) * 16 + 4 j, g = 0..3 (k = 32 j + 8 g + i,
// code i in bits 4 i..): a 256-B stride, k ascending in g.  Which block a lane takes in which of
// a chunk's two MFMA steps is free as long as both operands agree, so lane half h takes blocks
// 2 h + s in step s: its four 8-byte loads (dwords 2 h, 2 h + 1 at every g) hold both steps'
// codes, straight from global memory into the operand registers - every byte of the 1 KiB is
// loaded once, by the one wave that owns the rows.  The scale dword of the row (byte j = block
// j) is shifted so that byte 0 is block 2 h + s.  The activation fragment of step s follows the
// e4m3 lane map: 16 bytes at k = 128 c + 32 s + 16 h (block s, against e2m1 lane half 0) and 16
// bytes at k = 128 c + 64 + 32 s + 16 h (block 2 + s, lane half 1).
//
// Tile: 4 waves, each 32 weight rows x 64 activation rows (two accumulator fragments), so a
// workgroup covers 128 weight rows x 64 rows.  The activations of a chunk (64 x 128 B) are
// shared by the four waves through LDS (two buffers, rows padded to 144 B, filled from
// registers loaded one chunk ahead; one barrier per chunk); weights and scales of the next
// chunk are loaded into registers before the current chunk's MFMAs.  Workgroups of one weight
// stripe are adjacent in the grid (M fastest), so the stripe is read from HBM once and then
// from L2.  Data-parallel tiles only: no cross-workgroup wait, no K split.
//
// What bounds a tile: per chunk a wave issues 4 MFMAs for 2 KiB of codes and 8 KiB of shared
// activations, and nothing but other waves hides its loads: 18 KiB of LDS and 120 VGPRs let
// four workgroups share a CU.  A 128-row build (half the L2 bytes per MFMA, 196 VGPRs, two
// workgroups per CU) lost to this one by 5-20 % at every 8B shape from 160 to 3070 rows
// (docs/kernels.md "MXFP4 W4A8 prefill") and is not built; 64 rows also keep the padding of a
// 129-640-row step small.  The template keeps the height a parameter (MI fragments).
//
// Epilogues: PLAIN stores y[:, r] with r the ORIGINAL weight row (the qkv / silu tile row maps
// undone arithmetically: a lane's four accumulator registers 4 q..4 q + 3 are four consecutive
// original rows under every map - one 8-byte store); SILU (silu row map: 8 gate rows and their
// 8 up rows per 16-row tile) multiplies silu(gate) * up lane-locally - registers 4 q.. against
// 4 (q + 1).. for q = 0, 2 - into [M, I].
//
// Shape rule: K % 128 == 0, N % 32 == 0 (qkv map: N % 128 == 0); SILU needs the silu map.  M is
// free: rows past M are clamped on the load side and never stored.
#include "common.h"
#include "kernels.h"

namespace atta {
namespace {

enum { W4A8_PLAIN = 0, W4A8_SILU = 2 };  // ops.GEMM_PLAIN / ops.GEMM_SILU

constexpr int kW4Waves = 4;
constexpr int kW4Threads = kW4Waves * 64;
constexpr int kXRowB = 128 + 16;  // staged activation row: one chunk + one 16-B slot of padding

typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;

struct W4A8Args {
  uint16_t* y;
  const uint8_t* xq;
  const float* xs;
  const uint8_t* codes;
  const uint8_t* bscale;
  int64_t ldx, ldy;
  int M, N;     // N = weight rows
  int nch;      // K / 128
  int mt;       // M tiles
  int rowmap;
};

// original weight row of column c of a 16-row tile under a row map (skinny.h tile_row)
__device__ __forceinline__ int w4a8_row(int rowmap, int tile, int c, int inter) {
  if (rowmap == 1) return (tile >> 3) * 128 + (tile & 7) * 8 + (c & 7) + ((c & 8) ? 64 : 0);
  if (rowmap == 2) return c < 8 ? tile * 8 + c : inter + tile * 8 + c - 8;
  return tile * 16 + c;
}

__device__ __forceinline__ float w4a8_silu(float g) { return g / (1.f + __expf(-g)); }

template <int MODE, int MI>
__global__ __launch_bounds__(kW4Threads) void gemm_w4a8_kernel(W4A8Args p) {
  constexpr int BM = MI * 32;
  __shared__ __attribute__((aligned(16))) unsigned char xl[2][BM * kXRowB];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int tm = blockIdx.x % p.mt, tn = blockIdx.x / p.mt;
  const int frag = tn * kW4Waves + wid;   // this wave's 32 weight rows
  const bool live = frag < p.N / 32;      // wave-uniform; a dead wave only stages activations
  const int nch = p.nch;

  // weights: the lane's 8 bytes at every g of (tile, chunk); scales: the row's dword
  const int tile = (live ? frag : 0) * 2 + (r >> 4);
  const uint8_t* wp = p.codes + static_cast<int64_t>(tile) * nch * 1024 + (r & 15) * 16 + h * 8;
  const uint8_t* sp = p.bscale + static_cast<int64_t>(tile) * nch * 64 + (r & 15) * 4;
  // activation staging: thread t moves 16 B of row (t >> 3) + 32 i, segment t & 7
  const uint8_t* xp[MI];
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const int m = min(tm * BM + i * 32 + (tid >> 3), p.M - 1);
    xp[i] = p.xq + static_cast<int64_t>(m) * p.ldx + (tid & 7) * 16;
  }
  const int x_wr = (tid >> 3) * kXRowB + (tid & 7) * 16;
  const int x_rd = r * kXRowB + h * 16;

  f32x16 acc[MI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;

  u32x4 xr[MI];
  u32x2 w[4], wn[4];
  uint32_t s = 0, sn = 0;
#pragma unroll
  for (int g = 0; g < 4; ++g) w[g] = wn[g] = u32x2{0u, 0u};
#pragma unroll
  for (int i = 0; i < MI; ++i) xr[i] = *reinterpret_cast<const u32x4*>(xp[i]);
  if (live) {
#pragma unroll
    for (int g = 0; g < 4; ++g) w[g] = *reinterpret_cast<const u32x2*>(wp + g * 256);
    s = *reinterpret_cast<const uint32_t*>(sp);
  }

  for (int c = 0; c < nch; ++c) {
    unsigned char* buf = xl[c & 1];
#pragma unroll
    for (int i = 0; i < MI; ++i)
      *reinterpret_cast<u32x4*>(buf + i * 32 * kXRowB + x_wr) = xr[i];
    // one barrier per chunk: buffer c & 1 is next written in chunk c + 2, after every wave has
    // passed the barrier of chunk c + 1, i.e. finished reading it in chunk c
    __syncthreads();
    if (c + 1 < nch) {
#pragma unroll
      for (int i = 0; i < MI; ++i)
        xr[i] = *reinterpret_cast<const u32x4*>(xp[i] + static_cast<int64_t>(c + 1) * 128);
      if (live) {
#pragma unroll
        for (int g = 0; g < 4; ++g)
          wn[g] = *reinterpret_cast<const u32x2*>(wp + static_cast<int64_t>(c + 1) * 1024 + g * 256);
        sn = *reinterpret_cast<const uint32_t*>(sp + static_cast<int64_t>(c + 1) * 64);
      }
    }
    if (live) {
#pragma unroll
      for (int st = 0; st < 2; ++st) {
        const i32x8 a = {static_cast<int>(w[0][st]), static_cast<int>(w[1][st]),
                         static_cast<int>(w[2][st]), static_cast<int>(w[3][st]), 0, 0, 0, 0};
        const int sa = static_cast<int>((s >> (16 * h + 8 * st)) & 0xffu);
#pragma unroll
        for (int i = 0; i < MI; ++i) {
          const unsigned char* src = buf + i * 32 * kXRowB + x_rd + st * 32;
          const u32x4 lo = *reinterpret_cast<const u32x4*>(src);
          const u32x4 hi = *reinterpret_cast<const u32x4*>(src + 64);
          const i32x8 b =
              __builtin_bit_cast(i32x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
          acc[i] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, acc[i], 4, 0, 0, sa, 0,
                                                                   127);
        }
      }
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) w[g] = wn[g];
    s = sn;
  }
  if (!live) return;

  // lane holds activation row m = i * 32 + r and weight rows 8 q + 4 h + j of the fragment in
  // register 4 q + j: tile 2 frag + (q >> 1), tile column 8 (q & 1) + 4 h + j
  const int inter = p.N / 2;
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const int m = tm * BM + i * 32 + r;
    if (m >= p.M) continue;
    const float xsc = p.xs[m];
    uint16_t* yrow = p.y + static_cast<int64_t>(m) * p.ldy;
    if constexpr (MODE == W4A8_SILU) {
#pragma unroll
      for (int q = 0; q < 4; q += 2) {
        Pack4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          o.v[j] = from_f32<__bf16>(w4a8_silu(acc[i][4 * q + j] * xsc) *
                                    (acc[i][4 * q + 4 + j] * xsc));
        *reinterpret_cast<Pack4*>(yrow + (frag * 2 + (q >> 1)) * 8 + 4 * h) = o;
      }
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        Pack4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o.v[j] = from_f32<__bf16>(acc[i][4 * q + j] * xsc);
        const int n0 = w4a8_row(p.rowmap, frag * 2 + (q >> 1), 8 * (q & 1) + 4 * h, inter);
        *reinterpret_cast<Pack4*>(yrow + n0) = o;
      }
    }
  }
}

constexpr int kW4MI = 2;  // tile height / 32

}  // namespace
}  // namespace atta

using namespace atta;

// mode 0: y [M, N] bf16, columns in original weight-row order; mode 2 (rowmap 2 only):
// y [M, N / 2] = silu(gate) * up.
int atta_gemm_w4a8(void* y, const void* xq, const float* xs, const void* codes,
                   const uint8_t* bscale, int M, int N, int K, int64_t ldx, int64_t ldy,
                   int rowmap, int mode, hipStream_t stream) {
  if (y == nullptr || xq == nullptr || xs == nullptr || codes == nullptr || bscale == nullptr ||
      M <= 0 || N < 32 || N % 32 != 0 || K < 128 || K % 128 != 0 || rowmap < 0 || rowmap > 2 ||
      (rowmap == 1 && N % 128 != 0) || (mode != W4A8_PLAIN && mode != W4A8_SILU) ||
      (mode == W4A8_SILU && rowmap != 2) || ldx < K || ldx % 16 != 0 ||
      ldy < (mode == W4A8_SILU ? N / 2 : N) || ldy % 4 != 0)
    return -1;
  constexpr int bm = kW4MI * 32;
  W4A8Args p;
  p.y = static_cast<uint16_t*>(y);
  p.xq = static_cast<const uint8_t*>(xq);
  p.xs = xs;
  p.codes = static_cast<const uint8_t*>(codes);
  p.bscale = bscale;
  p.ldx = ldx;
  p.ldy = ldy;
  p.M = M;
  p.N = N;
  p.nch = K / 128;
  p.mt = (M + bm - 1) / bm;
  p.rowmap = rowmap;
  const int64_t blocks = static_cast<int64_t>(p.mt) * ((N / 32 + kW4Waves - 1) / kW4Waves);
  if (blocks > 0x7fffffff) return -1;
  const dim3 grid(static_cast<unsigned>(blocks));
  if (mode == W4A8_SILU)
    hipLaunchKernelGGL((gemm_w4a8_kernel<W4A8_SILU, kW4MI>), grid, dim3(kW4Threads), 0, stream, p);
  else
    hipLaunchKernelGGL((gemm_w4a8_kernel<W4A8_PLAIN, kW4MI>), grid, dim3(kW4Threads), 0, stream, p);
  return static_cast<int>(hipGetLastError());
}
