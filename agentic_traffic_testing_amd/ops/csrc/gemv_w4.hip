// MXFP4 builds of the skinny (decode) GEMV (skinny_w4.h), in a translation unit of their own:
// {bf16, fp16} x {nt, cached} x {1, 2 row tiles} x {4, 8, 16 waves} x the PLAIN / RESADD /
// QKVROPE / SILU epilogues.  gemv.hip routes to atta_w4_launch (route(): the fourth layout).
#include "common.h"
#include "kernels.h"
#include "skinny_w4.h"

namespace atta {

template <typename T, int WAVES, int UNROLL, int MT, int EPI, bool NTL>
__global__ __launch_bounds__(WAVES * 64) void skinny_w4_kernel(SkinnyParams p) {
  unsigned long long t0 = 0;
  if (p.wg_trace != nullptr) t0 = wall_clock64();
  const int tile = blockIdx.x, ks = blockIdx.y;
  skinny_w4_body<T, WAVES, UNROLL, MT, EPI, NTL>(p, tile, ks, p.ksplit);
  if (p.wg_trace != nullptr && ks == 0) {  // timeline probe, as skinny_kernel's
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
      p.wg_trace[2 * tile] = t0;
      p.wg_trace[2 * tile + 1] = wall_clock64();
    }
  }
}

// Two 128-wide loads per register stage and two stages: 64 B of codes per lane in flight, what
// the pre-shuffled 16-bit builds keep (8 waves x 4-deep stages of 16 B).
constexpr int kW4Unroll = 2;

template <int WAVES, int MT, int EPI>
static void launch_w4_t(int dtype, bool nt, dim3 grid, hipStream_t st, const SkinnyParams& p) {
  const dim3 block(WAVES * 64);
  if (dtype == 0) {
    if (nt) skinny_w4_kernel<__bf16, WAVES, kW4Unroll, MT, EPI, true><<<grid, block, 0, st>>>(p);
    else skinny_w4_kernel<__bf16, WAVES, kW4Unroll, MT, EPI, false><<<grid, block, 0, st>>>(p);
  } else {
    if (nt) skinny_w4_kernel<_Float16, WAVES, kW4Unroll, MT, EPI, true><<<grid, block, 0, st>>>(p);
    else skinny_w4_kernel<_Float16, WAVES, kW4Unroll, MT, EPI, false><<<grid, block, 0, st>>>(p);
  }
}

template <int EPI>
static void launch_w4_epi(int dtype, bool nt, int mt, int waves, dim3 grid, hipStream_t st,
                          const SkinnyParams& p) {
  if (waves == 16) {
    if (mt == 1) launch_w4_t<16, 1, EPI>(dtype, nt, grid, st, p);
    else launch_w4_t<16, 2, EPI>(dtype, nt, grid, st, p);
  } else if (waves == 8) {
    if (mt == 1) launch_w4_t<8, 1, EPI>(dtype, nt, grid, st, p);
    else launch_w4_t<8, 2, EPI>(dtype, nt, grid, st, p);
  } else {
    if (mt == 1) launch_w4_t<4, 1, EPI>(dtype, nt, grid, st, p);
    else launch_w4_t<4, 2, EPI>(dtype, nt, grid, st, p);
  }
}

}  // namespace atta

using namespace atta;

// The MXFP4 16-row-tile GEMV for filled params (p.w codes, p.bscale block scales, p.wg_trace
// set by the caller).  K in whole 128-wide loads; the split is halved until a slice is whole
// loads, the waves until every wave of a slice could have one (the loads need not divide
// evenly among them).  Returns 0, -1 (unsupported) or -2 (split without a workspace for it).
int atta_w4_launch(SkinnyParams& p, int epi, int tiles, int waves, int ksplit, int dtype, bool nt,
                   float* sk_ws, int* sk_counters, int64_t ws_floats, int n_counters,
                   hipStream_t stream) {
  if (p.bscale == nullptr || p.w == nullptr || p.M < 1 || p.M > kSkinnyMaxM || p.K < 128 ||
      p.K % 128 != 0 || tiles < 1 || (dtype != 0 && dtype != 1))
    return -1;
  const int chunks = p.K / 128;
  if (ksplit < 1) ksplit = 1;
  while (ksplit > 1 && chunks % ksplit != 0) ksplit >>= 1;
  if (waves != 4 && waves != 8 && waves != 16) waves = 8;
  while (waves > 4 && chunks / ksplit < waves) waves >>= 1;
  p.ksplit = ksplit;
  if (ksplit > 1) {
    const int64_t slot = static_cast<int64_t>(p.M <= 16 ? 16 : kSkinnyMaxM) * 17;
    if (sk_ws == nullptr || sk_counters == nullptr || tiles > n_counters ||
        static_cast<int64_t>(tiles) * ksplit * slot > ws_floats)
      return -2;
    p.sk_ws = sk_ws;
    p.sk_counters = sk_counters;
  }
  const dim3 grid(tiles, ksplit);
  const int mt = p.M <= 16 ? 1 : 2;
  switch (epi) {
    case EPI_PLAIN: launch_w4_epi<EPI_PLAIN>(dtype, nt, mt, waves, grid, stream, p); break;
    case EPI_RESADD: launch_w4_epi<EPI_RESADD>(dtype, nt, mt, waves, grid, stream, p); break;
    case EPI_QKVROPE: launch_w4_epi<EPI_QKVROPE>(dtype, nt, mt, waves, grid, stream, p); break;
    case EPI_SILU: launch_w4_epi<EPI_SILU>(dtype, nt, mt, waves, grid, stream, p); break;
    default: return -1;
  }
  return static_cast<int>(hipGetLastError());
}
