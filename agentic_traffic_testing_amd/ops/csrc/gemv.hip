// Skinny (decode) GEMM on MFMA with fused prologue/epilogues.
//
//   acc[M, 16-col tile] = x[M, K] . W[rows(tile), K]^T          (M <= 32, W streamed once)
//
// Decode steps of the 8B model stream ~15 GB of weights per token while M (= sequences in
// the batch) is 1..16, so the layer GEMMs are pure HBM streams (guide: "GEMV / M <= 16
// decode weights: load straight to VGPRs, deep unroll, late vmcnt").  Structure:
//   * a workgroup owns one 16-column output tile; WAVES waves split K; each wave streams
//     its K slice of the tile's 16 weight rows with 16-byte loads through two register
//     stages.  One row tile of 16-bit weights (every decode step): a stage holds UNROLL
//     weight loads AND the UNROLL x fragments they meet, issued together one stage ahead of
//     use with no load under a branch, so the MFMAs of stage s wait with vmcnt(loads of
//     stage s + 1) and the next stage stays in flight across them (skinny.h, PIPE).  Two
//     row tiles and fp8 weights keep the older order - next stage's weights, then this
//     stage's x under an exec mask, then vmcnt(0) - which drains the queue every stage but
//     needs fewer registers (profiles/r7_gemv_pipeline_isa.txt);
//   * the 16 rows x 32 k chunk is the B operand of mfma_f32_16x16x32_bf16 (lane l: weight
//     row rows(tile, l&15), k = 8(l>>4)..+8); x rows are the A operand (lane l: row l&15,
//     L1/L2 resident; rows >= M are zeros);
//   * `rows(tile, c)` is an epilogue-defined row map, so the epilogue can see partner
//     columns without any weight permutation: RoPE pairs (d, d+64) and SwiGLU pairs
//     (gate_j, up_j) land in the same tile;
//   * RMSNorm fusion: with the norm weight folded into W on the host, the kernel only needs
//     sum(x^2) per row, accumulated from the x fragments it already loads for the MFMAs;
//     the epilogue scales by rsqrt(mean + eps);
//   * wave partials + row sums are reduced through LDS; epilogues:
//       PLAIN   y = acc                      RESADD  r += acc (residual stream, in place)
//       QKVROPE q/k rotated (RoPE) -> q buffer / paged K cache, v -> transposed V cache
//       SILU    out[:, j] = silu(gate_j) * up_j
//       SAMPLE  logits -> greedy / Gumbel-max key -> one partial max per (row, tile)
//               (sampler fused into the LM head; `sample_finalize` reduces a row's
//               partials to its token id with one workgroup per row)
#include <cstdlib>
#include <type_traits>

#include "common.h"
#include "kernels.h"
#include "skinny.h"

namespace atta {

template <typename T, int WAVES, int UNROLL, int MT, int EPI, bool NTL = false, bool PS = false,
          bool W8 = false>
__global__ __launch_bounds__(WAVES * 64) void skinny_kernel(SkinnyParams p) {
  unsigned long long t0 = 0;
  if (p.wg_trace != nullptr) t0 = wall_clock64();
  const int tile = blockIdx.x, ks = blockIdx.y;
  skinny_body<T, WAVES, UNROLL, MT, EPI, NTL, PS, W8>(p, tile, ks, p.ksplit);
  if (p.wg_trace != nullptr && ks == 0) {  // timeline probe (one entry per tile, bounded by
    // the tile count whatever the split): every thread's stores issued, then one stamp
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
      p.wg_trace[2 * tile] = t0;
      p.wg_trace[2 * tile + 1] = wall_clock64();
    }
  }
}


// Weight-stream cache policy.  Non-temporal (nt) weight loads: every decode weight byte is
// read once per step by one CU, so keeping it out of the caches helps - but only with the
// pre-shuffled layout (one contiguous 1 KiB per wave instruction): there nt lifted the
// fan-out bench from 703 to 756 tok/s (profiles/bench_r1_v10_nt.log).  On the row-major
// layout (16 rows x 64 B per instruction) nt made every GEMV slower (gate_up 42 -> 48 us,
// profiles/bench_r1_ab_nt.log), so it stays off there.  ATTA_NT_WEIGHTS=0 disables it for
// A/B runs, =1 forces it on for row-major weights too.
static int nt_weights() {
  static const int mode = [] {
    const char* e = std::getenv("ATTA_NT_WEIGHTS");
    return e == nullptr ? -1 : (e[0] == '1' ? 1 : 0);  // -1 = default policy per layout
  }();
  return mode;
}

template <int WAVES, int UNROLL, int MT, int EPI>
static void launch_t(int dtype, dim3 grid, hipStream_t st, const SkinnyParams& p) {
  const int mode = nt_weights();
  const bool w8 = p.wscale != nullptr, ps = p.ps || w8;
  const bool nt = ps ? mode != 0 : mode == 1;
  // runtime (dtype, nt, layout) -> template arguments: {bf16, fp16} x {nt, cached} x
  // {row-major, pre-shuffled, fp8}.  fp8 weights are pre-shuffled by construction and a
  // 16-byte lane load carries two K steps, so their stage is twice as deep to keep the same
  // bytes in flight per wave.  (Twice that again - a wave's whole K slice in flight in its
  // first two stages - measured slower in situ: fp8 bench 986 vs 1022 tok/s,
  // profiles/r2_ab_fp8_stage_depth.txt.)
  auto launch = [&](auto t, auto nt_, auto ps_, auto w8_) {
    constexpr bool W8 = decltype(w8_)::value;
    skinny_kernel<decltype(t), WAVES, W8 ? UNROLL * 2 : UNROLL, MT, EPI, decltype(nt_)::value,
                  decltype(ps_)::value, W8><<<grid, dim3(WAVES * 64), 0, st>>>(p);
  };
  constexpr std::true_type yes{};
  constexpr std::false_type no{};
  auto by_layout = [&](auto t, auto nt_) {
    if (w8) {
      // (no fp8 build of the logprob sampler and scorer epilogues: route() sends none here)
      if constexpr (!epi_records(EPI)) launch(t, nt_, yes, yes);
    } else if (ps) launch(t, nt_, yes, no);
    else launch(t, nt_, no, no);
  };
  auto by_nt = [&](auto t) {
    if (nt) by_layout(t, yes);
    else by_layout(t, no);
  };
  if (dtype == 0) by_nt(__bf16{});
  else by_nt(_Float16{});
}

template <int EPI>
static void launch_epi(int dtype, int mt, int waves, dim3 grid, hipStream_t st,
                       const SkinnyParams& p) {
  // (waves, unroll) picked from cold-cache on-device sweeps (profiles/r1_microbench_*):
  // row-major 16-bit weights: 8 x 2 for the small projections, 16 x 2 for the large ones;
  // pre-shuffled 16-bit weights: 8 waves stream best with 4-deep stages (o, down), 16 x 2
  // (gate_up, lm_head), 4 x 4 (qkv).  fp8 doubles the depth inside launch_t.  Re-swept on the
  // pipelined loop (waves {4, 8, 16} x unroll {2, 4, 8}, profiles/r7_gemv_pipeline_ab.txt):
  // 8-deep stages never win, the rest lie within 5 % of these picks cold and no other wave
  // count won in situ, so the table stands.
  const bool ps16 = p.ps && p.wscale == nullptr;
  if (waves == 16) {
    if (mt == 1) launch_t<16, 2, 1, EPI>(dtype, grid, st, p);
    else launch_t<16, 2, 2, EPI>(dtype, grid, st, p);
  } else if (waves == 8 && ps16) {
    if (mt == 1) launch_t<8, 4, 1, EPI>(dtype, grid, st, p);
    else launch_t<8, 4, 2, EPI>(dtype, grid, st, p);
  } else if (waves == 8) {
    if (mt == 1) launch_t<8, 2, 1, EPI>(dtype, grid, st, p);
    else launch_t<8, 2, 2, EPI>(dtype, grid, st, p);
  } else {
    if (mt == 1) launch_t<4, 4, 1, EPI>(dtype, grid, st, p);
    else launch_t<4, 4, 2, EPI>(dtype, grid, st, p);
  }
}

// Largest supported wave count <= requested that divides K into 32-wide MFMA steps.
// (fp8 weights stream 64-wide K-step pairs: granule 64, and 128 per wave at 4 waves.)
static int fit_waves(int waves, int K, bool fp8 = false) {
  if (waves != 4 && waves != 8 && waves != 16) waves = 8;
  const int gran = fp8 ? 64 : 32;
  while (waves > 4 && K % (gran * waves) != 0) waves >>= 1;
  return waves;
}

// One workgroup per row reduces the row's per-tile partial keys to the winning token.
// 1024 threads x 8 independent loads in flight cover the 8016 partials of a 128256 vocab
// in one memory round trip.
// KEY_OUT writes the row's packed key with the sign bit flipped (signed-int64 orderable) so
// TP ranks can combine their vocab shards with one int64 MAX all-reduce.
constexpr int kFinThreads = 1024;
template <bool KEY_OUT>
__global__ void __launch_bounds__(kFinThreads) sample_finalize_kernel(
    int64_t* out, const unsigned long long* keys, int n_tiles) {
  __shared__ unsigned long long red[kFinThreads / kWave];
  const int m = blockIdx.x;
  const unsigned long long* row = keys + static_cast<int64_t>(m) * n_tiles;
  unsigned long long best = 0ull;
  for (int base = 0; base < n_tiles; base += 8 * kFinThreads) {
    unsigned long long k[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int i = base + j * kFinThreads + threadIdx.x;
      k[j] = i < n_tiles ? row[i] : 0ull;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) best = k[j] > best ? k[j] : best;
  }
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const unsigned long long other = __shfl_xor(best, o, kWave);
    best = other > best ? other : best;
  }
  if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = best;
  __syncthreads();
  if (threadIdx.x < kWave) {
    best = threadIdx.x < kFinThreads / kWave ? red[threadIdx.x] : 0ull;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
      const unsigned long long other = __shfl_xor(best, o, kWave);
      best = other > best ? other : best;
    }
    if (threadIdx.x == 0) {
      if constexpr (KEY_OUT)
        out[m] = static_cast<int64_t>(best ^ 0x8000000000000000ull);
      else
        out[m] = static_cast<int64_t>(0xFFFFFFFFu - static_cast<unsigned>(best & 0xFFFFFFFFull));
    }
  }
}

// (max, sum exp(l - max)) of two sets of logits -> of their union.  An empty set is
// (-inf, 0): the guard keeps exp(-inf - -inf) out.
__device__ __forceinline__ void lse_merge(float& m, float& s, float om, float os) {
  const float nm = fmaxf(m, om);
  if (nm > -__builtin_huge_valf()) s = s * __expf(m - nm) + os * __expf(om - nm);
  m = nm;
}

// sample_finalize_kernel for the SAMPLE_LP epilogue: the same key reduction to the row's token
// (same load shape: 1024 threads x 8 loads cover 8192 tiles per trip), and the row's logprob
// from the per-tile records rec[m][tile] = {max_i, s_i, raw logit of the tile's winner}:
//   logZ = gmax + log(sum_i s_i exp(max_i - gmax)),   lp[m] = l_win - logZ
// with l_win read from the winning tile's record.  ids in the keys are global: vocab_offset is
// the id of column 0.
__global__ void __launch_bounds__(kFinThreads) sample_lp_finalize_kernel(
    int64_t* out, float* lp, const unsigned long long* keys, const f32x4* rec, int n_tiles,
    int vocab_offset) {
  __shared__ unsigned long long red[kFinThreads / kWave];
  __shared__ float rm[kFinThreads / kWave], rs[kFinThreads / kWave];
  const int m = blockIdx.x;
  const unsigned long long* row = keys + static_cast<int64_t>(m) * n_tiles;
  const f32x4* rrow = rec + static_cast<int64_t>(m) * n_tiles;
  unsigned long long best = 0ull;
  float gm = -__builtin_huge_valf(), gs = 0.f;
  for (int base = 0; base < n_tiles; base += 8 * kFinThreads) {
    unsigned long long k[8];
    f32x4 r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int i = base + j * kFinThreads + threadIdx.x;
      k[j] = i < n_tiles ? row[i] : 0ull;
      r[j] = i < n_tiles ? rrow[i] : f32x4{-__builtin_huge_valf(), 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      best = k[j] > best ? k[j] : best;
      lse_merge(gm, gs, r[j][0], r[j][1]);
    }
  }
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const unsigned long long other = __shfl_xor(best, o, kWave);
    best = other > best ? other : best;
    const float om = __shfl_xor(gm, o, kWave), os = __shfl_xor(gs, o, kWave);
    lse_merge(gm, gs, om, os);
  }
  if ((threadIdx.x & (kWave - 1)) == 0) {
    red[threadIdx.x / kWave] = best;
    rm[threadIdx.x / kWave] = gm;
    rs[threadIdx.x / kWave] = gs;
  }
  __syncthreads();
  if (threadIdx.x < kWave) {
    const bool has = threadIdx.x < kFinThreads / kWave;
    best = has ? red[threadIdx.x] : 0ull;
    gm = has ? rm[threadIdx.x] : -__builtin_huge_valf();
    gs = has ? rs[threadIdx.x] : 0.f;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
      const unsigned long long other = __shfl_xor(best, o, kWave);
      best = other > best ? other : best;
      const float om = __shfl_xor(gm, o, kWave), os = __shfl_xor(gs, o, kWave);
      lse_merge(gm, gs, om, os);
    }
    if (threadIdx.x == 0) {
      const int id = static_cast<int>(0xFFFFFFFFu - static_cast<unsigned>(best & 0xFFFFFFFFull));
      out[m] = id;
      // the winner's tile; clamped so that keys no launch wrote can never index past the row
      const int tile = min(max((id - vocab_offset) >> 4, 0), n_tiles - 1);
      lp[m] = rrow[tile][2] - (gm + logf(gs));
    }
  }
}

// The SCORE epilogue's finalize, one workgroup per row: sample_lp_finalize_kernel's load shape
// and lse_merge tree over the records rec[m][tile] = {max_i, s_i, target's raw logit or 0},
// without the keys:  lp[m] = rec[m][target >> 4].z - (gmax + log(sum_i s_i exp(max_i - gmax))).
__global__ void __launch_bounds__(kFinThreads) score_finalize_kernel(
    float* lp, const int* targets, const f32x4* rec, int n_tiles, int vocab_offset) {
  __shared__ float rm[kFinThreads / kWave], rs[kFinThreads / kWave];
  const int m = blockIdx.x;
  const f32x4* rrow = rec + static_cast<int64_t>(m) * n_tiles;
  float gm = -__builtin_huge_valf(), gs = 0.f;
  for (int base = 0; base < n_tiles; base += 8 * kFinThreads) {
    f32x4 r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int i = base + j * kFinThreads + threadIdx.x;
      r[j] = i < n_tiles ? rrow[i] : f32x4{-__builtin_huge_valf(), 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) lse_merge(gm, gs, r[j][0], r[j][1]);
  }
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const float om = __shfl_xor(gm, o, kWave), os = __shfl_xor(gs, o, kWave);
    lse_merge(gm, gs, om, os);
  }
  if ((threadIdx.x & (kWave - 1)) == 0) {
    rm[threadIdx.x / kWave] = gm;
    rs[threadIdx.x / kWave] = gs;
  }
  __syncthreads();
  if (threadIdx.x < kWave) {
    const bool has = threadIdx.x < kFinThreads / kWave;
    gm = has ? rm[threadIdx.x] : -__builtin_huge_valf();
    gs = has ? rs[threadIdx.x] : 0.f;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
      const float om = __shfl_xor(gm, o, kWave), os = __shfl_xor(gs, o, kWave);
      lse_merge(gm, gs, om, os);
    }
    if (threadIdx.x == 0) {
      // the target's tile; clamped so that a bad id can never index past the row
      const int tile = min(max((targets[m] - vocab_offset) >> 4, 0), n_tiles - 1);
      lp[m] = rrow[tile][2] - (gm + logf(gs));
    }
  }
}
}  // namespace atta

using namespace atta;
// Timeline probe for the NEXT skinny launch only (nullptr: off); see SkinnyParams.wg_trace
static unsigned long long* g_gemv_trace = nullptr;
void atta_set_gemv_trace(void* trace) { g_gemv_trace = static_cast<unsigned long long*>(trace); }
static unsigned long long* take_trace() {
  unsigned long long* t = g_gemv_trace;
  g_gemv_trace = nullptr;
  return t;
}

// The wide small-M kernel (wide.hip): its (waves, split) plan is automatic unless overridden
// for the NEXT such launch by atta_set_wide_plan (tuning sweeps).
int atta_wide_launch(SkinnyParams& p, int epi, int ntiles, int waves, int ksplit, int dtype,
                     const float* sk_ws, int* sk_counters, int64_t ws_floats, int n_counters,
                     hipStream_t stream);
static int g_wide_waves = 0, g_wide_ksplit = 0;
void atta_set_wide_plan(int waves, int ksplit) {
  g_wide_waves = waves;
  g_wide_ksplit = ksplit;
}
// Pre-shuffled 16-bit calls run the wide kernel from g_wide_min_m rows (gate_up + SiLU:
// g_wide_min_m_silu), see route().  At 17-32 rows the 16-row-tile
// GEMVs re-read x per weight tile in two row blocks (per layer 120-137 us vs 95-98 us wide);
// at 12-16 rows only gate_up gains (43.3 / 48.2 -> 39.3 / 39.1 us); at <= 8 rows (decode)
// the GEMVs win every projection (profiles/r5_wide_vs_skinny.txt)
static int g_wide_min_m = 17, g_wide_min_m_silu = 12;
void atta_set_wide_min_rows(int m, int m_silu) {
  g_wide_min_m = m < 1 ? 1 : m;
  g_wide_min_m_silu = m_silu < 1 ? 1 : m_silu;
}
void atta_get_wide_min_rows(int* m, int* m_silu) {
  *m = g_wide_min_m;
  *m_silu = g_wide_min_m_silu;
}

// Which kernel runs M rows of a weight layout with an epilogue - the one routing table of
// the library (ops.fused_kernel is the same table under the Python-side row policy).
// min = g_wide_min_m (17), for EPI_SILU g_wide_min_m_silu (12):
//
//   weights               epilogue          rows               kernel
//   any                   any               M < 1              None
//   row-major 16-bit      any               1 - 32             Skinny
//   row-major 16-bit      any               > 32               None
//   pre-shuffled 16-bit   any               1 .. min - 1       Skinny
//   pre-shuffled 16-bit   any               min .. 128         Wide
//   pre-shuffled 16-bit   any but SAMPLE    129 .. kMidmMaxM   MidM
//   fp8 (pre-shuffled)    any but SAMPLE    1 - 32             Skinny
//   fp8                   any but SAMPLE    33 - 128           Wide
//   fp8                   any but SAMPLE    129 .. kMidmMaxM   MidM
//   any                   SAMPLE            > 128              None   (no sampler epilogue in
//   fp8                   SAMPLE            > 32               None    those builds)
//   any                   the push variant  1 - 32             Skinny (routes as row-major:
//   any                   the push variant  > 32               None    the GEMV alone pushes)
//   MXFP4 (pre-shuffled)  any but SAMPLE    1 - 32             Skinny (its W4 build,
//   MXFP4                 any but SAMPLE    > 32               None    gemv_w4.hip)
//   MXFP4, wide_w4 chosen any but SAMPLE    33 - 128           Wide   (its W4 builds,
//   MXFP4, wide_w4 chosen any but SAMPLE    > 128              None    wide_w4_mt<N>.hip)
//   MXFP4                 SAMPLE, the push  any                None
// wide_w4: the caller's explicit per-call choice (kWideW4 in the dtype code); a default MXFP4
// call past 32 rows keeps having no kernel.
// SAMPLE_LP (the sampler with the logprob record) routes as SAMPLE does, except that it has no
// fp8 build at any row count: None.  SCORE (the teacher-forced scorer) routes as SAMPLE_LP.
enum class Route { None, Skinny, Wide, MidM };
static Route route(int M, bool ps, bool w8, bool w4, int epi, bool wide_w4 = false) {
  if (M < 1) return Route::None;
  if (w4) {
    if (epi_lm_head(epi)) return Route::None;
    if (M <= kSkinnyMaxM) return Route::Skinny;
    return wide_w4 && M <= kWideMaxM ? Route::Wide : Route::None;
  }
  if (epi_records(epi) && w8) return Route::None;
  if (!ps) return M <= kSkinnyMaxM ? Route::Skinny : Route::None;
  const int wide_min = epi == EPI_SILU ? g_wide_min_m_silu : g_wide_min_m;
  if (M <= kSkinnyMaxM && (w8 || M < wide_min)) return Route::Skinny;
  if (epi_lm_head(epi) && (w8 || M > kWideMaxM)) return Route::None;
  if (M <= kWideMaxM) return Route::Wide;
  return M <= kMidmMaxM ? Route::MidM : Route::None;
}

// Split-K workspace per device (ops.set_splitk_workspace): fp32 partial slots + one arrival
// counter per 16-column tile (zeroed once; the last arriver re-arms it).
struct SplitKWs {
  float* ws = nullptr;
  int* counters = nullptr;
  int64_t ws_floats = 0;
  int n_counters = 0;
};
static SplitKWs g_splitk[64];

int atta_set_splitk_ws(int device, float* ws, int* counters, int64_t ws_floats, int n_counters) {
  if (device < 0 || device >= 64) return -1;
  g_splitk[device] = SplitKWs{ws, counters, ws_floats, n_counters};
  return 0;
}

static const SplitKWs* splitk_ws() {  // the current device's, or nullptr
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
  return &g_splitk[dev];
}

// Resolve the split for one launch: waves fitted to the K slice (fp8: 64-wide granule), the
// split reduced until every wave's slice is whole; a split > 1 needs the device workspace.
// Returns 0 or -1 (unsupported), -2 (split requested but no / too small workspace).
static int setup_split(SkinnyParams& p, int& waves, int ksplit, int tiles, bool fp8) {
  const int gran = fp8 ? 64 : 32;
  if (ksplit < 1) ksplit = 1;
  while (ksplit > 1 && p.K % (ksplit * gran * 4) != 0) ksplit >>= 1;
  waves = fit_waves(waves, p.K / ksplit, fp8);
  if ((p.K / ksplit) % (gran * waves) != 0) return -1;
  p.ksplit = ksplit;
  if (ksplit == 1) return 0;
  const SplitKWs* w = splitk_ws();
  if (w == nullptr) return -2;
  // one slot per (tile, slice): the launch's row blocks (16 or kSkinnyMaxM rows) x 17 floats
  const int64_t slot = static_cast<int64_t>(p.M <= 16 ? 16 : kSkinnyMaxM) * 17;
  if (w->ws == nullptr || tiles > w->n_counters ||
      static_cast<int64_t>(tiles) * ksplit * slot > w->ws_floats)
    return -2;
  p.sk_ws = w->ws;
  p.sk_counters = w->counters;
  return 0;
}

// The 16-row-tile GEMV for filled params: split, grid, pending timeline probe, launch.
template <int EPI>
static int launch_skinny(SkinnyParams& p, int tiles, int waves, int ksplit, int dtype,
                         hipStream_t stream) {
  if (const int rc = setup_split(p, waves, ksplit, tiles, p.wscale != nullptr)) return rc;
  const dim3 grid(tiles, p.ksplit);
  p.wg_trace = take_trace();
  launch_epi<EPI>(dtype, p.M <= 16 ? 1 : 2, waves, grid, stream, p);
  return static_cast<int>(hipGetLastError());
}

// The MXFP4 build of the 16-row-tile GEMV (gemv_w4.hip) for filled params; it fits the
// split and the waves to K itself.
int atta_w4_launch(SkinnyParams& p, int epi, int tiles, int waves, int ksplit, int dtype, bool nt,
                   float* sk_ws, int* sk_counters, int64_t ws_floats, int n_counters,
                   hipStream_t stream);
static int launch_w4(SkinnyParams& p, int epi, int tiles, int waves, int ksplit, int dtype,
                     hipStream_t stream) {
  const SplitKWs* w = splitk_ws();
  const SplitKWs none{};
  if (w == nullptr) w = &none;
  p.wg_trace = take_trace();
  return atta_w4_launch(p, epi, tiles, waves, ksplit, dtype, nt_weights() != 0, w->ws,
                        w->counters, w->ws_floats, w->n_counters, stream);
}

int atta_midm_launch(SkinnyParams& p, int epi, int ntiles, int dtype, float* sk_ws,
                     int64_t ws_floats, hipStream_t stream);
// The wide small-M kernel (wide.hip) for filled params: the next-launch plan override and
// the pending timeline probe are consumed here.
static int launch_wide(SkinnyParams& p, int epi, int tiles, int dtype, hipStream_t stream) {
  const SplitKWs* w = splitk_ws();
  if (w == nullptr) return -2;
  const int waves = g_wide_waves, ksplit = g_wide_ksplit;
  g_wide_waves = g_wide_ksplit = 0;
  p.wg_trace = take_trace();  // 4 stamps per workgroup here (wide.hip)
  return atta_wide_launch(p, epi, tiles, waves, ksplit, dtype, w->ws, w->counters, w->ws_floats,
                          w->n_counters, stream);
}

// The mid-M kernel (midm.hip, row-blocked grid).  It has no timeline probe: a pending one
// stays pending for the next GEMV or wide launch.
static int launch_midm(SkinnyParams& p, int epi, int tiles, int dtype, hipStream_t stream) {
  const SplitKWs* w = splitk_ws();
  if (w == nullptr) return -2;
  p.wg_trace = nullptr;
  return atta_midm_launch(p, epi, tiles, dtype, w->ws, w->ws_floats, stream);
}

// Launch filled params on the kernel route() names; tiles: 16-column weight tiles; waves /
// ksplit: the caller's plan for the 16-row-tile GEMV (the other two plan for themselves).
template <int EPI>
static int launch_routed(SkinnyParams& p, int tiles, int waves, int ksplit, int dtype,
                         hipStream_t stream) {
  if (p.bscale != nullptr && p.wscale != nullptr) return -1;
  const bool wide_w4 = (dtype & kWideW4) != 0;
  dtype &= ~kWideW4;
  switch (route(p.M, p.ps != 0, p.wscale != nullptr, p.bscale != nullptr, EPI, wide_w4)) {
    case Route::Skinny:
      if (p.bscale != nullptr) return launch_w4(p, EPI, tiles, waves, ksplit, dtype, stream);
      return launch_skinny<EPI>(p, tiles, waves, ksplit, dtype, stream);
    case Route::Wide: return launch_wide(p, EPI, tiles, dtype, stream);
    case Route::MidM: return launch_midm(p, EPI, tiles, dtype, stream);
    case Route::None: break;
  }
  return -1;
}

// The fields every entry point fills the same way.
static SkinnyParams base_params(const void* x, const void* w, int M, int N, int K,
                                int64_t x_stride, float eps, int ps, const float* wscale,
                                const uint8_t* bscale = nullptr) {
  SkinnyParams p{};
  p.x = static_cast<const uint16_t*>(x);
  p.w = static_cast<const uint16_t*>(w);
  p.M = M;
  p.N = N;
  p.K = K;
  p.x_stride = x_stride;
  p.eps = eps;
  p.ps = ps;
  p.wscale = wscale;
  p.bscale = bscale;
  return p;
}

int atta_skinny_gemm(void* y, const void* x, const void* w, const void* residual, int M, int N,
                     int K, int64_t x_stride, int64_t y_stride, int64_t res_stride, int waves,
                     int ksplit, const float* wscale, const uint8_t* bscale, int dtype,
                     hipStream_t stream) {
  const int ps = (dtype & kPreshuffled) ? 1 : 0;
  dtype &= ~kPreshuffled;
  // y := residual + x W^T is computed in place on the residual buffer: copy semantics are
  // not supported (callers pass y == residual)
  if (N % 16 != 0 || (residual != nullptr && residual != y)) return -1;
  SkinnyParams p = base_params(x, w, M, N, K, x_stride, 0.f, ps, wscale, bscale);
  p.y = static_cast<uint16_t*>(y);
  p.y_stride = residual != nullptr ? res_stride : y_stride;
  return residual != nullptr
             ? launch_routed<EPI_RESADD>(p, N / 16, waves, ksplit, dtype, stream)
             : launch_routed<EPI_PLAIN>(p, N / 16, waves, ksplit, dtype, stream);
}

// Row-parallel TP GEMV with the all-reduce push fused into its epilogue: x W^T of this rank's
// K shard goes straight into slot (parity, rank) of every rank's IPC buffer (bases[q]); the
// receive side is atta_ar_push_reduce (allreduce.hip), which also adds the residual.
int atta_skinny_gemm_push(const void* x, const void* w, int M, int N, int K, int64_t x_stride,
                          int waves, int ksplit, const float* wscale, int dtype,
                          void* const* bases, int rank, int world, int64_t max_elems,
                          hipStream_t stream) {
  const int ps = (dtype & kPreshuffled) ? 1 : 0;
  dtype &= ~kPreshuffled;
  // only the 16-row-tile GEMV has the push epilogue: whatever the layout, the call routes
  // as row-major weights do
  if (route(M, false, wscale != nullptr, false, EPI_PLAIN) != Route::Skinny || N % 16 != 0) return -1;
  if ((world != 2 && world != 4 && world != 8) || rank < 0 || rank >= world ||
      static_cast<int64_t>(M) * N > max_elems)
    return -1;
  SkinnyParams p = base_params(x, w, M, N, K, x_stride, 0.f, ps, wscale);
  for (int q = 0; q < world; ++q) p.push_base[q] = static_cast<uint8_t*>(bases[q]);
  p.push_world = world;
  p.push_rank = rank;
  p.push_max_elems = max_elems;
  return launch_skinny<EPI_PLAIN>(p, N / 16, waves, ksplit, dtype, stream);
}

int atta_fused_qkv_rope(void* q_out, void* k_cache, void* v_cache, const void* x, const void* w,
                        const int* positions, const int* slots, const float* cos_sin, int M,
                        int K, int64_t x_stride, int64_t q_stride, int n_q_heads, int n_kv_heads,
                        int block_size, float eps, int waves, int ksplit, const float* wscale,
                        const uint8_t* bscale, int dtype, hipStream_t stream) {
  const int ps = (dtype & kPreshuffled) ? 1 : 0;
  dtype &= ~kPreshuffled;
  int shift = 0;
  while ((1 << shift) < block_size) ++shift;
  if ((1 << shift) != block_size) return -1;
  SkinnyParams p = base_params(x, w, M, (n_q_heads + 2 * n_kv_heads) * 128, K, x_stride, eps,
                               ps, wscale, bscale);
  p.y = static_cast<uint16_t*>(q_out);
  p.y_stride = q_stride;
  p.k_cache = static_cast<uint16_t*>(k_cache);
  p.v_cache = static_cast<uint16_t*>(v_cache);
  p.positions = positions;
  p.slots = slots;
  p.cos_sin = cos_sin;
  p.n_q_heads = n_q_heads;
  p.n_kv_heads = n_kv_heads;
  p.bs_shift = shift;
  return launch_routed<EPI_QKVROPE>(p, p.N / 16, waves, ksplit, dtype, stream);
}

int atta_fused_gate_up_silu(void* out, const void* x, const void* w, int M, int K, int inter,
                            int64_t x_stride, int64_t out_stride, float eps, int waves,
                            int ksplit, const float* wscale, const uint8_t* bscale, int dtype,
                            hipStream_t stream) {
  const int ps = (dtype & kPreshuffled) ? 1 : 0;
  dtype &= ~kPreshuffled;
  if (inter % 8 != 0) return -1;
  SkinnyParams p = base_params(x, w, M, 2 * inter, K, x_stride, eps, ps, wscale, bscale);
  p.y = static_cast<uint16_t*>(out);
  p.y_stride = out_stride;
  p.inter = inter;
  return launch_routed<EPI_SILU>(p, inter / 8, waves, ksplit, dtype, stream);
}

int atta_fused_lm_head_sample(int64_t* tokens, unsigned long long* keys, const void* x,
                              const void* w, int M, int N, int K, int64_t x_stride, float eps,
                              const float* temperature, const int64_t* seeds,
                              const int64_t* steps, int finalize, int vocab_offset,
                              int waves, const float* wscale, int dtype, hipStream_t stream) {
  const int ps = (dtype & kPreshuffled) ? 1 : 0;
  dtype &= ~kPreshuffled;
  if (N % 16 != 0) return -1;
  SkinnyParams p = base_params(x, w, M, N, K, x_stride, eps, ps, wscale);
  p.keys = keys;
  p.key_stride = N / 16;
  p.vocab_offset = vocab_offset;
  p.temperature = temperature;
  p.seeds = seeds;
  p.steps = steps;
  // unsplit: the partial keys of a (row, tile) come from one workgroup
  if (const int rc = launch_routed<EPI_SAMPLE>(p, N / 16, waves, 1, dtype, stream)) return rc;
  if (finalize == 1)
    sample_finalize_kernel<false><<<M, kFinThreads, 0, stream>>>(tokens, keys, N / 16);
  else if (finalize == 2)
    sample_finalize_kernel<true><<<M, kFinThreads, 0, stream>>>(tokens, keys, N / 16);
  return static_cast<int>(hipGetLastError());
}

// The same launch with the SAMPLE_LP epilogue and its finalize: tokens as above (bit-identical
// keys) and lp[m] = the sampled token's logprob over the raw logits.  lp_ws: M * N / 16 records
// of 16 B next to keys.  One GPU only (no key-only finalize): vocab_offset is 0.
int atta_fused_lm_head_sample_lp(int64_t* tokens, float* lp, unsigned long long* keys,
                                 void* lp_ws, const void* x, const void* w, int M, int N, int K,
                                 int64_t x_stride, float eps, const float* temperature,
                                 const int64_t* seeds, const int64_t* steps, int waves,
                                 int dtype, hipStream_t stream) {
  const int ps = (dtype & kPreshuffled) ? 1 : 0;
  dtype &= ~kPreshuffled;
  if (N % 16 != 0) return -1;
  SkinnyParams p = base_params(x, w, M, N, K, x_stride, eps, ps, nullptr);
  p.keys = keys;
  p.key_stride = N / 16;
  p.vocab_offset = 0;
  p.temperature = temperature;
  p.seeds = seeds;
  p.steps = steps;
  p.y = static_cast<uint16_t*>(lp_ws);  // lp_records()
  if (const int rc = launch_routed<EPI_SAMPLE_LP>(p, N / 16, waves, 1, dtype, stream)) return rc;
  sample_lp_finalize_kernel<<<M, kFinThreads, 0, stream>>>(tokens, lp, keys, lp_records(p), N / 16,
                                                           0);
  return static_cast<int>(hipGetLastError());
}

// Teacher-forced scoring: the SCORE epilogue and its finalize, lp[m] = logprob of targets[m] in
// row m over the raw logits.  No sampler and no keys; ws: M * N / 16 records of 16 B.  One GPU
// only: vocab_offset is 0.  A target outside [0, N) is the caller's error (its lp is then that
// of a clamped tile's record, never a read past the row).
int atta_fused_lm_head_score(float* lp, void* ws, const void* x, const void* w,
                             const int* targets, int M, int N, int K, int64_t x_stride, float eps,
                             int waves, int dtype, hipStream_t stream) {
  const int ps = (dtype & kPreshuffled) ? 1 : 0;
  dtype &= ~kPreshuffled;
  if (N % 16 != 0 || lp == nullptr || ws == nullptr || targets == nullptr) return -1;
  SkinnyParams p = base_params(x, w, M, N, K, x_stride, eps, ps, nullptr);
  p.key_stride = N / 16;
  p.vocab_offset = 0;
  p.positions = targets;                // score_targets()
  p.y = static_cast<uint16_t*>(ws);     // lp_records()
  if (const int rc = launch_routed<EPI_SCORE>(p, N / 16, waves, 1, dtype, stream)) return rc;
  score_finalize_kernel<<<M, kFinThreads, 0, stream>>>(lp, targets, lp_records(p), N / 16, 0);
  return static_cast<int>(hipGetLastError());
}

// Tuning sweep entry: plain GEMM with a selectable (waves, unroll, load policy) variant.
int atta_skinny_variant(void* y, const void* x, const void* w, int M, int N, int K,
                        int variant, hipStream_t stream) {
  SkinnyParams p{};
  p.x = static_cast<const uint16_t*>(x);
  p.w = static_cast<const uint16_t*>(w);
  p.y = static_cast<uint16_t*>(y);
  p.x_stride = K;
  p.y_stride = N;
  p.M = M;
  p.N = N;
  p.K = K;
  p.ksplit = 1;
  if (M < 1 || M > 16 || N % 16) return -1;
  dim3 grid(N / 16);
  static const int waves_of[23] = {8, 8, 4, 4, 8, 16, 8, 16, 8, 16, 8, 16, 4, 4,
                                   4, 4, 4, 8, 8, 8, 16, 16, 16};
  if (variant < 0 || variant > 22 || K % (32 * waves_of[variant])) return -1;
  switch (variant) {
    case 0: skinny_kernel<__bf16, 8, 4, 1, EPI_PLAIN, true><<<grid, 512, 0, stream>>>(p); break;
    case 1: skinny_kernel<__bf16, 8, 8, 1, EPI_PLAIN, false><<<grid, 512, 0, stream>>>(p); break;
    case 2: skinny_kernel<__bf16, 4, 4, 1, EPI_PLAIN, false><<<grid, 256, 0, stream>>>(p); break;
    case 3: skinny_kernel<__bf16, 4, 8, 1, EPI_PLAIN, false><<<grid, 256, 0, stream>>>(p); break;
    case 4: skinny_kernel<__bf16, 8, 4, 1, EPI_PLAIN, false><<<grid, 512, 0, stream>>>(p); break;
    case 5: skinny_kernel<__bf16, 16, 4, 1, EPI_PLAIN, false><<<grid, 1024, 0, stream>>>(p); break;
    case 6: skinny_kernel<__bf16, 8, 2, 1, EPI_PLAIN, false><<<grid, 512, 0, stream>>>(p); break;
    case 7: skinny_kernel<__bf16, 16, 2, 1, EPI_PLAIN, false><<<grid, 1024, 0, stream>>>(p); break;
    // 8 / 9: pre-shuffled weights (w must come from ops.preshuffle)
    case 8: skinny_kernel<__bf16, 8, 2, 1, EPI_PLAIN, false, true><<<grid, 512, 0, stream>>>(p); break;
    case 9: skinny_kernel<__bf16, 16, 2, 1, EPI_PLAIN, false, true><<<grid, 1024, 0, stream>>>(p); break;
    case 10: skinny_kernel<__bf16, 8, 4, 1, EPI_PLAIN, false, true><<<grid, 512, 0, stream>>>(p); break;
    case 11: skinny_kernel<__bf16, 16, 4, 1, EPI_PLAIN, false, true><<<grid, 1024, 0, stream>>>(p); break;
    case 12: skinny_kernel<__bf16, 4, 4, 1, EPI_PLAIN, false, true><<<grid, 256, 0, stream>>>(p); break;
    case 13: skinny_kernel<__bf16, 4, 8, 1, EPI_PLAIN, false, true><<<grid, 256, 0, stream>>>(p); break;
    // 14-22: pre-shuffled + non-temporal (the production load policy), waves x unroll grid
    case 14: skinny_kernel<__bf16, 4, 2, 1, EPI_PLAIN, true, true><<<grid, 256, 0, stream>>>(p); break;
    case 15: skinny_kernel<__bf16, 4, 4, 1, EPI_PLAIN, true, true><<<grid, 256, 0, stream>>>(p); break;
    case 16: skinny_kernel<__bf16, 4, 8, 1, EPI_PLAIN, true, true><<<grid, 256, 0, stream>>>(p); break;
    case 17: skinny_kernel<__bf16, 8, 2, 1, EPI_PLAIN, true, true><<<grid, 512, 0, stream>>>(p); break;
    case 18: skinny_kernel<__bf16, 8, 4, 1, EPI_PLAIN, true, true><<<grid, 512, 0, stream>>>(p); break;
    case 19: skinny_kernel<__bf16, 8, 8, 1, EPI_PLAIN, true, true><<<grid, 512, 0, stream>>>(p); break;
    case 20: skinny_kernel<__bf16, 16, 2, 1, EPI_PLAIN, true, true><<<grid, 1024, 0, stream>>>(p); break;
    case 21: skinny_kernel<__bf16, 16, 4, 1, EPI_PLAIN, true, true><<<grid, 1024, 0, stream>>>(p); break;
    case 22: skinny_kernel<__bf16, 16, 8, 1, EPI_PLAIN, true, true><<<grid, 1024, 0, stream>>>(p); break;
    default: return -1;
  }
  return static_cast<int>(hipGetLastError());
}

int atta_sample_finalize(int64_t* tokens, const unsigned long long* keys, int M, int n_tiles,
                         hipStream_t stream) {
  if (M <= 0 || n_tiles <= 0) return 0;
  sample_finalize_kernel<false><<<M, kFinThreads, 0, stream>>>(tokens, keys, n_tiles);
  return static_cast<int>(hipGetLastError());
}
