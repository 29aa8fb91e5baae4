// MXFP4 build of the skinny (decode) GEMV body (skinny.h; launchers: gemv_w4.hip): 4-bit
// e2m1 weights in 32-element blocks with one e8m0 scale each (OCP Microscaling FP4),
// converted to 16-bit MFMA operands in registers with the block scale already applied.
//
// Layout (ops.preshuffle_mxfp4).  Codes: per 16-row tile (rows permuted by tile_row<EPI>) and
// 128-wide K chunk c, the 1 KiB the 64 lanes load - lane l's 16 bytes are row (l & 15) of the
// chunk's four 32-wide K steps: dword j holds k = 128 c + 32 j + 8 (l >> 4) + i, code i in
// bits 4i .. 4i + 3.  Byte b of the dword is elements 2b, 2b + 1 - what byte select b of
// v_cvt_scalef32_pk_{bf16,f16}_fp4 converts - so four converts turn dword j into the lane's
// B fragment of MFMA step j.  Scales: a separate array, 64 B per tile and chunk - one dword
// per row, byte j = the e8m0 scale of K step j (+ 6.25 % on the codes); e8m0 byte b is the
// float with bits b << 23.
//
// K: a wave load covers 128 of K, so K % 128 == 0 is the only shape rule.  A (split-K) slice
// is `chunks` whole loads, dealt to the waves in runs of ceil(chunks / WAVES): the last waves
// take fewer or none (inter 2816 = 22 loads, hidden 256 = 2).  No scale after the K reduction:
// every block's scale went in with the convert.
#pragma once

#include "skinny.h"

namespace atta {

template <typename T>
struct Fp4Cvt;
template <>
struct Fp4Cvt<__bf16> {
  template <int B>
  __device__ static __forceinline__ uint32_t pk(uint32_t w, float s) {
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, s, B));
  }
};
template <>
struct Fp4Cvt<_Float16> {
  template <int B>
  __device__ static __forceinline__ uint32_t pk(uint32_t w, float s) {
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, s, B));
  }
};

// eight e2m1 codes (one dword) times 2^(e8m0 - 127) -> the 8 x 16-bit MFMA operand
template <typename T>
__device__ __forceinline__ typename MfmaK32<T>::frag8 fp4x8_to_frag(uint32_t codes,
                                                                     uint32_t e8m0) {
  const float s = __uint_as_float(e8m0 << 23);
  const u32x4 r = {Fp4Cvt<T>::template pk<0>(codes, s), Fp4Cvt<T>::template pk<1>(codes, s),
                   Fp4Cvt<T>::template pk<2>(codes, s), Fp4Cvt<T>::template pk<3>(codes, s)};
  return __builtin_bit_cast(typename MfmaK32<T>::frag8, r);
}

// Everything after the K loop, as in skinny_body (kept a copy there: its builds' generated
// code stays as it is): cross-wave LDS reduction of the per-wave accumulators acc[t] (+ row
// sums of squares ss[t]), split-K hand-over, tile_epilogue.  No row scale and no TP push.
template <typename T, int WAVES, int MT, int EPI>
__device__ __forceinline__ void skinny_finish(const SkinnyParams& p, const int tile, const int ks,
                                              const int ksplit, const f32x4 (&acc)[MT],
                                              const float (&ss)[MT],
                                              float (&red)[WAVES][MT * 16][17],
                                              float (&ssq)[WAVES][MT * 16],
                                              float (&inv_rms)[MT * 16], int& sk_last,
                                              const bool norm, const int wid, const int col,
                                              const int grp) {
  constexpr int R = MT * 16;
  // ---- cross-wave reduction ------------------------------------------------------------
#pragma unroll
  for (int t = 0; t < MT; ++t) {
#pragma unroll
    for (int i = 0; i < 4; ++i) red[wid][t * 16 + 4 * grp + i][col] = acc[t][i];
    if (norm) {
      float v = ss[t];
      v += __shfl_xor(v, 16, kWave);
      v += __shfl_xor(v, 32, kWave);
      if (grp == 0) ssq[wid][t * 16 + col] = v;
    }
  }
  __syncthreads();
  // inv_rms[] holds the row sum of squares until the rsqrt below
  if (norm && threadIdx.x < R) {
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < WAVES; ++q) s += ssq[q][threadIdx.x];
    inv_rms[threadIdx.x] = s;
  }
  // sum wave partials into red[0]
  for (int e = threadIdx.x; e < R * 16; e += WAVES * 64) {
    const int m = e >> 4, n = e & 15;
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < WAVES; ++q) s += red[q][m][n];
    red[0][m][n] = s;
  }
  __syncthreads();
  if (ksplit > 1) {
    // ---- split-K hand-over (device-scope sc1 stores/loads + arrival counter, no fences:
    // common.h "device-coherent hand-over"); slot = R*16 partial sums + R row sums of squares
    constexpr int kSlot = R * 16 + R;
    const auto rws = dev_rsrc(p.sk_ws);
    const uint32_t mine = static_cast<uint32_t>((tile * ksplit + ks) * kSlot) * 4u;
    for (int e = threadIdx.x; e < R * 16; e += WAVES * 64)
      if ((e >> 4) < p.M) dev_store4(rws, mine + e * 4, red[0][e >> 4][e & 15]);
    if (norm && threadIdx.x < R && threadIdx.x < p.M)
      dev_store4(rws, mine + (R * 16 + threadIdx.x) * 4, inv_rms[threadIdx.x]);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's stores acknowledged
    __syncthreads();
    if (threadIdx.x == 0) {
      const int old = __hip_atomic_fetch_add(p.sk_counters + tile, 1, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT);
      sk_last = (old == ksplit - 1);
    }
    __syncthreads();
    if (!sk_last) return;  // block-uniform
    const uint32_t first = static_cast<uint32_t>(tile * ksplit * kSlot) * 4u;
    for (int e = threadIdx.x; e < R * 16; e += WAVES * 64) {
      if ((e >> 4) >= p.M) continue;
      float s = 0.f;
      for (int q = 0; q < ksplit; ++q) s += dev_load4(rws, first + (q * kSlot + e) * 4);
      red[0][e >> 4][e & 15] = s;
    }
    if (norm && threadIdx.x < R && threadIdx.x < p.M) {
      float s = 0.f;
      for (int q = 0; q < ksplit; ++q)
        s += dev_load4(rws, first + (q * kSlot + R * 16 + threadIdx.x) * 4);
      inv_rms[threadIdx.x] = s;
    }
    if (threadIdx.x == 0)
      __hip_atomic_store(p.sk_counters + tile, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
  }
  if (norm && threadIdx.x < R)
    inv_rms[threadIdx.x] = rsqrtf(inv_rms[threadIdx.x] / static_cast<float>(p.K) + p.eps);
  __syncthreads();

  tile_epilogue<T, EPI, MT>(p, tile, red[0], inv_rms, norm, threadIdx.x, WAVES * 64);
}

// UNROLL: 128-wide K chunks per register stage (4 MFMA steps each).  Drained load order (the
// next stage's weights, then this stage's x): see skinny_body.
template <typename T, int WAVES, int UNROLL, int MT, int EPI, bool NTL>
__device__ __forceinline__ void skinny_w4_body(const SkinnyParams& p, const int tile,
                                               const int ks, const int ksplit) {
  using MF = MfmaK32<T>;
  using frag8 = typename MF::frag8;
  constexpr int R = MT * 16;
  __shared__ float red[WAVES][R][17];
  __shared__ float ssq[WAVES][R];
  __shared__ float inv_rms[R];
  __shared__ int sk_last;

  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int col = lane & 15;
  const int grp = lane >> 4;
  const int row_chunks = p.K / 128;
  const int chunks = row_chunks / ksplit;            // this slice's loads
  const int per = (chunks + WAVES - 1) / WAVES;      // a wave's run
  const int c0 = min(wid * per, chunks);
  const int n = min(c0 + per, chunks) - c0;          // this wave's loads (may be 0)
  const int cbeg = ks * chunks + c0;
  const int64_t first = static_cast<int64_t>(tile) * row_chunks + cbeg;
  const uint8_t* wp = reinterpret_cast<const uint8_t*>(p.w) + first * 1024 + lane * 16;
  const uint8_t* sp = p.bscale + first * 64 + col * 4;
  const uint16_t* xp[MT];
  bool xv[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int m = t * 16 + col;
    xv[t] = m < p.M;
    xp[t] = p.x + static_cast<int64_t>(xv[t] ? m : 0) * p.x_stride + cbeg * 128 + 8 * grp;
  }
  f32x4 acc[MT];
  float ss[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    ss[t] = 0.f;
  }
  const bool norm = p.eps > 0.f;

  using Raw = u32x4;
  auto load_codes = [&](int c) -> Raw {
    const Raw* src = reinterpret_cast<const Raw*>(wp + static_cast<int64_t>(c) * 1024);
    if constexpr (NTL) return __builtin_nontemporal_load(src);
    else return *src;
  };
  auto load_scales = [&](int c) -> uint32_t {
    return *reinterpret_cast<const uint32_t*>(sp + static_cast<int64_t>(c) * 64);
  };
  // one chunk: four converts + one MFMA per 32-wide K step and row tile
  auto compute_chunk = [&](const Raw w, const uint32_t s, int c) {
    frag8 wf[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) wf[j] = fp4x8_to_frag<T>(w[j], (s >> (8 * j)) & 0xffu);
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      frag8 xf[4];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        xf[j] = xv[t] ? *reinterpret_cast<const frag8*>(xp[t] + c * 128 + 32 * j) : frag8{};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        acc[t] = MF::mma(xf[j], wf[j], acc[t]);
        if (norm) ss[t] = MF::sq8(xf[j], ss[t]);
      }
    }
  };
  struct Stage {
    Raw w[UNROLL];
    uint32_t s[UNROLL];
  };
  auto load_stage = [&](Stage& st, int c) {
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      st.w[u] = load_codes(c + u);
      st.s[u] = load_scales(c + u);
    }
  };
  auto compute_stage = [&](const Stage& st, int c) {
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) compute_chunk(st.w[u], st.s[u], c + u);
  };
  const int nstages = n / UNROLL;
  if (nstages > 0) {
    Stage sa, sb;
    load_stage(sa, 0);
    int s = 0;
    for (; s + 2 <= nstages; s += 2) {
      load_stage(sb, (s + 1) * UNROLL);
      compute_stage(sa, s * UNROLL);
      if (s + 2 < nstages) load_stage(sa, (s + 2) * UNROLL);
      compute_stage(sb, (s + 1) * UNROLL);
    }
    if (s < nstages) compute_stage(sa, s * UNROLL);
  }
  for (int c = nstages * UNROLL; c < n; ++c)  // tail: one load at a time
    compute_chunk(load_codes(c), load_scales(c), c);

  skinny_finish<T, WAVES, MT, EPI>(p, tile, ks, ksplit, acc, ss, red, ssq, inv_rms, sk_last,
                                   norm, wid, col, grp);
}

}  // namespace atta
