// Decode paged attention: split-K over context partitions with an in-kernel combine
// (guide §5 "In-launch split-K reduction").  One body for both decode
// kernels: attention_decode.hip instantiates it with MQ = false (one query token per
// sequence, plain decode), attention_decode_mq.hip with MQ = true (up to 16 / G query tokens
// per sequence, the verify step of speculative decoding).
//
// grid = (seqs, kv_heads, max_partitions); a workgroup of WAVES waves owns one partition of
// WAVES * 16 * TPW tokens of one (sequence, KV head).  Decode attention at agent-workload
// sizes is LATENCY bound (a few MB of KV per layer), so the kernel minimises dependent
// memory round trips per wave:
//   1. Q fragment + the block-table entries of the wave's TPW tiles are loaded together;
//   2. the K/V fragments of ALL the wave's tiles are issued at once (no per-tile
//      block-table -> K/V dependency chain);
//   3. online softmax + PV over the tiles, one LDS merge of the WAVES partial states.
// The GQA group's G query heads are the MFMA columns (swapped QK^T, see attention.hip), so
// K/V are read once for all G heads.  Partitions past the sequence end exit immediately,
// so a hipGraph captured with the maximum partition count costs nothing for short contexts.
//
// Combine: with more than one partition each workgroup writes (O normalised, lse) fp32 to a
// workspace with device-scope stores and arrives on a per-(seq, kv-head) counter; the last
// arriver reads every partition back with device-scope loads, merges them and writes the
// bf16 output, then re-arms the counter (counters are zeroed once at allocation).
//
// Multi-query (MQ): the one-token kernel leaves 16 - G of the 16 MFMA columns empty.  With MQ
// the same K/V fragments and the same MFMAs serve up to 16 / G query tokens of one sequence:
// sequence s owns the query rows seq_qstart[s] .. seq_qstart[s + 1] - 1 (qlen of them,
// 1 <= qlen <= 16 / G) and the MFMA column of (token j, head g) is j * G + g.  Token j sits at
// position kvlen - qlen + j (seq_kvlen counts the rows of this step), so it sees the keys
// < kvlen - (qlen - 1 - j): a per-lane bound, a lane's column being fixed.  Everything per
// column (running max and sum, the shfl_xor 16 / 32 reductions) is the same; the wave merge,
// the publish, the last arriver's combine and the output store run over the G * qlen live
// columns.  A partition in which a column sees no key (the first tokens of a sequence whose
// last partition holds only draft positions) publishes lse = -inf for it and still arrives.
//
// The two variants differ only inside `if constexpr (MQ)` (a discarded branch emits no code,
// so each instantiation sees one straight-line body): the query rows of a column, its causal
// bound, the live column count (G at compile time, G * qlen at run time), the LDS staging
// of the wave merge, the output row and the timeline probe.  Keep the statements in this one
// function: hoisting a part of it into a helper moves the register allocation of every
// instantiation.
#pragma once

#include "common.h"

namespace atta {

// MFMA pair of the swapped-QK^T attention kernels (attention.hip header comment).
template <typename T>
struct Mfma;
template <>
struct Mfma<__bf16> {
  typedef bf16x8 frag8;
  __device__ static __forceinline__ f32x4 qk(frag8 a, frag8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  }
  __device__ static __forceinline__ f32x4 pv(i16x4 a, i16x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, b, c, 0, 0, 0);
  }
};
template <>
struct Mfma<_Float16> {
  typedef f16x8 frag8;
  __device__ static __forceinline__ f32x4 qk(frag8 a, frag8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
  }
  __device__ static __forceinline__ f32x4 pv(i16x4 a, i16x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_bit_cast(f16x4, a),
                                                 __builtin_bit_cast(f16x4, b), c, 0, 0, 0);
  }
};

namespace dec {

constexpr int kD = 128;
constexpr float kNegInf = -__builtin_huge_valf();

struct DecParams {
  uint16_t* out;
  float* part_out;  // [S, Hkv, P, 16, D]
  float* part_lse;  // [S, Hkv, P, 16]
  int* counters;    // [S, Hkv]
  const uint16_t* q;
  const uint16_t* k_cache;
  const uint16_t* v_cache;
  const int* block_tables;
  const int* seq_kvlen;
  const int* seq_qstart;
  int64_t q_stride, out_stride;
  int bt_stride, n_kv_heads, bs_shift, part_tokens, max_parts;
  float scale_log2;
  // optional per-workgroup timeline (100 MHz wall clock): [start, past-wait, end, hw id];
  // one-token kernel only (null for multi-query)
  unsigned long long* wg_trace;
};

template <typename T>
struct TileFrags {
  typename Mfma<T>::frag8 k[4];
  i16x4 v[8];
};

template <typename T, int G, int WAVES, int TPW, bool MQ>
__device__ __forceinline__ void decode_attention_body(const DecParams& p, const int s,
                                                      const int hk, const int part,
                                                      unsigned long long (&tr)[3]) {
  using frag8 = typename Mfma<T>::frag8;
  constexpr int NT = WAVES * 64;
  constexpr int QMAX = 16 / G;       // query tokens per sequence the 16 columns hold
  constexpr int LC = MQ ? 16 : G;    // columns a workgroup can have live
  // merge groups of the last arriver's combine when one token is live, and the partitions
  // each of its threads loads per round trip: 8 when there are few merge groups (4-wave
  // workgroups: 4 groups cover 32 partitions - a 4k context at 128-token partitions - in one
  // round trip), else 4
  constexpr int NG1 = NT / (16 * G) < 16 ? NT / (16 * G) : 16;
  constexpr int PPI = NG1 <= 4 ? 8 : 4;
  __shared__ float lds_m[WAVES][LC];
  __shared__ float lds_l[WAVES][LC];
  __shared__ int lds_last;
  // multi-query: the wave merge stages WAVES x columns x 128 fp32 in LDS: 8-wave workgroups
  // take the columns in two passes of 8 (one pass of 16 would need 66 KB); the combine's group
  // states reuse the staging area (dead by then).  The one-token kernel declares its two
  // arrays where it uses them.
  constexpr int CPP = WAVES > 4 ? 8 : 16;
  float* lds_raw = nullptr;
  if constexpr (MQ) {
    static_assert(NT >= 256, "one merger thread per (column, 8 dims)");
    constexpr int kStage = WAVES * CPP * (kD + 4);
    __shared__ float raw[kStage > 10 * NT ? kStage : 10 * NT];
    lds_raw = raw;
  }

  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int col = lane & 15;
  const int grp = lane >> 4;
  const int PT = WAVES * 16 * TPW;
  const int kv_begin = part * PT;
  // ---- round trip 1: sequence length, query rows and the block-table entries of this wave's
  // tiles are independent loads - the entries are fetched unconditionally (index clamped to
  // the table row) and only used for tiles inside the sequence
  const int* bt = p.block_tables + static_cast<int64_t>(s) * p.bt_stride;
  const int wid_u = __builtin_amdgcn_readfirstlane(wid);  // wave-uniform -> scalar loads
  int kt[TPW], bte[TPW];
#pragma unroll
  for (int i = 0; i < TPW; ++i) {
    kt[i] = kv_begin + (wid_u + i * WAVES) * 16;
    bte[i] = bt[min(kt[i] >> p.bs_shift, p.bt_stride - 1)];
  }
  int kvlen = p.seq_kvlen[s];
  int qlast = p.seq_qstart[s + 1] - 1;  // the sequence's last query row
  int qbeg = 0;                         // its first: multi-query only
  // one wait for all of them (keeps the compiler from chaining the loads behind branches)
  if constexpr (MQ) {
    qbeg = p.seq_qstart[s];
    asm volatile("" : "+s"(kvlen), "+s"(qbeg), "+s"(qlast));
  } else {
    asm volatile("" : "+s"(kvlen), "+s"(qlast));
  }
#pragma unroll
  for (int i = 0; i < TPW; ++i) asm volatile("" : "+s"(bte[i]));
  // timeline probe: clock reads only after the scalar loads above - an earlier one makes
  // them vector loads, which the scalar-operand asm cannot take
  if constexpr (!MQ) tr[0] = wall_clock64();
  const int nparts = (kvlen + PT - 1) / PT;
  if (part >= nparts) return;  // block-uniform (also kvlen == 0 dummy sequences)
  int qlen = 1;  // query rows of the sequence
  if constexpr (MQ) {
    // the host validates 1 <= qlen <= QMAX; the clamp keeps a bad table inside the 16
    // columns (it then serves the last QMAX rows)
    qlen = min(qlast + 1 - qbeg, QMAX);
    if (qlen < 1) return;
  }
  const int qstart = qlast + 1 - qlen;
  const int ncol = G * qlen;  // live columns (one-token: the constant G)
  const int kv_end = min(kvlen, kv_begin + PT);
  const int BS = 1 << p.bs_shift;
  const int64_t hs = static_cast<int64_t>(BS) * kD;
  int page[TPW];
#pragma unroll
  for (int i = 0; i < TPW; ++i) page[i] = kt[i] < kv_end ? bte[i] : 0;

  // this lane's column: query token jq, head hg of the group; keys it sees end at klim
  const int jq = MQ ? col / G : 0;
  const int hg = col - jq * G;
  const bool live = col < ncol;
  const int klim = MQ ? (live ? min(kv_end, kvlen - (qlen - 1 - jq)) : kv_begin) : kv_end;

  // ---- round trip 2: Q fragment (needs the query row) + K/V fragments of all tiles --------
  frag8 qf[4];
  {
    const uint16_t* qp = p.q + static_cast<int64_t>(qstart + (live ? jq : 0)) * p.q_stride +
                         static_cast<int64_t>(hk * G + (live ? hg : 0)) * kD + 32 * grp;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
      qf[kk] = live ? *reinterpret_cast<const frag8*>(qp + 8 * kk) : frag8{};
  }

  TileFrags<T> f[TPW];
#pragma unroll
  for (int i = 0; i < TPW; ++i) {
    if (kt[i] < kv_end) {
      const uint16_t* base = p.k_cache + (static_cast<int64_t>(page[i]) * p.n_kv_heads + hk) * hs;
      const uint16_t* kp = base + static_cast<int64_t>((kt[i] + col) & (BS - 1)) * kD + 32 * grp;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) f[i].k[kk] = *reinterpret_cast<const frag8*>(kp + 8 * kk);
      const uint16_t* vb = p.v_cache + (static_cast<int64_t>(page[i]) * p.n_kv_heads + hk) * hs;
      const uint16_t* vp = vb + static_cast<int64_t>(col) * BS + ((kt[i] + 4 * grp) & (BS - 1));
#pragma unroll
      for (int dt = 0; dt < 8; ++dt)
        f[i].v[dt] = *reinterpret_cast<const i16x4*>(vp + static_cast<int64_t>(16 * dt) * BS);
    }
  }

  // ---- compute --------------------------------------------------------------------------
  f32x4 o[8];
#pragma unroll
  for (int dt = 0; dt < 8; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run = kNegInf, l_run = 0.f;
#pragma unroll
  for (int i = 0; i < TPW; ++i) {
    if (kt[i] >= kv_end) break;  // wave-uniform
    const TileFrags<T>& ft = f[i];
    const int kbase = kt[i];
    const int kend = kv_end;
    f32x4 sacc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) sacc = Mfma<T>::qk(ft.k[kk], qf[kk], sacc);
    float sv[4], tmax = kNegInf;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      sv[j] = (kbase + 4 * grp + j < klim) ? sacc[j] * p.scale_log2 : kNegInf;
      tmax = fmaxf(tmax, sv[j]);
    }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 16, kWave));
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, kWave));
    const float m_new = fmaxf(m_run, tmax);
    const float m_use = (m_new == kNegInf) ? 0.f : m_new;
    const float alpha = exp2f(m_run - m_use);
    float psum = 0.f;
    i16x4 pf;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float pv = exp2f(sv[j] - m_use);
      psum += pv;
      pf[j] = static_cast<short>(from_f32<T>(pv));
    }
    psum += __shfl_xor(psum, 16, kWave);
    psum += __shfl_xor(psum, 32, kWave);
    l_run = l_run * alpha + psum;
    m_run = m_new;
    // keys past the sequence end (the tail slots of its last page) hold stale bytes of the
    // page's previous owner: P is 0 there, and V is zeroed too so a non-finite stale value
    // cannot make 0 * V a NaN (wave-uniform edge test: the last tile only).  Keyed on kvlen,
    // not on klim: the keys a token's causal bound hides were written by this step and are
    // finite
    i16x4 vv[8];
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) vv[dt] = ft.v[dt];
    if (kbase + 16 > kend) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (kbase + 4 * grp + j >= kend) {
#pragma unroll
          for (int dt = 0; dt < 8; ++dt) vv[dt][j] = 0;
        }
    }
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) {
      o[dt] *= alpha;
      o[dt] = Mfma<T>::pv(vv[dt], pf, o[dt]);
    }
  }
  if constexpr (!MQ) tr[1] = wall_clock64();

  // ---- merge the WAVES partial states of the live columns -----------------------------------
  // thread t < 16 * ncol merges column t / 16, dims 8 * (t % 16) ..
  const bool merger = threadIdx.x < ncol * 16;
  const int c = threadIdx.x >> 4;          // column
  const int d0 = (threadIdx.x & 15) * 8;   // dims d0..d0+7
  float r[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float mu = 0.f, L = 0.f;
  if constexpr (MQ) {
    // with CPP = 8 the columns >= 8 go through lds_o in a second pass (skipped when none is
    // live)
    float (*lds_o)[CPP][kD + 4] = reinterpret_cast<float (*)[CPP][kD + 4]>(lds_raw);
    if (live && grp == 0) {
      lds_m[wid][col] = m_run;
      lds_l[wid][col] = l_run;
    }
#pragma unroll
    for (int c0 = 0; c0 < 16; c0 += CPP) {
      if (c0 >= ncol) break;  // block-uniform
      if (c0 > 0) __syncthreads();  // the first pass's readers are done with lds_o
      if (live && col >= c0 && col < c0 + CPP) {
#pragma unroll
        for (int dt = 0; dt < 8; ++dt)
#pragma unroll
          for (int j = 0; j < 4; ++j) lds_o[wid][col - c0][16 * dt + 4 * grp + j] = o[dt][j];
      }
      __syncthreads();
      if (merger && c >= c0 && c < c0 + CPP) {
        float mx = kNegInf;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) mx = fmaxf(mx, lds_m[w][c]);
        mu = (mx == kNegInf) ? 0.f : mx;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
          const float fw = exp2f(lds_m[w][c] - mu);
          L += fw * lds_l[w][c];
#pragma unroll
          for (int j = 0; j < 8; ++j) r[j] += fw * lds_o[w][c - c0][d0 + j];
        }
        const float invL = L > 0.f ? 1.f / L : 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] *= invL;
      }
    }
  } else {
    __shared__ float lds_o[WAVES][G][kD + 4];
    if (live) {
#pragma unroll
      for (int dt = 0; dt < 8; ++dt)
#pragma unroll
        for (int j = 0; j < 4; ++j) lds_o[wid][col][16 * dt + 4 * grp + j] = o[dt][j];
      if (grp == 0) {
        lds_m[wid][col] = m_run;
        lds_l[wid][col] = l_run;
      }
    }
    __syncthreads();
    if (merger) {
      float mx = kNegInf;
#pragma unroll
      for (int w = 0; w < WAVES; ++w) mx = fmaxf(mx, lds_m[w][c]);
      mu = (mx == kNegInf) ? 0.f : mx;
#pragma unroll
      for (int w = 0; w < WAVES; ++w) {
        const float fw = exp2f(lds_m[w][c] - mu);
        L += fw * lds_l[w][c];
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] += fw * lds_o[w][c][d0 + j];
      }
      const float invL = L > 0.f ? 1.f / L : 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) r[j] *= invL;
    }
  }
  const int tj = MQ ? c / G : 0;  // the column's query token
  uint16_t* outp = p.out + static_cast<int64_t>(qstart + tj) * p.out_stride +
                   static_cast<int64_t>(hk * G + (c - tj * G)) * kD + d0;
  if (nparts == 1) {
    if (merger) {
      Pack8 o8;
#pragma unroll
      for (int j = 0; j < 8; ++j) o8.v[j] = from_f32<T>(r[j]);
      *reinterpret_cast<Pack8*>(outp) = o8;
    }
    return;
  }

  // ---- publish this partition; the last arriver combines -----------------------------------
  // Partials travel with device-scope (sc1) buffer stores/loads (common.h "device-coherent
  // hand-over"): no agent-scope release/acquire, i.e. no whole-L2 writeback/invalidate per
  // workgroup - 12.6 -> 10.2 us at ctx 1000, 24.3 -> 16.0 us at ctx 2000 (B = 5,
  // profiles/r1_fused_attn_oproj_experiment.txt).
  const int64_t sh = static_cast<int64_t>(s) * p.n_kv_heads + hk;
  const auto rpo = dev_rsrc(p.part_out);
  const auto rpl = dev_rsrc(p.part_lse);
  if (merger) {
    const int64_t base = (sh * p.max_parts + part) * 16 + c;
    const uint32_t off = static_cast<uint32_t>((base * kD + d0) * 4);
    dev_store16(rpo, off, __builtin_bit_cast(u32x4, f32x4{r[0], r[1], r[2], r[3]}));
    dev_store16(rpo, off + 16, __builtin_bit_cast(u32x4, f32x4{r[4], r[5], r[6], r[7]}));
    if ((threadIdx.x & 15) == 0)
      dev_store4(rpl, static_cast<uint32_t>(base * 4), (L > 0.f) ? (mu + log2f(L)) : kNegInf);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // device-scope stores acknowledged
  __syncthreads();
  if (threadIdx.x == 0) {
    const int old = __hip_atomic_fetch_add(p.counters + sh, 1, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
    lds_last = (old == nparts - 1);
  }
  __syncthreads();
  if constexpr (!MQ) tr[2] = wall_clock64();
  if (!lds_last) return;
  // merge in one round trip for <= PPI * ng partitions: the workgroup's threads form ng merge
  // groups of mg = 16 * ncol (one thread per (column, 8 dims)); group g loads partitions g,
  // g + ng, ... (PPI per round trip) and folds them into a running (max, weight sum, weighted
  // sum); the group states meet in LDS and group 0 folds them in group order (fixed order: the
  // output does not depend on timing or on the launch's partition grid).  ng follows the live
  // column count, so a one-token sequence folds its partitions in the same order in both
  // kernels.  Was: the 64 merger threads alone, 4 partitions per dependent round trip
  // (12 partitions at 3k tokens = 3 round trips).
  {
    // group states in LDS: value k (max, weight sum, 8 sums) of thread lt of group g is at
    // g * gstride + k * kstride + lt
    constexpr int kstride = MQ ? NT : G * 16;
    float* lds_mg = lds_raw;
    if constexpr (!MQ) {
      __shared__ float mg1[NG1 * 10 * kstride];
      lds_mg = mg1;
    }
    const int mg = ncol * 16;
    const int ng = min(NT / mg, 16);
    const int gstride = MQ ? mg : 10 * kstride;
    const int gidx = threadIdx.x / mg;
    const int lt = threadIdx.x % mg;
    const int mc = lt >> 4;
    const int md0 = (lt & 15) * 8;
    const int np = min(nparts, 64);
    float m_acc = kNegInf, wsum = 0.f;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (gidx < ng) {
      for (int u0 = 0; gidx + ng * u0 < np; u0 += PPI) {
        float lse[PPI];
        f32x4 pa[PPI], pb[PPI];
#pragma unroll
        for (int u = 0; u < PPI; ++u) {
          const int q = min(gidx + ng * (u0 + u), np - 1);
          const int64_t base = (sh * p.max_parts + q) * 16 + mc;
          const uint32_t off = static_cast<uint32_t>((base * kD + md0) * 4);
          lse[u] = dev_load4(rpl, static_cast<uint32_t>(base * 4));
          pa[u] = __builtin_bit_cast(f32x4, dev_load16(rpo, off));
          pb[u] = __builtin_bit_cast(f32x4, dev_load16(rpo, off + 16));
        }
#pragma unroll
        for (int u = 0; u < PPI; ++u) {
          if (gidx + ng * (u0 + u) >= np || lse[u] == kNegInf) continue;  // weight 0
          const float m_new = fmaxf(m_acc, lse[u]);
          const float sc = exp2f(m_acc - m_new);  // m_acc == -inf -> 0
          const float w = exp2f(lse[u] - m_new);
          wsum = wsum * sc + w;
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) {
            acc[jj] = acc[jj] * sc + w * pa[u][jj];
            acc[4 + jj] = acc[4 + jj] * sc + w * pb[u][jj];
          }
          m_acc = m_new;
        }
      }
      float* mine = lds_mg + gidx * gstride + lt;
      mine[0] = m_acc;
      mine[kstride] = wsum;
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) mine[(2 + jj) * kstride] = acc[jj];
    }
    __syncthreads();
    if (gidx == 0) {
      for (int g = 1; g < ng; ++g) {
        const float* theirs = lds_mg + g * gstride + lt;
        const float gm = theirs[0];
        if (gm == kNegInf) continue;
        const float m_new = fmaxf(m_acc, gm);
        const float sc = exp2f(m_acc - m_new);
        const float w = exp2f(gm - m_new);
        wsum = wsum * sc + w * theirs[kstride];
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) acc[jj] = acc[jj] * sc + w * theirs[(2 + jj) * kstride];
        m_acc = m_new;
      }
      const float inv = wsum > 0.f ? 1.f / wsum : 0.f;
      const int tj = MQ ? mc / G : 0;
      Pack8 o8;
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) o8.v[jj] = from_f32<T>(acc[jj] * inv);
      *reinterpret_cast<Pack8*>(p.out + static_cast<int64_t>(qstart + tj) * p.out_stride +
                                static_cast<int64_t>(hk * G + (mc - tj * G)) * kD + md0) = o8;
    }
  }
  if (threadIdx.x == 0)
    __hip_atomic_store(p.counters + sh, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The two kernels: each translation unit defines its own (the one-token one records the
// timeline probe).
template <typename T, int G, int WAVES, int TPW>
__global__ __launch_bounds__(WAVES * 64) void decode_attention_kernel(DecParams p);
template <typename T, int G, int WAVES, int TPW>
__global__ __launch_bounds__(WAVES * 64) void decode_attention_mq_kernel(DecParams p);

template <typename T, int G, int WAVES, int TPW, bool MQ>
static int launch_kernel(dim3 grid, hipStream_t st, const DecParams& p) {
  if constexpr (MQ)
    decode_attention_mq_kernel<T, G, WAVES, TPW><<<grid, WAVES * 64, 0, st>>>(p);
  else
    decode_attention_kernel<T, G, WAVES, TPW><<<grid, WAVES * 64, 0, st>>>(p);
  return 0;
}

template <typename T, int WAVES, int TPW, bool MQ>
static int launch_g(int G, dim3 grid, hipStream_t st, const DecParams& p) {
  switch (G) {
    case 1: return launch_kernel<T, 1, WAVES, TPW, MQ>(grid, st, p);
    case 2: return launch_kernel<T, 2, WAVES, TPW, MQ>(grid, st, p);
    case 3: return launch_kernel<T, 3, WAVES, TPW, MQ>(grid, st, p);
    case 4: return launch_kernel<T, 4, WAVES, TPW, MQ>(grid, st, p);
    case 8: return launch_kernel<T, 8, WAVES, TPW, MQ>(grid, st, p);
    default: return -1;
  }
}

// part_tokens selects the workgroup shape: 64 = 4 waves x 1 tile, 128 = 8 waves x 1 tile (or
// 4 x 2 where the one-token caller asks for waves128 = 4), 256 = 8 x 2, 512 = 16 x 2 (16 waves
// cap VGPRs at 128: more tiles per wave would spill).  The 4 x 2 and the 16-wave shapes have
// no multi-query twin.
template <typename T, bool MQ>
static int launch(int G, int part_tokens, int waves128, dim3 grid, hipStream_t st,
                  const DecParams& p) {
  switch (part_tokens) {
    case 64: return launch_g<T, 4, 1, MQ>(G, grid, st, p);
    case 128:
      if constexpr (!MQ)
        if (waves128 == 4) return launch_g<T, 4, 2, MQ>(G, grid, st, p);
      return launch_g<T, 8, 1, MQ>(G, grid, st, p);
    case 256: return launch_g<T, 8, 2, MQ>(G, grid, st, p);
    case 512:
      if constexpr (!MQ) return launch_g<T, 16, 2, MQ>(G, grid, st, p);
      return -1;
    default: return -1;
  }
}

// Host side of both entry points (kernels.h: atta_attention_decode_v2 / _mq): validates the
// shapes, fills the parameters and launches.
template <bool MQ>
static int decode_attention(void* out, float* part_out, float* part_lse, int* counters,
                            const void* q, const void* k_cache, const void* v_cache,
                            const int* block_tables, const int* seq_kvlen, const int* seq_qstart,
                            int num_seqs, int max_parts, int part_tokens, int n_q_heads,
                            int n_kv_heads, int head_dim, int block_size, int bt_stride,
                            int64_t q_stride, int64_t out_stride, float scale, int dtype,
                            hipStream_t stream, int waves128, unsigned long long* wg_trace) {
  const int G = n_q_heads / n_kv_heads;
  int shift = 0;
  while ((1 << shift) < block_size) ++shift;
  if (head_dim != 128 || (1 << shift) != block_size || block_size < 16) return -1;
  if (n_q_heads % n_kv_heads || G > 8 || ((G & (G - 1)) && G != 3)) return -1;
  if (max_parts < 1 || max_parts > 64) return -1;
  if (num_seqs == 0) return 0;
  DecParams p{};
  p.out = static_cast<uint16_t*>(out);
  p.part_out = part_out;
  p.part_lse = part_lse;
  p.counters = counters;
  p.q = static_cast<const uint16_t*>(q);
  p.k_cache = static_cast<const uint16_t*>(k_cache);
  p.v_cache = static_cast<const uint16_t*>(v_cache);
  p.block_tables = block_tables;
  p.seq_kvlen = seq_kvlen;
  p.seq_qstart = seq_qstart;
  p.q_stride = q_stride;
  p.out_stride = out_stride;
  p.bt_stride = bt_stride;
  p.n_kv_heads = n_kv_heads;
  p.bs_shift = shift;
  p.part_tokens = part_tokens;
  p.max_parts = max_parts;
  p.scale_log2 = scale * 1.4426950408889634f;
  p.wg_trace = wg_trace;
  dim3 grid(num_seqs, n_kv_heads, max_parts);
  const int rc = dtype == 0 ? launch<__bf16, MQ>(G, part_tokens, waves128, grid, stream, p)
                            : launch<_Float16, MQ>(G, part_tokens, waves128, grid, stream, p);
  if (rc) return rc;
  return static_cast<int>(hipGetLastError());
}

}  // namespace dec
}  // namespace atta
