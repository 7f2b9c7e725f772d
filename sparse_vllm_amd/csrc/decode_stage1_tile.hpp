// The tile body of split-KV decode stage 1, shared by decode_stage1_kernel_v3 (decode_attention.hip: one wave per KV
// head, head_dim 64 / 128) and decode_stage1_d256_kernel (decode_attention_d256.hip: two waves per KV head, 128 head
// dims each).  Each kernel composes the pieces in its own order, so its load schedule is still written down in that
// kernel, and keeps its own LDS layout; v3 keeps the rotated store, the d256 kernel the partial-S exchange and its LEAN
// schedule.  Stage 2 is not here.
//
// The pieces are statement macros, not functions: a piece that is a function goes through the optimiser on its own
// before it is inlined, and every such split moved registers and the order of loads in the 192 instantiations (see
// profiles/r10/stage1_sharing.md).  As text the pieces compile to the instruction streams of the two hand-written
// kernels.  They work on the kernel's own locals, under these names:
//   a, b, blk, lane, n (lane & 15), jq (lane >> 4), len, start, end; constexpr D, G, NC, JQ, DW, MODE, OFF32
//   Pw / Pl (P tile), slot_lds, q_lds, spart, SP                      - the kernel's LDS layout
//   mid_o, mid_lse, direct_o, row, k_ptr, v_ptr, fetch_slots, sm_scale - declared by OUT_PTRS and ADDRESSING
//   kr, m, l, acc, s_next                                              - declared by PROLOGUE
//   has_next, cur_slots, nxt_slots, vr, s, t0, c0                     - the kernel's tile lambda
//   tv, p, alpha, rescale                                              - declared by TOKEN_VALID and SOFTMAX_STEP
// What differs between the two kernels is a macro argument:           v3            d256 (wave w = 2 kvh + hx)
//   KVH      the KV head of the wave                                  w             kvh
//   COL0P    first head dim the wave covers, as a prefix of a sum     (empty)       hx * kHalf +
//   DWV      head dims a wave covers (DW = DWV / 8 segments)          D             kHalf
//   VSEG     16-byte V segment of the lane's MFMA column              dg = n % DW   n
//   STATS    "this wave writes lse and scores &&"                     (empty)       hx == 0 &&
//   BARRIER  workgroup barrier around the HEADMAX combine             __syncthreads lds_barrier
#pragma once

#include <type_traits>

#include "svk_common.hpp"

namespace svk {
namespace {

constexpr int kTileTokens = 32;    // 2 MFMA column groups of 16 tokens
constexpr int kScoreChunk = 256;   // tokens between two score-combine barriers
constexpr int kPRow = 40;          // P tile row stride in bf16 (32 tokens + pad, 16-byte aligned rows)
constexpr int kPFloats = 16 * kPRow / 2;           // P tile [16][kPRow] bf16 expressed in floats

constexpr int stage1_jq(int G) { return (G + 3) / 4; }     // accumulator row groups holding real heads

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;

template <bool NT>
__device__ __forceinline__ uint4 ld16(const char* p) {
  if (NT) return __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(p)));
  return *reinterpret_cast<const uint4*>(p);
}

#define SVK_S1_UNROLL _Pragma("unroll")

// the partial rows of (b, blk); mid_o and direct_o start at the wave's first head dim (COL0T: "+ hx * kHalf" | empty)
#define SVK_S1_OUT_PTRS(COL0T)                                                                                        \
  float* mid_o = a.mid_o + (int64_t)b * a.mid_o_stride_b + (int64_t)blk * a.mid_o_stride_s COL0T;                    \
  float* mid_lse = a.mid_lse + (int64_t)b * a.mid_lse_stride_b + blk;                                                \
  uint16_t* direct_o = a.direct_o == nullptr ? nullptr : a.direct_o + (int64_t)b * a.direct_stride_b COL0T;

// a block beyond the row's length: partial (0, -inf)
#define SVK_S1_FILL_EMPTY(KVH, DWV, STATS)                                                                            \
  for (int h = 0; h < G; ++h) {                                                                                       \
    if (direct_o != nullptr) {                                                                                        \
      for (int d = lane; d < DWV; d += 64) direct_o[(int64_t)(KVH * G + h) * a.direct_stride_h + d] = 0;              \
    } else {                                                                                                          \
      float* o = mid_o + (int64_t)(KVH * G + h) * a.mid_o_stride_h;                                                   \
      for (int d = lane; d < DWV; d += 64) o[d] = 0.f;                                                                \
    }                                                                                                                 \
    if (STATS lane == 0) mid_lse[(int64_t)(KVH * G + h) * a.mid_lse_stride_h] = -INFINITY;                            \
  }

// Plain fused store_kvcache, for the workgroup that owns the lane's newest token: the wave writes its DWV dims of its
// kv head's K and V rows (2 x DW lanes, 16 bytes each) before any read of the row.  COL: the lane's column in the
// head row, `seg * 8` | `col` with COLDECL `const int64_t col = hx * kHalf + seg * 8;` (each kernel's own integer width).
#define SVK_S1_STORE_NEW_KV(KVH, COLDECL, COL)                                                                        \
  {                                                                                                                   \
    const int ns = a.slot_mapping[b];                                                                                 \
    if (ns >= 0 && lane < 2 * DW) {                                                                                   \
      const bool is_v = lane >= DW;                                                                                   \
      const int seg = lane % DW;                                                                                      \
      COLDECL                                                                                                         \
      const uint16_t* src = (is_v ? a.new_v : a.new_k) + (int64_t)b * a.new_stride_b + (int64_t)KVH * a.new_stride_h + COL; \
      uint16_t* dst = const_cast<uint16_t*>(is_v ? a.v_cache : a.k_cache) + (int64_t)ns * a.kv_slot_stride +          \
                      (int64_t)KVH * a.kv_head_stride + COL;                                                          \
      *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(src);                                          \
    }                                                                                                                 \
  }
// Behind a fused store (plain or rotated).  Only the storing wave reads those bytes of the slot's head row in this
// launch and the CU cannot hold a stale line of it (L1 is write-through, invalidated at kernel start), so a
// workgroup-scope fence pair (= the store has completed) is enough; agent scope would write back the XCD's L2
// (+10 us per launch measured).
#define SVK_S1_STORE_FENCE()                                                                                          \
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");                                                              \
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");

// Byte addressing of the K and V rows, and the slot ids of a tile.
// OFF32: the whole K (V) tensor spans < 4 GiB, so a row address is the wave-uniform tensor base (SGPR pair) + a 32-bit
// per-lane byte offset: one VGPR per address and 32-bit integer math instead of 64-bit (frees ~20 VGPRs in the
// pipelined loop).
// fetch_slots: slot ids of one 32-token tile: lanes 0..31 fetch row[t0 + lane] (one coalesced 128 B read)
// (index clamped to the last valid token: always a legal, branch-free load - a conditional load would make the
//  compiler's vmcnt bookkeeping conservative for the whole tile body; the lane id is taken fresh so that it is not
//  hoisted out of the loop and spilled)
// (slot_page_size > 0, a power of two: `row` holds page slots, token slot = page slot * size + offset in the page)
#define SVK_S1_ADDRESSING(KVH, COL0P, VSEG)                                                                           \
  const int32_t* row = a.req_to_tokens + (int64_t)a.b_req_idx[b] * a.req_stride;                                     \
  const char* const kt = reinterpret_cast<const char*>(a.k_cache);                                                   \
  const char* const vt = reinterpret_cast<const char*>(a.v_cache);                                                   \
  const int64_t slot_bytes = a.kv_slot_stride * 2;                                                                    \
  const int64_t k_lane_bytes = ((int64_t)KVH * a.kv_head_stride + COL0P jq * 8) * 2;                                  \
  const int64_t v_lane_bytes = ((int64_t)KVH * a.kv_head_stride + COL0P VSEG * 8) * 2;                                \
  auto k_ptr = [&](int slot) -> const char* {                                                                         \
    if (OFF32) return kt + (size_t)((uint32_t)slot * (uint32_t)slot_bytes + (uint32_t)k_lane_bytes);                  \
    return kt + (int64_t)slot * slot_bytes + k_lane_bytes;                                                            \
  };                                                                                                                  \
  auto v_ptr = [&](int slot) -> const char* {                                                                         \
    if (OFF32) return vt + (size_t)((uint32_t)slot * (uint32_t)slot_bytes + (uint32_t)v_lane_bytes);                  \
    return vt + (int64_t)slot * slot_bytes + v_lane_bytes;                                                            \
  };                                                                                                                  \
  const float sm_scale = rsqrtf((float)D);                                                                            \
  const int page_shift = a.slot_page_size > 0 ? __builtin_ctz((unsigned)a.slot_page_size) : 0;                        \
  const uint32_t page_mask = (uint32_t)max(a.slot_page_size, 1) - 1u;                                                 \
  auto fetch_slots = [&](int t0_) -> int {                                                                            \
    const uint32_t t = (uint32_t)min(t0_ + (lane_id_fresh() & 31), end - 1);                                          \
    return (row[t >> page_shift] << page_shift) + (int)(t & page_mask);                                               \
  };

// K tile into kr: lane (n, jq) loads its 8-element k chunk of every 32-dim MFMA chunk of tokens n and 16 + n of SLOTS
#define SVK_S1_LOAD_K(SLOTS)                                                                                          \
  SVK_S1_UNROLL                                                                                                       \
  for (int g = 0; g < 2; ++g) {                                                                                       \
    const char* kp = k_ptr(SLOTS[g * 16 + n]);                                                                        \
    SVK_S1_UNROLL                                                                                                     \
    for (int c = 0; c < NC; ++c) kr[g][c] = ld16<false>(kp + c * 64);                                                 \
  }

// V tile into vr: vr[e] = the lane's 16-byte segment of token jq*8+e (the k index of P.V)
#define SVK_S1_LOAD_V(NT)                                                                                             \
  SVK_S1_UNROLL                                                                                                       \
  for (int e = 0; e < 8; ++e)                                                                                         \
    vr[e] = ld16<NT>(v_ptr(cur_slots[jq * 8 + e]));

// Prologue: zero P tile, slot ids of tile 0 and the wave's Q fragments (rows >= G zero) into LDS, slot ids of tile 1
// parked in a register (s_next), K(0) requested, softmax state cleared.  acc[i][r]: head jq*4+r, dim i of the lane's
// V segment.
#define SVK_S1_PROLOGUE(KVH, COL0P)                                                                                   \
  for (int i = lane; i < kPFloats; i += 64) Pw[i] = 0.f;                                                              \
  {                                                                                                                   \
    const int s0 = fetch_slots(start);                                                                                \
    if (lane < 32) slot_lds[lane] = s0;                                                                               \
    const uint16_t* qp = a.q + (int64_t)b * a.q_stride_b + (int64_t)(KVH * G + n) * a.q_stride_h + COL0P jq * 8;      \
    SVK_S1_UNROLL                                                                                                     \
    for (int c = 0; c < NC; ++c) {                                                                                    \
      uint4 t = make_uint4(0, 0, 0, 0);                                                                               \
      if (n < G) t = *reinterpret_cast<const uint4*>(qp + c * 32);                                                    \
      q_lds[c * 64 + lane] = t;                                                                                       \
    }                                                                                                                 \
  }                                                                                                                   \
  int s_next = fetch_slots(start + kTileTokens);                                                                      \
  wave_sync();                                                                                                        \
  uint4 kr[2][NC];                                                                                                    \
  SVK_S1_LOAD_K(slot_lds)                                                                                             \
  float m[4], l[4];                                                                                                   \
  SVK_S1_UNROLL                                                                                                       \
  for (int r = 0; r < 4; ++r) { m[r] = -INFINITY; l[r] = 0.f; }                                                       \
  f32x4_t acc[8];                                                                                                     \
  SVK_S1_UNROLL                                                                                                       \
  for (int i = 0; i < 8; ++i) acc[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};

// publish tile i+1's slot ids (fetched one iteration ago), fetch tile i+2's
#define SVK_S1_ADVANCE_SLOTS()                                                                                        \
  {                                                                                                                   \
    const int ln = lane_id_fresh();                                                                                   \
    if (ln < 32) nxt_slots[ln] = s_next;                                                                              \
  }                                                                                                                   \
  s_next = fetch_slots(t0 + 2 * kTileTokens);

// s = Q K^T over the wave's NC chunks of K(i): A = the <= 16 query heads, B = 2 x 16 token rows
#define SVK_S1_QK()                                                                                                   \
  f32x4_t s[2];                                                                                                       \
  {                                                                                                                   \
    bf16x8_t qa[NC];                                                                                                  \
    SVK_S1_UNROLL                                                                                                     \
    for (int c = 0; c < NC; ++c) qa[c] = __builtin_bit_cast(bf16x8_t, q_lds[c * 64 + lane]);                          \
    SVK_S1_UNROLL                                                                                                     \
    for (int g = 0; g < 2; ++g) {                                                                                     \
      s[g] = f32x4_t{0.f, 0.f, 0.f, 0.f};                                                                             \
      SVK_S1_UNROLL                                                                                                   \
      for (int c = 0; c < NC; ++c)                                                                                    \
        s[g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa[c], __builtin_bit_cast(bf16x8_t, kr[g][c]), s[g], 0, 0, 0); \
    }                                                                                                                 \
  }

// tv: which of the lane's two token columns (t0 + n, t0 + 16 + n) lie before `end`; a tile with a successor is full
#define SVK_S1_TOKEN_VALID()                                                                                          \
  bool tv[2];                                                                                                         \
  tv[0] = full || (t0 + n < end);                                                                                     \
  tv[1] = full || (t0 + 16 + n < end);

// Raw token scores of the tile.  PERHEAD: plain stores.  HEADMAX: the lane-local max over the 4 accumulator rows goes
// to the LDS score chunk `spart` [token][SP = Hkv * JQ], combined by SCORE_CHUNK_END.
#define SVK_S1_EMIT_SCORES(KVH, STATS)                                                                                \
  if constexpr (MODE == SVK_SCORE_PERHEAD) {                                                                          \
    if (STATS true) {                                                                                                 \
      SVK_S1_UNROLL                                                                                                   \
      for (int g = 0; g < 2; ++g)                                                                                     \
        SVK_S1_UNROLL                                                                                                 \
        for (int r = 0; r < 4; ++r) {                                                                                 \
          const int h = jq * 4 + r;                                                                                   \
          if (h < G && tv[g])                                                                                         \
            a.attn_score[(int64_t)b * a.score_stride_b + (int64_t)(KVH * G + h) * a.score_stride_h + t0 + g * 16 + n] = s[g][r]; \
        }                                                                                                             \
    }                                                                                                                 \
  } else if constexpr (MODE == SVK_SCORE_HEADMAX) {                                                                   \
    if (STATS jq < JQ) {                                                                                              \
      SVK_S1_UNROLL                                                                                                   \
      for (int g = 0; g < 2; ++g) {                                                                                   \
        float pm = -INFINITY;                                                                                         \
        SVK_S1_UNROLL                                                                                                 \
        for (int r = 0; r < 4; ++r)                                                                                   \
          if (jq * 4 + r < G) pm = fmaxf(pm, s[g][r]);                                                                \
        spart[(t0 - c0 + g * 16 + n) * SP + KVH * JQ + jq] = tv[g] ? pm : -INFINITY;                                  \
      }                                                                                                               \
    }                                                                                                                 \
  }

// Online-softmax step on one tile (DPP row reductions: 16 tokens live in one DPP row); `rescale`: a row maximum of
// this lane moved
#define SVK_S1_SOFTMAX_STEP()                                                                                         \
  float p[2][4];                                                                                                      \
  float alpha[4];                                                                                                     \
  bool rescale = false;                                                                                               \
  SVK_S1_UNROLL                                                                                                       \
  for (int r = 0; r < 4; ++r) {                                                                                       \
    const bool hv = (jq * 4 + r < G);                                                                                 \
    const float x0 = (hv && tv[0]) ? s[0][r] * sm_scale : -INFINITY;                                                  \
    const float x1 = (hv && tv[1]) ? s[1][r] * sm_scale : -INFINITY;                                                  \
    const float tmax = row16_allmax(fmaxf(x0, x1));                                                                   \
    const float nm = fmaxf(m[r], tmax);                                                                               \
    if (hv) {                                                                                                         \
      alpha[r] = __expf(m[r] - nm);                                                                                   \
      p[0][r] = __expf(x0 - nm);                                                                                      \
      p[1][r] = __expf(x1 - nm);                                                                                      \
      rescale |= (nm != m[r]);                                                                                        \
    } else {                                                                                                          \
      alpha[r] = 1.f; p[0][r] = 0.f; p[1][r] = 0.f;                                                                   \
    }                                                                                                                 \
    l[r] = l[r] * alpha[r] + row16_allsum(p[0][r] + p[1][r]);                                                         \
    m[r] = hv ? nm : m[r];                                                                                            \
  }

// P (rounded to bf16) into the wave's LDS tile [16 heads][kPRow], accumulator rescaled where a maximum moved
#define SVK_S1_WRITE_P_RESCALE()                                                                                      \
  if (jq < JQ) {                                                                                                      \
    SVK_S1_UNROLL                                                                                                     \
    for (int g = 0; g < 2; ++g)                                                                                       \
      SVK_S1_UNROLL                                                                                                   \
      for (int r = 0; r < 4; ++r) Pl[(jq * 4 + r) * kPRow + g * 16 + n] = (uint16_t)f32_to_bf16_bits(p[g][r]);       \
  }                                                                                                                   \
  if (__any(rescale)) {                                                                                               \
    SVK_S1_UNROLL                                                                                                     \
    for (int i = 0; i < 8; ++i)                                                                                       \
      SVK_S1_UNROLL                                                                                                   \
      for (int r = 0; r < 4; ++r) acc[i][r] *= alpha[r];                                                              \
  }

// P.V on the matrix cores: A = P [head n][tokens jq*8 .. +8] (one 16-byte LDS row read), B column n of MFMA i
// = dim i of the lane's V segment, whose 8 k-values are the i-th halves of the 8 loaded 16-byte V segments
// (vv[e * 4 + i / 2]).
#define SVK_S1_PV()                                                                                                   \
  {                                                                                                                   \
    const bf16x8_t pfrag = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(Pl + n * kPRow + jq * 8));    \
    const uint32_t* vv = reinterpret_cast<const uint32_t*>(vr);                                                       \
    SVK_S1_UNROLL                                                                                                     \
    for (int i = 0; i < 8; ++i) {                                                                                     \
      uint32_t vf[4];                                                                                                 \
      SVK_S1_UNROLL                                                                                                   \
      for (int e2 = 0; e2 < 4; ++e2)                                                                                  \
        vf[e2] = __builtin_amdgcn_perm(vv[(2 * e2 + 1) * 4 + i / 2], vv[(2 * e2) * 4 + i / 2], (i & 1) ? 0x07060302u : 0x05040100u); \
      acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pfrag, __builtin_bit_cast(bf16x8_t, make_uint4(vf[0], vf[1], vf[2], vf[3])), acc[i], 0, 0, 0); \
    }                                                                                                                 \
  }

// End of a score chunk (or of the block), HEADMAX: one owner thread per token column takes the max over the KV-head
// waves and row groups -> plain coalesced store or max-combine, no float atomics.  The condition depends on
// (t0, c0, has_next) alone, which every wave of the workgroup shares; BARRIER is the kernel's own workgroup barrier.
// `dst` is a wave-uniform base.
#define SVK_S1_SCORE_CHUNK_END(BARRIER)                                                                               \
  if (MODE == SVK_SCORE_HEADMAX && (!has_next || (t0 + kTileTokens - c0) == kScoreChunk)) {                           \
    const int c1 = min(end, t0 + kTileTokens);                                                                        \
    BARRIER();                                                                                                        \
    float* const dst = a.attn_score + (int64_t)b * a.score_stride_b + c0;                                             \
    for (uint32_t t = threadIdx.x; t < (uint32_t)(c1 - c0); t += blockDim.x) {                                        \
      float mx = -INFINITY;                                                                                           \
      for (int j = 0; j < SP; ++j) mx = fmaxf(mx, spart[t * SP + j]);                                                 \
      dst[t] = a.score_overwrite ? mx : fmaxf(dst[t], mx);                                                            \
    }                                                                                                                 \
    BARRIER();                                                                                                        \
    c0 = t0 + kTileTokens;                                                                                            \
  }

// Epilogue: lane (n, jq) owns heads jq*4+r and 8 consecutive head dims of its V segment.  The lane id is laundered
// through an empty asm so that none of the output addresses can be hoisted above the tile loop.
// GUARD / SEG: v3 at head_dim 64 has 8 segments for 16 MFMA columns: `if (n_e < DW)` / `(n_e % DW)`; d256: empty / n_e.
// direct_o: the single partial of the row IS the output: stage 2 would weight it by exp(lse - lse) = 1 and round.
#define SVK_S1_EPILOGUE(KVH, STATS, GUARD, SEG)                                                                       \
  int lane_e = lane;                                                                                                  \
  asm volatile("" : "+v"(lane_e));                                                                                    \
  const int n_e = lane_e & 15, jq_e = lane_e >> 4;                                                                    \
  if (jq_e < JQ) {                                                                                                    \
    SVK_S1_UNROLL                                                                                                     \
    for (int r = 0; r < 4; ++r) {                                                                                     \
      const int h = jq_e * 4 + r;                                                                                     \
      if (h < G) {                                                                                                    \
        if (STATS n_e == 0) mid_lse[(int64_t)(KVH * G + h) * a.mid_lse_stride_h] = m[r] + __logf(l[r]);               \
        GUARD {                                                                                                       \
          if (direct_o != nullptr) {                                                                                  \
            uint32_t pk[4];                                                                                           \
            SVK_S1_UNROLL                                                                                             \
            for (int e = 0; e < 4; ++e)                                                                               \
              pk[e] = f32_to_bf16_bits(acc[2 * e][r] / l[r]) | (f32_to_bf16_bits(acc[2 * e + 1][r] / l[r]) << 16);    \
            *reinterpret_cast<uint4*>(direct_o + (int64_t)(KVH * G + h) * a.direct_stride_h + SEG * 8) =              \
                make_uint4(pk[0], pk[1], pk[2], pk[3]);                                                               \
          } else {                                                                                                    \
            float* o = mid_o + (int64_t)(KVH * G + h) * a.mid_o_stride_h + SEG * 8;                                   \
            *reinterpret_cast<float4*>(o) = make_float4(acc[0][r] / l[r], acc[1][r] / l[r], acc[2][r] / l[r], acc[3][r] / l[r]); \
            *reinterpret_cast<float4*>(o + 4) = make_float4(acc[4][r] / l[r], acc[5][r] / l[r], acc[6][r] / l[r], acc[7][r] / l[r]); \
          }                                                                                                           \
        }                                                                                                             \
      }                                                                                                               \
    }                                                                                                                 \
  }

// ---- host side

// 32-bit row offsets whenever the caller tells us the KV tensors span < 4 GiB
inline bool stage1_off32(const SvkFlashDecodeStage1Args& a) {
  return a.kv_num_slots > 0 && (a.kv_num_slots * a.kv_slot_stride * 2) < (int64_t)0xffffffffll;
}
// floats of the HEADMAX score chunk [kScoreChunk tokens][Hkv * JQ]
template <int G>
inline size_t stage1_score_floats(const SvkFlashDecodeStage1Args& a) {
  return a.score_mode == SVK_SCORE_HEADMAX ? (size_t)kScoreChunk * a.num_kv_heads * stage1_jq(G) : 0;
}

// Run-time (G, score_mode, off32) -> template arguments: calls launch(G, MODE, OFF32) with three
// std::integral_constant values; `launch` enqueues the kernel.
template <class Launch>
int stage1_dispatch(const SvkFlashDecodeStage1Args& a, Launch&& launch) {
  const int G = a.num_q_heads / a.num_kv_heads;
  const bool off32 = stage1_off32(a);
  auto with_group = [&](auto g) {
    auto with_mode = [&](auto mode) {
      if (off32) launch(g, mode, std::true_type{});
      else launch(g, mode, std::false_type{});
    };
    if (a.score_mode == SVK_SCORE_HEADMAX) with_mode(std::integral_constant<int, SVK_SCORE_HEADMAX>{});
    else if (a.score_mode == SVK_SCORE_PERHEAD) with_mode(std::integral_constant<int, SVK_SCORE_PERHEAD>{});
    else with_mode(std::integral_constant<int, SVK_SCORE_NONE>{});
    return check_launch("svk_flash_decode_stage1");
  };
  switch (G) {
    case 1: return with_group(std::integral_constant<int, 1>{});
    case 2: return with_group(std::integral_constant<int, 2>{});
    case 3: return with_group(std::integral_constant<int, 3>{});
    case 4: return with_group(std::integral_constant<int, 4>{});
    case 5: return with_group(std::integral_constant<int, 5>{});
    case 6: return with_group(std::integral_constant<int, 6>{});
    case 7: return with_group(std::integral_constant<int, 7>{});
    case 8: return with_group(std::integral_constant<int, 8>{});
    default:
      set_error("svk_flash_decode_stage1: GQA group size %d unsupported (1..8)", G);
      return SVK_ERR_LAYOUT;
  }
}

}  // namespace
}  // namespace svk
