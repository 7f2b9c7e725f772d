// Split-KV GQA decode attention, stage 1, at head_dim 256 (Gemma-2/3, Qwen3-Next attention layers).  gfx950 only.
//
// Same contract as decode_stage1_kernel_v3 (decode_attention.hip, include/svk.h): partials mid_o = acc / l,
// mid_lse = m + log l, empty block = (0, -inf), P rounded to bf16 before P.V, raw (unscaled) token scores.
//
// Why not v3 at D = 256: its P.V mapping gives the 16 MFMA columns of a wave 8 head dims each (128 dims at most), and a
// wave that owned a whole 512-byte head row would carry kr[2][8] + 64 accumulator registers on top of 154 VGPRs.
//
// Design:
//   * one workgroup = (batch lane, block_seq block), as in v3, but TWO waves per KV head.  Wave hx of a pair owns head
//     dims [128 hx, 128 hx + 128) of its KV head for both products, so its register profile is v3's D = 128 profile and
//     a workgroup has twice the waves - what the 1- and 2-KV-head ranks typical of 256-wide models lack.  The two
//     256-byte halves of a head row are fetched by adjacent waves back to back, every K and V byte exactly once.
//   * Q.K^T: wave hx loads its half of each K row straight into the MFMA B-operand layout (4 chunks of 32 dims), its Q
//     half-fragments sit in LDS, and v_mfma_f32_16x16x32_bf16 gives a PARTIAL S of the 32-token tile.  The partial tiles
//     of a pair are exchanged through LDS (row groups jq < JQ only) and added as half 0 + half 1 in both waves: both hold
//     bit-identical S, run the identical online softmax and agree on m, l and P without further traffic.
//   * the exchange buffer is double buffered by tile parity, so ONE workgroup barrier per tile is enough: a wave
//     overwrites the buffer of tile i only after the barrier of tile i + 1, which its partner reaches after reading it.
//     The barrier is `s_waitcnt lgkmcnt(0); s_barrier`: it orders LDS traffic only and leaves the K / V loads in flight.
//   * every wave of a workgroup walks the same [start, end), so every barrier is under workgroup-uniform control flow:
//     the empty-block return happens before the first barrier, the peeled last tile and the score-chunk combine depend
//     on (start, end, t0) alone.
//   * P.V: v3's mapping unchanged on the wave's 128 V dims (acc[8]: 8 dims x 4 heads per lane).
//   * scores: wave 0 of each pair stores (PERHEAD) or writes its tile maxima into the LDS score chunk (HEADMAX), one
//     owner thread per token column combines across KV heads: store or max-combine, no float atomics.
//   * epilogue: each wave writes its 128 dims of mid_o / direct_o, wave 0 of the pair writes mid_lse.
//   * KV heads 1..4: __launch_bounds__(512); 5..8 (up to 16 waves): a second instantiation with __launch_bounds__(1024).
//
// Not carried over: the rotated form of the fused store (deltakv_view.hip is head_dim 128 only; refused by the caller).

#include <type_traits>

#include "svk_common.hpp"

namespace svk {
namespace {

constexpr int kTileTokens = 32;    // 2 MFMA column groups of 16 tokens
constexpr int kScoreChunk = 256;   // tokens between two score-combine barriers
constexpr int kPRow = 40;          // P tile row stride in bf16 (32 tokens + pad, 16-byte aligned rows)
constexpr int kPFloats = 16 * kPRow / 2;
constexpr int kHalf = 128;         // head dims per wave
constexpr int kNC = kHalf / 32;    // MFMA k-chunks per half row
constexpr int kMaxLds = 160 * 1024;

template <int G>
struct D256Lds {
  static constexpr int JQ = (G + 3) / 4;           // accumulator row groups holding real heads
  static constexpr int XCH = JQ * 16 * 2 * 4;      // one exchange buffer: JQ*16 lanes x 2 column groups x 4 rows
  // P tile (bf16) | 2 x 32 slot ids | Q half-fragments (kNC x 64 lanes x 16 B) | 2 exchange buffers
  static constexpr int WAVE_FLOATS = kPFloats + 64 + kNC * 64 * 4 + 2 * XCH;
};

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;

template <bool NT>
__device__ __forceinline__ uint4 ld16(const char* p) {
  if (NT) return __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(p)));
  return *reinterpret_cast<const uint4*>(p);
}

template <int G, int MODE, bool OFF32, int MAXT>
__global__ void __launch_bounds__(MAXT)
decode_stage1_d256_kernel(const SvkFlashDecodeStage1Args a) {
  constexpr int D = 256, NC = kNC, JQ = D256Lds<G>::JQ, XCH = D256Lds<G>::XCH;
  constexpr int WF = D256Lds<G>::WAVE_FLOATS;
  constexpr int DW = kHalf / 8;                    // 16-byte segments per half row = MFMA columns
  // 16 waves leave 128 registers per lane: K(i+1) and V(i) cannot both be in flight beside the accumulator.  The lean
  // form issues V(i) once the K registers are dead and K(i+1) once the V registers are dead; the other three waves of
  // the SIMD cover the latency a wave exposes that way.
  constexpr bool LEAN = MAXT > 512;
  extern __shared__ __attribute__((aligned(16))) float lds[];

  const int b = blockIdx.y;
  const int blk = blockIdx.x;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int kvh = w >> 1;                          // KV head of the pair
  const int hx = w & 1;                            // half of the head row this wave owns
  const int Hkv = a.num_kv_heads;
  const int n = lane & 15;
  const int jq = lane >> 4;
  constexpr int score_mode = MODE;

  const int len = a.b_seqlen[b];
  const int start = blk * a.block_seq;
  const int end = min(len, start + a.block_seq);

  // per-wave LDS
  float* Pw = lds + w * WF;
  uint16_t* Pl = reinterpret_cast<uint16_t*>(Pw);                 // [16 heads][kPRow] bf16, rows >= G stay zero
  int* slot_lds = reinterpret_cast<int*>(Pw + kPFloats);
  uint4* q_lds = reinterpret_cast<uint4*>(Pw + kPFloats + 64);
  f32x4_t* xch_mine = reinterpret_cast<f32x4_t*>(Pw + kPFloats + 64 + NC * 64 * 4);
  const f32x4_t* xch_other = reinterpret_cast<const f32x4_t*>(lds + (w ^ 1) * WF + kPFloats + 64 + NC * 64 * 4);
  float* spart = lds + 2 * Hkv * WF;
  const int SP = Hkv * JQ;

  float* mid_o = a.mid_o + (int64_t)b * a.mid_o_stride_b + (int64_t)blk * a.mid_o_stride_s + hx * kHalf;
  float* mid_lse = a.mid_lse + (int64_t)b * a.mid_lse_stride_b + blk;
  uint16_t* direct_o = a.direct_o == nullptr ? nullptr : a.direct_o + (int64_t)b * a.direct_stride_b + hx * kHalf;

  // (b, blk) are the workgroup's: every wave takes this return or none does, and no barrier has been passed yet
  if (end <= start) {
    for (int h = 0; h < G; ++h) {
      if (direct_o != nullptr) {
        for (int d = lane; d < kHalf; d += 64) direct_o[(int64_t)(kvh * G + h) * a.direct_stride_h + d] = 0;
      } else {
        float* o = mid_o + (int64_t)(kvh * G + h) * a.mid_o_stride_h;
        for (int d = lane; d < kHalf; d += 64) o[d] = 0.f;
      }
      if (hx == 0 && lane == 0) mid_lse[(int64_t)(kvh * G + h) * a.mid_lse_stride_h] = -INFINITY;
    }
    return;
  }

  if (a.new_k != nullptr && end == len) {
    // fused store_kvcache: this workgroup owns the lane's newest token.  Wave (kvh, hx) writes ITS half of the head's K
    // and V rows (2 x 16 lanes, 16 bytes each) before any read of the row; only this wave reads those bytes in this
    // launch, so the workgroup-scope fence pair of v3 (= the store has completed) is enough here as well.
    const int ns = a.slot_mapping[b];
    if (ns >= 0 && lane < 2 * DW) {
      const bool is_v = lane >= DW;
      const int seg = lane % DW;
      const int64_t col = hx * kHalf + seg * 8;
      const uint16_t* src = (is_v ? a.new_v : a.new_k) + (int64_t)b * a.new_stride_b + (int64_t)kvh * a.new_stride_h + col;
      uint16_t* dst = const_cast<uint16_t*>(is_v ? a.v_cache : a.k_cache) + (int64_t)ns * a.kv_slot_stride +
                      (int64_t)kvh * a.kv_head_stride + col;
      *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(src);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  }
  const int32_t* row = a.req_to_tokens + (int64_t)a.b_req_idx[b] * a.req_stride;
  // byte addressing; OFF32: wave-uniform tensor base + a 32-bit per-lane offset (the tensors span < 4 GiB)
  const char* const kt = reinterpret_cast<const char*>(a.k_cache);
  const char* const vt = reinterpret_cast<const char*>(a.v_cache);
  const int64_t slot_bytes = a.kv_slot_stride * 2;
  const int64_t k_lane_bytes = ((int64_t)kvh * a.kv_head_stride + hx * kHalf + jq * 8) * 2;
  const int64_t v_lane_bytes = ((int64_t)kvh * a.kv_head_stride + hx * kHalf + n * 8) * 2;
  auto k_ptr = [&](int slot) -> const char* {
    if (OFF32) return kt + (size_t)((uint32_t)slot * (uint32_t)slot_bytes + (uint32_t)k_lane_bytes);
    return kt + (int64_t)slot * slot_bytes + k_lane_bytes;
  };
  auto v_ptr = [&](int slot) -> const char* {
    if (OFF32) return vt + (size_t)((uint32_t)slot * (uint32_t)slot_bytes + (uint32_t)v_lane_bytes);
    return vt + (int64_t)slot * slot_bytes + v_lane_bytes;
  };
  const float sm_scale = rsqrtf((float)D);

  // slot ids of one 32-token tile (index clamped to the last valid token: always a legal, branch-free load)
  const int page_shift = a.slot_page_size > 0 ? __builtin_ctz((unsigned)a.slot_page_size) : 0;
  const uint32_t page_mask = (uint32_t)max(a.slot_page_size, 1) - 1u;
  auto fetch_slots = [&](int t0) -> int {
    const uint32_t t = (uint32_t)min(t0 + (lane_id_fresh() & 31), end - 1);
    return (row[t >> page_shift] << page_shift) + (int)(t & page_mask);
  };
  auto wave_sync = [&]() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  };
  // workgroup barrier over LDS traffic only: the wave's LDS writes have completed, global loads stay in flight
  auto lds_barrier = [&]() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); };

  // ---- prologue
  for (int i = lane; i < kPFloats; i += 64) Pw[i] = 0.f;
  {
    const int s0 = fetch_slots(start);
    if (lane < 32) slot_lds[lane] = s0;
    const uint16_t* qp = a.q + (int64_t)b * a.q_stride_b + (int64_t)(kvh * G + n) * a.q_stride_h + hx * kHalf + jq * 8;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      uint4 t = make_uint4(0, 0, 0, 0);
      if (n < G) t = *reinterpret_cast<const uint4*>(qp + c * 32);
      q_lds[c * 64 + lane] = t;
    }
  }
  int s_next = fetch_slots(start + kTileTokens);     // slot ids of tile 1, parked in a register
  wave_sync();
  uint4 kr[2][NC];
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    const char* kp = k_ptr(slot_lds[g * 16 + n]);
#pragma unroll
    for (int c = 0; c < NC; ++c) kr[g][c] = ld16<false>(kp + c * 64);
  }

  float m[4], l[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) { m[r] = -INFINITY; l[r] = 0.f; }
  f32x4_t acc[8];                                  // acc[i][r]: head jq*4+r, head dim hx*128 + n*8 + i
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  int c0 = start;     // first token of the current score chunk
  int buf = 0;        // parity of the tile: slot_lds half and exchange buffer in use
  int t0 = start;
  // One tile; the last one is peeled (HAS_NEXT is a compile-time flag, see v3) - for every wave of the workgroup alike.
  auto tile = [&](auto has_next_c) {
    constexpr bool has_next = decltype(has_next_c)::value;
    const bool full = has_next || (t0 + kTileTokens <= end);
    const int* cur_slots = slot_lds + buf * 32;
    int* nxt_slots = slot_lds + (buf ^ 1) * 32;

    // ---- V(i) loads: this wave's 128 dims
    uint4 vr[8];                                   // vr[e] = dims hx*128 + n*8.. of token jq*8+e (the k index of P.V)
    if constexpr (!LEAN) {
#pragma unroll
      for (int e = 0; e < 8; ++e)
        vr[e] = ld16<true>(v_ptr(cur_slots[jq * 8 + e]));
    }

    // ---- publish tile i+1's slot ids (fetched one iteration ago), fetch tile i+2's
    {
      const int ln = lane_id_fresh();
      if (ln < 32) nxt_slots[ln] = s_next;
    }
    s_next = fetch_slots(t0 + 2 * kTileTokens);

    // ---- partial S = Q[:, half] K[:, half]^T on K(i)
    f32x4_t s[2];
    {
      bf16x8_t qa[NC];
#pragma unroll
      for (int c = 0; c < NC; ++c) qa[c] = __builtin_bit_cast(bf16x8_t, q_lds[c * 64 + lane]);
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        s[g] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < NC; ++c)
          s[g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa[c], __builtin_bit_cast(bf16x8_t, kr[g][c]), s[g], 0, 0, 0);
      }
    }
    // ---- hand the partial tile to the partner wave (row groups holding real heads only)
    if (jq < JQ) {
#pragma unroll
      for (int g = 0; g < 2; ++g) xch_mine[buf * (XCH / 4) + g * (JQ * 16) + lane] = s[g];
    }
    lds_barrier();      // the pair's partials and this wave's nxt_slots are visible
    // ---- K registers are dead: re-arm them with K(i+1)
    if constexpr (has_next && !LEAN) {
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        const char* kp = k_ptr(nxt_slots[g * 16 + n]);
#pragma unroll
        for (int c = 0; c < NC; ++c) kr[g][c] = ld16<false>(kp + c * 64);
      }
    }
    // (per-head scores: their 64-bit store addresses and 32 V registers do not fit together - V(i) follows the stores)
    if constexpr (LEAN && score_mode != SVK_SCORE_PERHEAD) {
#pragma unroll
      for (int e = 0; e < 8; ++e)
        vr[e] = ld16<true>(v_ptr(cur_slots[jq * 8 + e]));
    }
    // ---- S = half 0 + half 1, in that order in both waves
    if (jq < JQ) {
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        const f32x4_t o = xch_other[buf * (XCH / 4) + g * (JQ * 16) + lane];
        const f32x4_t lo = hx == 0 ? s[g] : o, hi = hx == 0 ? o : s[g];
#pragma unroll
        for (int r = 0; r < 4; ++r) s[g][r] = add_rn(lo[r], hi[r]);
      }
    }

    bool tv[2];
    tv[0] = full || (t0 + n < end);
    tv[1] = full || (t0 + 16 + n < end);

    if constexpr (score_mode == SVK_SCORE_PERHEAD) {
      if (hx == 0) {
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int h = jq * 4 + r;
            if (h < G && tv[g])
              a.attn_score[(int64_t)b * a.score_stride_b + (int64_t)(kvh * G + h) * a.score_stride_h + t0 + g * 16 + n] = s[g][r];
          }
      }
    } else if constexpr (score_mode == SVK_SCORE_HEADMAX) {
      if (hx == 0 && jq < JQ) {
#pragma unroll
        for (int g = 0; g < 2; ++g) {
          float pm = -INFINITY;
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (jq * 4 + r < G) pm = fmaxf(pm, s[g][r]);
          spart[(t0 - c0 + g * 16 + n) * SP + kvh * JQ + jq] = tv[g] ? pm : -INFINITY;
        }
      }
    }
    if constexpr (LEAN && score_mode == SVK_SCORE_PERHEAD) {
#pragma unroll
      for (int e = 0; e < 8; ++e)
        vr[e] = ld16<true>(v_ptr(cur_slots[jq * 8 + e]));
    }

    float p[2][4];
    float alpha[4];
    bool rescale = false;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool hv = (jq * 4 + r < G);
      const float x0 = (hv && tv[0]) ? s[0][r] * sm_scale : -INFINITY;
      const float x1 = (hv && tv[1]) ? s[1][r] * sm_scale : -INFINITY;
      const float tmax = row16_allmax(fmaxf(x0, x1));
      const float nm = fmaxf(m[r], tmax);
      if (hv) {
        alpha[r] = __expf(m[r] - nm);
        p[0][r] = __expf(x0 - nm);
        p[1][r] = __expf(x1 - nm);
        rescale |= (nm != m[r]);
      } else {
        alpha[r] = 1.f; p[0][r] = 0.f; p[1][r] = 0.f;
      }
      l[r] = l[r] * alpha[r] + row16_allsum(p[0][r] + p[1][r]);
      m[r] = hv ? nm : m[r];
    }

    if (jq < JQ) {
#pragma unroll
      for (int g = 0; g < 2; ++g)
#pragma unroll
        for (int r = 0; r < 4; ++r) Pl[(jq * 4 + r) * kPRow + g * 16 + n] = (uint16_t)f32_to_bf16_bits(p[g][r]);
    }
    if (__any(rescale)) {
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[i][r] *= alpha[r];
    }
    wave_sync();

    // P.V on the matrix cores, v3's mapping: A = P [head n][tokens jq*8 .. +8], B column n of MFMA i = head dim
    // hx*128 + n*8 + i, whose 8 k-values are the i-th halves of the 8 loaded 16-byte V segments.
    {
      const bf16x8_t pfrag = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(Pl + n * kPRow + jq * 8));
      const uint32_t* vv = reinterpret_cast<const uint32_t*>(vr);            // vv[e * 4 + i / 2]
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        uint32_t vf[4];
#pragma unroll
        for (int e2 = 0; e2 < 4; ++e2)
          vf[e2] = __builtin_amdgcn_perm(vv[(2 * e2 + 1) * 4 + i / 2], vv[(2 * e2) * 4 + i / 2], (i & 1) ? 0x07060302u : 0x05040100u);
        acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pfrag, __builtin_bit_cast(bf16x8_t, make_uint4(vf[0], vf[1], vf[2], vf[3])), acc[i], 0, 0, 0);
      }
    }
    wave_sync();
    if constexpr (has_next && LEAN) {
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        const char* kp = k_ptr(nxt_slots[g * 16 + n]);
#pragma unroll
        for (int c = 0; c < NC; ++c) kr[g][c] = ld16<false>(kp + c * 64);
      }
    }

    // ---- end of a score chunk (or of the block): one owner thread per token column.  The condition depends on
    // (t0, c0, has_next) alone, which every wave of the workgroup shares.
    if (score_mode == SVK_SCORE_HEADMAX && (!has_next || (t0 + kTileTokens - c0) == kScoreChunk)) {
      const int c1 = min(end, t0 + kTileTokens);
      lds_barrier();
      float* const dst = a.attn_score + (int64_t)b * a.score_stride_b + c0;     // wave-uniform base
      for (uint32_t t = threadIdx.x; t < (uint32_t)(c1 - c0); t += blockDim.x) {
        float mx = -INFINITY;
        for (int j = 0; j < SP; ++j) mx = fmaxf(mx, spart[t * SP + j]);
        dst[t] = a.score_overwrite ? mx : fmaxf(dst[t], mx);
      }
      lds_barrier();
      c0 = t0 + kTileTokens;
    }
    t0 += kTileTokens;
    buf ^= 1;
  };
  while (t0 + kTileTokens < end) tile(std::true_type{});
  tile(std::false_type{});

  // ---- epilogue: lane (n, jq) owns heads jq*4+r and head dims hx*128 + n*8 .. +8 (lane id laundered as in v3)
  int lane_e = lane;
  asm volatile("" : "+v"(lane_e));
  const int n_e = lane_e & 15, jq_e = lane_e >> 4;
  if (jq_e < JQ) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int h = jq_e * 4 + r;
      if (h < G) {
        if (hx == 0 && n_e == 0) mid_lse[(int64_t)(kvh * G + h) * a.mid_lse_stride_h] = m[r] + __logf(l[r]);
        if (direct_o != nullptr) {
          // the single partial of the row IS the output: stage 2 would weight it by exp(lse - lse) = 1 and round
          uint32_t pk[4];
#pragma unroll
          for (int e = 0; e < 4; ++e)
            pk[e] = f32_to_bf16_bits(acc[2 * e][r] / l[r]) | (f32_to_bf16_bits(acc[2 * e + 1][r] / l[r]) << 16);
          *reinterpret_cast<uint4*>(direct_o + (int64_t)(kvh * G + h) * a.direct_stride_h + n_e * 8) =
              make_uint4(pk[0], pk[1], pk[2], pk[3]);
        } else {
          float* o = mid_o + (int64_t)(kvh * G + h) * a.mid_o_stride_h + n_e * 8;
          *reinterpret_cast<float4*>(o) = make_float4(acc[0][r] / l[r], acc[1][r] / l[r], acc[2][r] / l[r], acc[3][r] / l[r]);
          *reinterpret_cast<float4*>(o + 4) = make_float4(acc[4][r] / l[r], acc[5][r] / l[r], acc[6][r] / l[r], acc[7][r] / l[r]);
        }
      }
    }
  }
}

template <int G, int MAXT>
int launch_d256(const SvkFlashDecodeStage1Args& a, hipStream_t stream) {
  constexpr int JQ = D256Lds<G>::JQ;
  const int nblk = (a.max_len_in_batch + a.block_seq - 1) / a.block_seq;
  dim3 grid(nblk, a.batch);
  dim3 block(128 * a.num_kv_heads);                  // two waves per KV head
  const size_t score_floats = a.score_mode == SVK_SCORE_HEADMAX ? (size_t)kScoreChunk * a.num_kv_heads * JQ : 0;
  const size_t shm = sizeof(float) * ((size_t)2 * a.num_kv_heads * D256Lds<G>::WAVE_FLOATS + score_floats);
  const bool off32 = a.kv_num_slots > 0 && (a.kv_num_slots * a.kv_slot_stride * 2) < (int64_t)0xffffffffll;
  // 5..8 KV heads (and 4 with head-max scores) need more than the 64 KiB of dynamic LDS a kernel may use by default
#define SVK_LAUNCH_D256(MODE_, OFF32_)                                                                                  \
  do {                                                                                                                  \
    auto kern = decode_stage1_d256_kernel<G, MODE_, OFF32_, MAXT>;                                                      \
    static bool wide_lds = false;                                                                                       \
    if (shm > 64 * 1024 && !wide_lds) {                                                                                 \
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds); \
      wide_lds = true;                                                                                                  \
    }                                                                                                                   \
    hipLaunchKernelGGL(kern, grid, block, shm, stream, a);                                                              \
  } while (0)
#define SVK_LAUNCH_D256_MODE(MODE_)             \
  do {                                          \
    if (off32) SVK_LAUNCH_D256(MODE_, true);    \
    else SVK_LAUNCH_D256(MODE_, false);         \
  } while (0)
  if (a.score_mode == SVK_SCORE_HEADMAX) SVK_LAUNCH_D256_MODE(SVK_SCORE_HEADMAX);
  else if (a.score_mode == SVK_SCORE_PERHEAD) SVK_LAUNCH_D256_MODE(SVK_SCORE_PERHEAD);
  else SVK_LAUNCH_D256_MODE(SVK_SCORE_NONE);
#undef SVK_LAUNCH_D256_MODE
#undef SVK_LAUNCH_D256
  return check_launch("svk_flash_decode_stage1");
}

template <int MAXT>
int dispatch_group_d256(const SvkFlashDecodeStage1Args& a, int G, hipStream_t stream) {
  switch (G) {
    case 1: return launch_d256<1, MAXT>(a, stream);
    case 2: return launch_d256<2, MAXT>(a, stream);
    case 3: return launch_d256<3, MAXT>(a, stream);
    case 4: return launch_d256<4, MAXT>(a, stream);
    case 5: return launch_d256<5, MAXT>(a, stream);
    case 6: return launch_d256<6, MAXT>(a, stream);
    case 7: return launch_d256<7, MAXT>(a, stream);
    case 8: return launch_d256<8, MAXT>(a, stream);
    default:
      set_error("svk_flash_decode_stage1: GQA group size %d unsupported (1..8)", G);
      return SVK_ERR_LAYOUT;
  }
}

}  // namespace

// validated by svk_flash_decode_stage1 (decode_attention.hip): head_dim 256, 1..8 KV heads, no rotated store
int launch_flash_decode_stage1_d256(const SvkFlashDecodeStage1Args& a, hipStream_t stream) {
  const int G = a.num_q_heads / a.num_kv_heads;
  return a.num_kv_heads <= 4 ? dispatch_group_d256<512>(a, G, stream) : dispatch_group_d256<1024>(a, G, stream);
}

}  // namespace svk
