// Split-KV GQA decode attention over a token-granular paged KV cache, with the H2O /
// SnapKV token-score fused into stage 1.  gfx950 (MI355X) only.
//
// Replaces (include/svk.h cites the exact lines)
//   kernels/triton/gqa_flash_decoding_stage1.py  flash_decode_stage1{,_with_score}
//   kernels/triton/flash_decoding_stage2.py      flash_decode_stage2
//
// Design (DESIGN.md "decode stage 1"):
//   * one workgroup = (batch lane, block_seq block); one WAVE per KV head, so the four
//     256-byte head segments of each 1 KiB token row are fetched by the four waves of one
//     workgroup back to back (same DRAM page), every byte exactly once;
//   * Q.K^T on the matrix cores: v_mfma_f32_16x16x32_bf16 with A = the <=16 query heads
//     of the GQA group (rows >= G are zero) and B = 16 token rows loaded straight from
//     HBM in the B-operand layout (lane = (token, 8-element k chunk)), fp32 accumulate
//     like the reference's tl.dot;
//   * per-token score = max over heads of the raw logit: lane-local max over the 4
//     accumulator rows, then combined across the row groups and the KV-head waves
//     through LDS by ONE owner thread per token column -> plain coalesced store, no
//     float atomics (the reference issues 4 contended atomic_max per token);
//   * online softmax statistics with DPP row reductions (16 tokens live in one DPP row);
//   * P.V on the matrix cores as well: P (rounded to bf16 like `exp_logic.to(v.dtype)`) goes through a 1.25 KiB
//     per-wave LDS tile whose rows are the A operand, V rows are read as 16-byte segments in the B-operand token order.
//
// The pieces of the tile body live in decode_stage1_tile.hpp, one copy for this kernel and the head_dim 256 kernel of
// decode_attention_d256.hip: empty-block fill, plain fused store and its fence pair, K / V addressing, slot fetch,
// prologue, K and V tile loads, Q.K^T, score emission, online softmax, P write and rescale, P.V, the HEADMAX chunk
// combine, the epilogue and the host-side dispatch.  The device pieces are statement macros (SVK_S1_*) over this
// kernel's locals - the header says why and lists the names.  This file keeps v3's LDS layout, the order in which v3
// composes the pieces, the rotated store with its early loads, and stage 2.

#include <stdlib.h>

#include "decode_stage1_tile.hpp"
#include "rope_row.hpp"
#include "svk_select.hpp"

namespace svk {
namespace {

template <int D, int G>
struct Stage1Cfg {
  static constexpr int NC = D / 32;          // MFMA k-chunks per head row
  static constexpr int JQ = stage1_jq(G);
};

template <int D, int G>
struct Stage1V3Lds {
  // P tile (bf16) + 64 slot ids + Q fragments (NC x 64 lanes x 16 B)
  static constexpr int WAVE_FLOATS = kPFloats + 64 + Stage1Cfg<D, G>::NC * 64 * 4;
};

// ---------------------------------------------------------------------------------------
// v3 = v2's pipeline with P.V on the matrix cores as well: V rows are loaded as 16-byte segments in the B-operand
// token order (lane (n, jq): 8 head dims n*8.. of tokens jq*8+e) and the 8 MFMAs of a tile pick column
// "head dim n*8+i" with a byte permute, so the accumulator of a lane is 8 consecutive head dims of 4 heads
// (32 registers for any GQA group size, no cross-lane reduction in the epilogue).  The vector ALUs are left with
// the softmax only (v2 spent ~75 % of its VALU issue slots on the P.V FMAs).
// ---------------------------------------------------------------------------------------
template <int D, int G, int MODE, bool NTV, bool OFF32>
__global__ void __launch_bounds__(512)
decode_stage1_kernel_v3(const SvkFlashDecodeStage1Args a) {
  using C = Stage1Cfg<D, G>;
  constexpr int NC = C::NC, JQ = C::JQ;
  constexpr int WF = Stage1V3Lds<D, G>::WAVE_FLOATS;
  constexpr int DW = D / 8;                       // 16-byte segments per head row
  extern __shared__ __attribute__((aligned(16))) float lds[];

  const int b = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int Hkv = a.num_kv_heads;
  const int blk = blockIdx.x;
  const int n = lane & 15;
  const int jq = lane >> 4;
  const int dg = n % DW;                           // V: 16-byte segment (8 head dims) of this lane's MFMA column

  const int len = a.b_seqlen[b];
  // rotated form of the fused store (unscored launches): what it needs and what depends on nothing but (b, w, lane) is
  // requested here, beside the row length - the owner of the newest token then has one round trip (cos | sin and its
  // view slot) between the length and its stores instead of four
  bool rotated = false;
  int rot_ns = -1, rot_len = 0;
  uint4 rot_k1 = make_uint4(0, 0, 0, 0), rot_k2 = rot_k1, rot_v1 = rot_k1, rot_v2 = rot_k1;
  if constexpr (MODE == SVK_SCORE_NONE) {
    rotated = a.new_cos_sin != nullptr;
    if (rotated) {
      rot_ns = a.slot_mapping[b];
      if (a.new_row_lens != nullptr) rot_len = a.new_row_lens[b];
      if (lane < D / 16) {
        const int64_t src = (int64_t)b * a.new_stride_b + (int64_t)w * a.new_stride_h + lane * 8;
        rot_k1 = *reinterpret_cast<const uint4*>(a.new_k + src);
        rot_k2 = *reinterpret_cast<const uint4*>(a.new_k + src + D / 2);
        rot_v1 = *reinterpret_cast<const uint4*>(a.new_v + src);
        rot_v2 = *reinterpret_cast<const uint4*>(a.new_v + src + D / 2);
      }
    }
  }
  const int start = blk * a.block_seq;
  const int end = min(len, start + a.block_seq);

  // per-wave LDS: P tile | 16-float broadcast pad | 2 x 32 slot ids | Q fragments (lane-linear)
  float* Pw = lds + w * WF;
  uint16_t* Pl = reinterpret_cast<uint16_t*>(Pw);                 // [16 heads][kPRow] bf16, rows >= G stay zero
  int* slot_lds = reinterpret_cast<int*>(Pw + kPFloats);
  uint4* q_lds = reinterpret_cast<uint4*>(Pw + kPFloats + 64);
  float* spart = lds + Hkv * WF;
  const int SP = Hkv * JQ;

  SVK_S1_OUT_PTRS()
  if (end <= start) {
    SVK_S1_FILL_EMPTY(w, D, )
    return;
  }

  if (a.new_k != nullptr && end == len) {
    // fused store_kvcache: this workgroup owns the lane's newest token.  Wave w writes its kv head's K and V rows
    // before any read of the row, in the rotated form below or the plain one.
    if (rotated) {
      if constexpr (MODE == SVK_SCORE_NONE) {
        // rotated store (include/svk.h): the raw rows go to the pre-RoPE cache, the view's row of position len-1 gets
        // the k-normed, rotated key - lane j < D/16 owns elements 8j.. and their rotate-half partners, exactly as in
        // the view launch (rope_row.hpp), V rides with the same lanes.  Rows, slot and position were requested
        // above, beside the row length.
        constexpr int HD2 = D / 2, LPH = HD2 / 8;
        if (rot_ns >= 0 && rot_ns < a.raw_num_slots && lane < LPH) {
          const int p = lane * 8;
          const int vslot = a.req_to_tokens[(int64_t)a.b_req_idx[b] * a.req_stride + (len - 1)];
          const int pos = max(a.new_row_lens != nullptr ? rot_len - 1 : a.new_slot_to_pos[rot_ns], 0);
          float n1[8], n2[8];
          rope_row_norm<D>(rot_k1, rot_k2, a.new_k_norm_weight, a.new_k_norm_eps, p, n1, n2);
          uint4 o1, o2;
          rope_row_rotate<D>(n1, n2, a.new_cos_sin, (int64_t)pos * a.new_cos_stride, a.new_cos_dtype, p, o1, o2);
          const int64_t rd = (int64_t)rot_ns * a.raw_slot_stride + (int64_t)w * a.raw_head_stride + p;
          *reinterpret_cast<uint4*>(a.raw_k_cache + rd) = rot_k1;
          *reinterpret_cast<uint4*>(a.raw_k_cache + rd + HD2) = rot_k2;
          *reinterpret_cast<uint4*>(a.raw_v_cache + rd) = rot_v1;
          *reinterpret_cast<uint4*>(a.raw_v_cache + rd + HD2) = rot_v2;
          const int64_t vd = (int64_t)vslot * a.kv_slot_stride + (int64_t)w * a.kv_head_stride + p;
          *reinterpret_cast<uint4*>(const_cast<uint16_t*>(a.k_cache) + vd) = o1;
          *reinterpret_cast<uint4*>(const_cast<uint16_t*>(a.k_cache) + vd + HD2) = o2;
          *reinterpret_cast<uint4*>(const_cast<uint16_t*>(a.v_cache) + vd) = rot_v1;
          *reinterpret_cast<uint4*>(const_cast<uint16_t*>(a.v_cache) + vd + HD2) = rot_v2;
        }
      }
    } else
      SVK_S1_STORE_NEW_KV(w, , seg * 8)
    SVK_S1_STORE_FENCE()
  }
  SVK_S1_ADDRESSING(w, , dg)
  SVK_S1_PROLOGUE(w, )                             // acc[i][r]: head jq*4+r, head dim dg*8+i

  int c0 = start;     // first token of the current score chunk
  int buf = 0;        // slot_lds half holding the current tile's ids
  int t0 = start;
  // One tile.  HAS_NEXT is a compile-time flag (the last tile is peeled) so that the K(i+1)
  // re-arm is straight-line code: behind a run-time branch the compiler must assume the loads
  // may not have been issued and turns every later vmcnt(N) into a wait for K(i+1) itself.
  auto tile = [&](auto has_next_c) {
    constexpr bool has_next = decltype(has_next_c)::value;
    const bool full = has_next || (t0 + kTileTokens <= end);
    const int* cur_slots = slot_lds + buf * 32;
    int* nxt_slots = slot_lds + (buf ^ 1) * 32;

    // ---- V(i) loads (slot ids from LDS)
    uint4 vr[8];                                   // vr[e] = dims dg*8.. of token jq*8+e (the k index of P.V)
    SVK_S1_LOAD_V(NTV)

    SVK_S1_ADVANCE_SLOTS()

    // ---- S = Q K^T on K(i)
    SVK_S1_QK()
    wave_sync();        // nxt_slots visible to every lane of this wave
    // ---- K registers are dead: re-arm them with K(i+1)
    if constexpr (has_next) {
      SVK_S1_LOAD_K(nxt_slots)
    }

    SVK_S1_TOKEN_VALID()
    SVK_S1_EMIT_SCORES(w, )

    SVK_S1_SOFTMAX_STEP()
    SVK_S1_WRITE_P_RESCALE()
    wave_sync();
    SVK_S1_PV()                                    // B column n of MFMA i = head dim dg*8+i
    wave_sync();

    SVK_S1_SCORE_CHUNK_END(__syncthreads)
    t0 += kTileTokens;
    buf ^= 1;
  };
  while (t0 + kTileTokens < end) tile(std::true_type{});
  tile(std::false_type{});

  SVK_S1_EPILOGUE(w, , if (n_e < DW), (n_e % DW))
}

template <int D, int THREADS>
__global__ void __launch_bounds__(THREADS)
decode_stage2_kernel(const SvkFlashDecodeStage2Args a) {
  // one (batch lane, q head) per workgroup.  D/4 lanes cover one partial row with 16-byte loads; the THREADS/(D/4)
  // lane groups walk the split-KV partials interleaved (long contexts have ~1000 of them).  The row's maximum lse is
  // found first, so the weighted sum has no loop-carried exp chain and the partial loads stay in flight together
  // (the online form cost one HBM latency per partial: 41 us at 1025 partials).
  constexpr int LPR = D / 4, GROUPS = THREADS / LPR, WAVES = THREADS / 64;
  __shared__ float s_red[WAVES], s_l[GROUPS];
  __shared__ __attribute__((aligned(16))) float s_acc[GROUPS][D];
  const int b = blockIdx.x, h = blockIdx.y;
  const int g = threadIdx.x / LPR, d = (threadIdx.x % LPR) * 4;
  const int len = a.b_seqlen[b];
  const int nblk = len <= 0 ? 0 : (len + a.block_seq - 1) / a.block_seq + a.extra_partials;
  const float* mo = a.mid_o + (int64_t)b * a.mid_o_stride_b + (int64_t)h * a.mid_o_stride_h + d;
  const float* ml = a.mid_lse + (int64_t)b * a.mid_lse_stride_b + (int64_t)h * a.mid_lse_stride_h;
  // the first kPre partial rows of this lane group (and their lse) are requested BEFORE the row maximum is reduced: they do
  // not depend on it, and a launch of a few dozen partials is otherwise two dependent round trips (lse -> maximum ->
  // partials) of ~1.2 us each in a 4.7 us launch.  Same partials, same order, same arithmetic.
  constexpr int kPre = 8;
  float4 tvp[kPre];
  float lvp[kPre];
#pragma unroll
  for (int j = 0; j < kPre; ++j) {
    const int i = g + j * GROUPS;
    tvp[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    lvp[j] = 0.f;
    if (i < nblk) {
      tvp[j] = *reinterpret_cast<const float4*>(mo + (int64_t)i * a.mid_o_stride_s);
      lvp[j] = ml[i];
    }
  }
  float mx = -INFINITY;
  for (int i = threadIdx.x; i < nblk; i += THREADS) mx = fmaxf(mx, ml[i]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
  if constexpr (WAVES > 1) {
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = mx;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < WAVES; ++w) mx = fmaxf(mx, s_red[w]);
  }
  float sum = 0.f;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int j = 0; j < kPre; ++j) {
    if (g + j * GROUPS < nblk) {
      const float e = __expf(lvp[j] - mx);
      acc.x += e * tvp[j].x; acc.y += e * tvp[j].y; acc.z += e * tvp[j].z; acc.w += e * tvp[j].w;
      sum += e;
    }
  }
#pragma unroll 4
  for (int i = g + kPre * GROUPS; i < nblk; i += GROUPS) {
    const float4 tv = *reinterpret_cast<const float4*>(mo + (int64_t)i * a.mid_o_stride_s);
    const float e = __expf(ml[i] - mx);
    acc.x += e * tv.x; acc.y += e * tv.y; acc.z += e * tv.z; acc.w += e * tv.w;
    sum += e;
  }
  if (nblk > 1) {
    if (d == 0) s_l[g] = sum;
    *reinterpret_cast<float4*>(&s_acc[g][d]) = acc;
    __syncthreads();
    if constexpr (GROUPS > 8) {
      // two levels (1024 threads, 32 lane groups): every eighth group adds up its seven followers, then group 0 the
      // leaders - 7 + 3 dependent LDS reads instead of 31 (groups beyond the partial count hold zeros)
      if ((g & 7) == 0) {
#pragma unroll
        for (int j = 1; j < 8; ++j) {
          const float4 tv = *reinterpret_cast<const float4*>(&s_acc[g + j][d]);
          acc.x += tv.x; acc.y += tv.y; acc.z += tv.z; acc.w += tv.w;
          sum += s_l[g + j];
        }
        if (g != 0) {
          *reinterpret_cast<float4*>(&s_acc[g][d]) = acc;
          if (d == 0) s_l[g] = sum;
        }
      }
      __syncthreads();
      if (g != 0) return;
#pragma unroll
      for (int j = 8; j < GROUPS; j += 8) {
        const float4 tv = *reinterpret_cast<const float4*>(&s_acc[j][d]);
        acc.x += tv.x; acc.y += tv.y; acc.z += tv.z; acc.w += tv.w;
        sum += s_l[j];
      }
    } else {
      if (g != 0) return;
      const int used = min(nblk, GROUPS);
      for (int j = 1; j < used; ++j) {
        const float4 tv = *reinterpret_cast<const float4*>(&s_acc[j][d]);
        acc.x += tv.x; acc.y += tv.y; acc.z += tv.z; acc.w += tv.w;
        sum += s_l[j];
      }
    }
  } else if (g != 0) {
    return;
  }
  const uint32_t w0 = f32_to_bf16_bits(acc.x / sum) | (f32_to_bf16_bits(acc.y / sum) << 16);
  const uint32_t w1 = f32_to_bf16_bits(acc.z / sum) | (f32_to_bf16_bits(acc.w / sum) << 16);
  *reinterpret_cast<uint2*>(a.o + (int64_t)b * a.o_stride_b + (int64_t)h * a.o_stride_h + d) = make_uint2(w0, w1);
}

// ---- two-level merge (launches with many partials per row: KIVI full layers at 256 k tokens, one-row launches)
// The one-level kernel above gives a (row, head) ONE workgroup: 259 partials x 516 B are 134 KB through one CU, 28
// workgroups on a 256-CU chip - 29 us per KIVI layer at 1 x 256 k, 11 % of a DeltaKV decode step.  Here workgroup
// (b, h, s) merges the kSplitPPW partials [s * kSplitPPW, ...) into a second-level partial of the same form (normalised
// row + lse) in the caller's workspace, takes a ticket, and the LAST workgroup of the (b, h) to arrive merges the
// second-level partials in index order - whoever that is, the sums are formed in the same order - and writes the output.
// Tickets are the caller's [batch * heads] int32 (zero before the first launch; the last arriver leaves its ticket at zero
// again) - NOT part of the scratch, whose layout moves with the launch shape.
constexpr int kSplitPPW = 32;          // partials per first-level workgroup
constexpr int kSplitMin = 256;         // launches that may merge more partials than this per row take the two-level form

__host__ __device__ inline int64_t split_align(int64_t x) { return (x + 255) & ~(int64_t)255; }
__host__ __device__ inline int split_groups(int max_partials) { return (max_partials + kSplitPPW - 1) / kSplitPPW; }

template <int D>
__global__ void __launch_bounds__(256)
decode_stage2_split_kernel(const SvkFlashDecodeStage2Args a) {
  constexpr int THREADS = 256, LPR = D / 4, GROUPS = THREADS / LPR, WAVES = THREADS / 64, KPRE = kSplitPPW / GROUPS;
  static_assert(kSplitPPW % GROUPS == 0, "a workgroup's partials are whole rounds of its lane groups");
  __shared__ float s_red[WAVES], s_l[GROUPS];
  __shared__ __attribute__((aligned(16))) float s_acc[GROUPS][D];
  __shared__ int s_last;
  const int b = blockIdx.x, h = blockIdx.y, s = blockIdx.z;
  const int g = threadIdx.x / LPR, d = (threadIdx.x % LPR) * 4;
  const int len = a.b_seqlen[b];
  const int nblk = len <= 0 ? 0 : (len + a.block_seq - 1) / a.block_seq + a.extra_partials;
  const int s_row = max(1, (nblk + kSplitPPW - 1) / kSplitPPW);       // first-level workgroups this row needs
  if (s >= s_row) return;
  const int smax = split_groups(a.max_partials);
  const int64_t n_bh = (int64_t)gridDim.x * gridDim.y, bh = (int64_t)b * gridDim.y + h;
  unsigned char* ws = static_cast<unsigned char*>(a.split_ws);
  int* tickets = a.split_tickets;
  float* ws_lse = reinterpret_cast<float*>(ws) + bh * smax;
  float* ws_o = reinterpret_cast<float*>(ws + split_align(n_bh * smax * 4)) + bh * smax * D;
  const float* mo = a.mid_o + (int64_t)b * a.mid_o_stride_b + (int64_t)h * a.mid_o_stride_h + d;
  const float* ml = a.mid_lse + (int64_t)b * a.mid_lse_stride_b + (int64_t)h * a.mid_lse_stride_h;
  int64_t stride = a.mid_o_stride_s;
  int first = s * kSplitPPW, count = min(nblk - first, kSplitPPW);
  for (int level = 0; level < 2; ++level) {
    // merge rows [first, first + count) of (mo, ml): all loads of the round in flight together, the maximum reduced under them
    float4 tv[KPRE];
    float lv[KPRE];
#pragma unroll
    for (int j = 0; j < KPRE; ++j) {
      const int i = g + j * GROUPS;
      tv[j] = make_float4(0.f, 0.f, 0.f, 0.f);
      lv[j] = -INFINITY;
      if (i < count) {
        if (level == 0) {
          tv[j] = *reinterpret_cast<const float4*>(mo + (int64_t)(first + i) * stride);
          lv[j] = ml[first + i];
        } else {
          // other workgroups' second-level partials: agent-scope (sc1) loads - coherent across CUs and XCDs without an
          // acquire fence (1.7 us) in front of them
          uint64_t* p = reinterpret_cast<uint64_t*>(const_cast<float*>(mo) + (int64_t)(first + i) * stride);
          const uint64_t x0 = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          const uint64_t x1 = __hip_atomic_load(p + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          tv[j] = make_float4(__uint_as_float((uint32_t)x0), __uint_as_float((uint32_t)(x0 >> 32)),
                              __uint_as_float((uint32_t)x1), __uint_as_float((uint32_t)(x1 >> 32)));
          lv[j] = __uint_as_float(__hip_atomic_load(reinterpret_cast<uint32_t*>(const_cast<float*>(ml)) + first + i,
                                                    __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        }
      }
    }
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < KPRE; ++j) mx = fmaxf(mx, lv[j]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = mx;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < WAVES; ++w) mx = fmaxf(mx, s_red[w]);
    float sum = 0.f;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int j = 0; j < KPRE; ++j) {
      if (g + j * GROUPS < count) {
        const float e = __expf(lv[j] - mx);
        acc.x += e * tv[j].x; acc.y += e * tv[j].y; acc.z += e * tv[j].z; acc.w += e * tv[j].w;
        sum += e;
      }
    }
    if (d == 0) s_l[g] = sum;
    *reinterpret_cast<float4*>(&s_acc[g][d]) = acc;
    __syncthreads();
    if (g == 0) {
      const int used = min(max(count, 1), GROUPS);
      for (int j = 1; j < used; ++j) {
        const float4 t2 = *reinterpret_cast<const float4*>(&s_acc[j][d]);
        acc.x += t2.x; acc.y += t2.y; acc.z += t2.z; acc.w += t2.w;
        sum += s_l[j];
      }
      if (level == 1 || s_row == 1) {
        const uint32_t w0 = f32_to_bf16_bits(acc.x / sum) | (f32_to_bf16_bits(acc.y / sum) << 16);
        const uint32_t w1 = f32_to_bf16_bits(acc.z / sum) | (f32_to_bf16_bits(acc.w / sum) << 16);
        *reinterpret_cast<uint2*>(a.o + (int64_t)b * a.o_stride_b + (int64_t)h * a.o_stride_h + d) = make_uint2(w0, w1);
      } else {
        // write-through (sc1) stores: visible to every CU / XCD once they have completed - no release fence, whose L2
        // write-back of everything stage 1 has just written cost 13 us per launch
        uint64_t* p = reinterpret_cast<uint64_t*>(ws_o + (int64_t)s * D + d);
        const float o0 = acc.x / sum, o1 = acc.y / sum, o2 = acc.z / sum, o3 = acc.w / sum;
        __hip_atomic_store(p, (uint64_t)__float_as_uint(o0) | ((uint64_t)__float_as_uint(o1) << 32), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(p + 1, (uint64_t)__float_as_uint(o2) | ((uint64_t)__float_as_uint(o3) << 32), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
        if (d == 0)
          __hip_atomic_store(reinterpret_cast<uint32_t*>(ws_lse) + s, __float_as_uint(mx + __logf(sum)), __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    if (level == 1 || s_row == 1) return;
    // hand-over (cdna_hip_programming.md, guideline 16, R1): every storing wave drains its stores, then ONE lane takes the
    // ticket; the last arriver reads the others' partials with agent-scope loads
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0)
      s_last = __hip_atomic_fetch_add(&tickets[bh], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == s_row - 1;
    __syncthreads();
    if (!s_last) return;
    if (threadIdx.x == 0) __hip_atomic_store(&tickets[bh], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // self-cleaning
    mo = ws_o + d;
    ml = ws_lse;
    stride = D;
    first = 0;
    count = s_row;                                     // <= kSplitPPW (checked by the launcher)
  }
}

template <int D>
int launch_stage1(const SvkFlashDecodeStage1Args& a, hipStream_t stream) {
  const int nblk = (a.max_len_in_batch + a.block_seq - 1) / a.block_seq;
  dim3 grid(nblk, a.batch);
  dim3 block(64 * a.num_kv_heads);
  return stage1_dispatch(a, [&](auto g, auto mode, auto off32) {
    constexpr int G = decltype(g)::value;
    const size_t shm3 = sizeof(float) * ((size_t)a.num_kv_heads * Stage1V3Lds<D, G>::WAVE_FLOATS + stage1_score_floats<G>(a));
    hipLaunchKernelGGL((decode_stage1_kernel_v3<D, G, decltype(mode)::value, true, decltype(off32)::value>), grid, block, shm3,
                       stream, a);
  });
}

}  // namespace

// head_dim 256: the two-waves-per-KV-head kernel of decode_attention_d256.hip
int launch_flash_decode_stage1_d256(const SvkFlashDecodeStage1Args& a, hipStream_t stream);
}  // namespace svk

static int validate_stage1(const SvkFlashDecodeStage1Args* a, const char* who) {
  using namespace svk;
  SVK_REQUIRE(a != nullptr, SVK_ERR_VALUE, "%s: null args", who);
  SVK_REQUIRE(a->head_dim == 64 || a->head_dim == 128 || a->head_dim == 256, SVK_ERR_LAYOUT,
              "%s: head_dim %d unsupported (64, 128, 256)", who, a->head_dim);
  SVK_REQUIRE(a->block_seq > 0 && a->block_seq % 16 == 0, SVK_ERR_LAYOUT,
              "%s: block_seq %d must be a positive multiple of 16 (BLOCK_SEQ %% BLOCK_N)", who, a->block_seq);
  SVK_REQUIRE(a->num_kv_heads >= 1 && a->num_kv_heads <= 8, SVK_ERR_LAYOUT, "%s: num_kv_heads %d unsupported (1..8 per rank)", who,
              a->num_kv_heads);
  SVK_REQUIRE(a->num_q_heads % a->num_kv_heads == 0, SVK_ERR_LAYOUT, "%s: q heads %d not divisible by kv heads %d", who,
              a->num_q_heads, a->num_kv_heads);
  SVK_REQUIRE(a->score_mode == SVK_SCORE_NONE || a->score_mode == SVK_SCORE_HEADMAX || a->score_mode == SVK_SCORE_PERHEAD,
              SVK_ERR_VALUE, "%s: bad score_mode %d", who, a->score_mode);
  SVK_REQUIRE(a->slot_page_size >= 0 && (a->slot_page_size & (a->slot_page_size - 1)) == 0, SVK_ERR_VALUE,
              "%s: slot_page_size %d must be 0 or a power of two", who, a->slot_page_size);
  SVK_REQUIRE(a->score_mode == SVK_SCORE_NONE || a->attn_score != nullptr, SVK_ERR_VALUE, "%s: score_mode %d needs attn_score", who,
              a->score_mode);
  SVK_REQUIRE((a->kv_slot_stride % 8) == 0 && (a->kv_head_stride % 8) == 0 && (a->q_stride_h % 8) == 0 && (a->q_stride_b % 8) == 0,
              SVK_ERR_LAYOUT, "%s: q/k/v strides must keep 16-byte alignment", who);
  SVK_REQUIRE((a->mid_o_stride_h % 4) == 0 && (a->mid_o_stride_s % 4) == 0 && (a->mid_o_stride_b % 4) == 0, SVK_ERR_LAYOUT,
              "%s: mid_o strides must keep 16-byte alignment", who);
  if (a->new_k != nullptr || a->new_v != nullptr) {
    SVK_REQUIRE(a->new_k != nullptr && a->new_v != nullptr && a->slot_mapping != nullptr, SVK_ERR_VALUE,
                "%s: the fused store needs new_k, new_v and slot_mapping together", who);
    SVK_REQUIRE((a->new_stride_b % 8) == 0 && (a->new_stride_h % 8) == 0 && (reinterpret_cast<uintptr_t>(a->new_k) % 16) == 0 &&
                    (reinterpret_cast<uintptr_t>(a->new_v) % 16) == 0,
                SVK_ERR_LAYOUT, "%s: new_k/new_v rows must be 16-byte aligned", who);
  }
  if (a->new_cos_sin != nullptr) {
    SVK_REQUIRE(a->head_dim != 256, SVK_ERR_LAYOUT, "%s: the rotated store is head_dim 64 / 128 only, got %d", who, a->head_dim);
    SVK_REQUIRE(a->score_mode == SVK_SCORE_NONE && a->slot_page_size == 0, SVK_ERR_VALUE,
                "%s: the rotated store rides in unscored launches over token slots only", who);
    SVK_REQUIRE(a->new_k != nullptr && a->raw_k_cache != nullptr && a->raw_v_cache != nullptr && a->new_slot_to_pos != nullptr,
                SVK_ERR_VALUE, "%s: the rotated store needs new_k / new_v / slot_mapping, raw_k_cache, raw_v_cache and new_slot_to_pos", who);
    SVK_REQUIRE((a->raw_slot_stride % 8) == 0 && (a->raw_head_stride % 8) == 0 && a->raw_num_slots > 0, SVK_ERR_LAYOUT,
                "%s: raw cache rows must be 16-byte aligned", who);
    SVK_REQUIRE(a->new_cos_dtype == SVK_DTYPE_F32 || a->new_cos_dtype == SVK_DTYPE_BF16 || a->new_cos_dtype == SVK_DTYPE_F16,
                SVK_ERR_VALUE, "%s: new_cos_dtype %d", who, a->new_cos_dtype);
  }
  if (a->direct_o != nullptr) {
    SVK_REQUIRE(a->max_len_in_batch <= a->block_seq, SVK_ERR_VALUE,
                "%s: direct_o needs one block per sequence (max_len_in_batch %d > block_seq %d)", who, a->max_len_in_batch, a->block_seq);
    SVK_REQUIRE((a->direct_stride_b % 8) == 0 && (a->direct_stride_h % 8) == 0 && (reinterpret_cast<uintptr_t>(a->direct_o) % 16) == 0,
                SVK_ERR_LAYOUT, "%s: direct_o rows must be 16-byte aligned", who);
  }
  return SVK_OK;
}

extern "C" int svk_flash_decode_stage1(const SvkFlashDecodeStage1Args* a, svk_stream_t stream) {
  using namespace svk;
  const int rc = validate_stage1(a, "svk_flash_decode_stage1");
  if (rc != SVK_OK) return rc;
  if (a->batch <= 0 || a->max_len_in_batch <= 0) return SVK_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (a->head_dim == 256) return launch_flash_decode_stage1_d256(*a, s);
  return a->head_dim == 128 ? launch_stage1<128>(*a, s) : launch_stage1<64>(*a, s);
}

extern "C" int64_t svk_flash_decode_stage2_split_workspace_bytes(int32_t batch, int32_t num_q_heads, int32_t head_dim,
                                                                  int32_t max_partials) {
  using namespace svk;
  if (batch <= 0 || num_q_heads <= 0 || max_partials <= kSplitMin || max_partials > kSplitPPW * kSplitPPW) return 0;
  const int64_t n_bh = (int64_t)batch * num_q_heads, smax = split_groups(max_partials);
  return split_align(n_bh * smax * 4) + split_align(n_bh * smax * head_dim * 4);
}

extern "C" int svk_flash_decode_stage2(const SvkFlashDecodeStage2Args* a, svk_stream_t stream) {
  using namespace svk;
  SVK_REQUIRE(a != nullptr, SVK_ERR_VALUE, "svk_flash_decode_stage2: null args");
  SVK_REQUIRE(a->head_dim == 64 || a->head_dim == 128 || a->head_dim == 256, SVK_ERR_LAYOUT,
              "svk_flash_decode_stage2: head_dim %d unsupported (64, 128, 256)", a->head_dim);
  SVK_REQUIRE(a->block_seq > 0, SVK_ERR_VALUE, "svk_flash_decode_stage2: block_seq must be positive");
  SVK_REQUIRE(a->extra_partials >= 0 && a->extra_partials <= 8, SVK_ERR_VALUE, "svk_flash_decode_stage2: extra_partials %d out of range", a->extra_partials);
  SVK_REQUIRE((a->mid_o_stride_h % 4) == 0 && (a->mid_o_stride_s % 4) == 0 && (a->mid_o_stride_b % 4) == 0 &&
                  (a->o_stride_b % 4) == 0 && (a->o_stride_h % 4) == 0,
              SVK_ERR_LAYOUT, "svk_flash_decode_stage2: strides must be multiples of 4 elements (16-byte partial rows)");
  if (a->batch <= 0) return SVK_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  dim3 grid(a->batch, a->num_q_heads);
  // launches that may merge more than 128 partials per row get 1024 threads per (b, head) - 32 lane groups x 8
  // prefetched rows = 256 partials in ONE round trip, where 256 threads (8 groups) walk what lies beyond their first 64
  // in further trips (B=1 rows in 32-token blocks have 132 partials: 0.368 -> 0.355 ms per step; at 69 partials the
  // 1024-thread form is the slower one - its last lane group adds up 31 others).  The count is the LAUNCH's
  // (max_partials), not the workspace's capacity: the two forms add in different orders, so the output bits of a step
  // must not depend on what an earlier, longer launch grew the shared workspace to.
  SVK_REQUIRE(a->max_partials >= 0, SVK_ERR_VALUE, "svk_flash_decode_stage2: max_partials %d must be >= 0", a->max_partials);
  if (a->split_ws != nullptr && a->split_tickets != nullptr && a->max_partials > kSplitMin && a->max_partials <= kSplitPPW * kSplitPPW &&
      a->split_ws_bytes >= svk_flash_decode_stage2_split_workspace_bytes(a->batch, a->num_q_heads, a->head_dim, a->max_partials)) {
    SVK_REQUIRE((reinterpret_cast<uintptr_t>(a->split_ws) % 256) == 0, SVK_ERR_LAYOUT,
                "svk_flash_decode_stage2: split_ws must be 256-byte aligned");
    dim3 grid3(a->batch, a->num_q_heads, split_groups(a->max_partials));
    if (a->head_dim == 256) hipLaunchKernelGGL((decode_stage2_split_kernel<256>), grid3, dim3(256), 0, s, *a);
    else if (a->head_dim == 128) hipLaunchKernelGGL((decode_stage2_split_kernel<128>), grid3, dim3(256), 0, s, *a);
    else hipLaunchKernelGGL((decode_stage2_split_kernel<64>), grid3, dim3(256), 0, s, *a);
    return check_launch("svk_flash_decode_stage2");
  }
  const bool wide = (a->max_partials > 0 ? (int64_t)a->max_partials : a->mid_lse_stride_h) > 128;
  if (a->head_dim == 256) {
    // 64 lanes per partial row: 4 lane groups at 256 threads (8 prefetched rows each), 16 at 1024 (two-level LDS sum)
    if (wide) hipLaunchKernelGGL((decode_stage2_kernel<256, 1024>), grid, dim3(1024), 0, s, *a);
    else hipLaunchKernelGGL((decode_stage2_kernel<256, 256>), grid, dim3(256), 0, s, *a);
  } else if (a->head_dim == 128) {
    if (wide) hipLaunchKernelGGL((decode_stage2_kernel<128, 1024>), grid, dim3(1024), 0, s, *a);
    else hipLaunchKernelGGL((decode_stage2_kernel<128, 256>), grid, dim3(256), 0, s, *a);
  } else {
    if (wide) hipLaunchKernelGGL((decode_stage2_kernel<64, 1024>), grid, dim3(1024), 0, s, *a);
    else hipLaunchKernelGGL((decode_stage2_kernel<64, 256>), grid, dim3(256), 0, s, *a);
  }
  return check_launch("svk_flash_decode_stage2");
}
