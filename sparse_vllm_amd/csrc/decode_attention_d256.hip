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
//   * P.V: v3's mapping on the wave's 128 V dims (acc[8]: 8 dims x 4 heads per lane).
//   * scores: wave 0 of each pair stores (PERHEAD) or writes its tile maxima into the LDS score chunk (HEADMAX), one
//     owner thread per token column combines across KV heads: store or max-combine, no float atomics.
//   * epilogue: each wave writes its 128 dims of mid_o / direct_o, wave 0 of the pair writes mid_lse.
//   * KV heads 1..4: __launch_bounds__(512); 5..8 (up to 16 waves): a second instantiation with __launch_bounds__(1024).
//
// Shared with v3 (decode_stage1_tile.hpp, one copy): empty-block fill, plain fused store and its fence pair, K / V
// addressing, slot fetch, prologue, K and V tile loads, Q.K^T, score emission, online softmax, P write and rescale, P.V,
// the HEADMAX chunk combine, the epilogue (statement macros SVK_S1_*) and the host-side dispatch.  This kernel's own: the LDS layout, the partial-S
// exchange, the LDS-only barrier around the combine and the LEAN schedule with its three placements of the V loads.
//
// Not carried over: the rotated form of the fused store (deltakv_view.hip is head_dim 128 only; refused by the caller).

#include "decode_stage1_tile.hpp"

namespace svk {
namespace {

constexpr int kHalf = 128;         // head dims per wave
constexpr int kNC = kHalf / 32;    // MFMA k-chunks per half row
constexpr int kMaxLds = 160 * 1024;

template <int G>
struct D256Lds {
  static constexpr int JQ = stage1_jq(G);
  static constexpr int XCH = JQ * 16 * 2 * 4;      // one exchange buffer: JQ*16 lanes x 2 column groups x 4 rows
  // P tile (bf16) | 2 x 32 slot ids | Q half-fragments (kNC x 64 lanes x 16 B) | 2 exchange buffers
  static constexpr int WAVE_FLOATS = kPFloats + 64 + kNC * 64 * 4 + 2 * XCH;
};

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

  SVK_S1_OUT_PTRS(+ hx * kHalf)

  // (b, blk) are the workgroup's: every wave takes this return or none does, and no barrier has been passed yet
  if (end <= start) {
    SVK_S1_FILL_EMPTY(kvh, kHalf, hx == 0 &&)
    return;
  }

  if (a.new_k != nullptr && end == len) {
    // fused store_kvcache: wave (kvh, hx) writes ITS half of the head's K and V rows; only this wave reads those
    // bytes in this launch, so the workgroup-scope fence pair is enough here as well
    SVK_S1_STORE_NEW_KV(kvh, const int64_t col = hx * kHalf + seg * 8;, col)
    SVK_S1_STORE_FENCE()
  }
  SVK_S1_ADDRESSING(kvh, hx * kHalf +, n)         // 16 V segments per half row = the 16 MFMA columns
  SVK_S1_PROLOGUE(kvh, hx * kHalf +)               // acc[i][r]: head jq*4+r, head dim hx*128 + n*8 + i

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
      SVK_S1_LOAD_V(true)
    }

    SVK_S1_ADVANCE_SLOTS()

    // ---- partial S = Q[:, half] K[:, half]^T on K(i)
    SVK_S1_QK()
    // ---- hand the partial tile to the partner wave (row groups holding real heads only)
    if (jq < JQ) {
#pragma unroll
      for (int g = 0; g < 2; ++g) xch_mine[buf * (XCH / 4) + g * (JQ * 16) + lane] = s[g];
    }
    lds_barrier();      // the pair's partials and this wave's nxt_slots are visible
    // ---- K registers are dead: re-arm them with K(i+1)
    if constexpr (has_next && !LEAN) {
      SVK_S1_LOAD_K(nxt_slots)
    }
    // (per-head scores: their 64-bit store addresses and 32 V registers do not fit together - V(i) follows the stores)
    if constexpr (LEAN && MODE != SVK_SCORE_PERHEAD) {
      SVK_S1_LOAD_V(true)
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

    SVK_S1_TOKEN_VALID()

    SVK_S1_EMIT_SCORES(kvh, hx == 0 &&)
    if constexpr (LEAN && MODE == SVK_SCORE_PERHEAD) {
      SVK_S1_LOAD_V(true)
    }

    SVK_S1_SOFTMAX_STEP()
    SVK_S1_WRITE_P_RESCALE()
    wave_sync();
    SVK_S1_PV()                                    // B column n of MFMA i = head dim hx*128 + n*8 + i
    wave_sync();
    if constexpr (has_next && LEAN) {
      SVK_S1_LOAD_K(nxt_slots)
    }

    // every wave of the workgroup reaches the combine's barriers or none does: LDS-only, the loads stay in flight
    SVK_S1_SCORE_CHUNK_END(lds_barrier)
    t0 += kTileTokens;
    buf ^= 1;
  };
  while (t0 + kTileTokens < end) tile(std::true_type{});
  tile(std::false_type{});

  SVK_S1_EPILOGUE(kvh, hx == 0 &&, , n_e)
}

// 1..4 KV heads: MAXT = 512; 5..8: 1024
template <int MAXT>
int launch_d256(const SvkFlashDecodeStage1Args& a, hipStream_t stream) {
  const int nblk = (a.max_len_in_batch + a.block_seq - 1) / a.block_seq;
  dim3 grid(nblk, a.batch);
  dim3 block(128 * a.num_kv_heads);                  // two waves per KV head
  return stage1_dispatch(a, [&](auto g, auto mode, auto off32) {
    constexpr int G = decltype(g)::value;
    const size_t shm = sizeof(float) * ((size_t)2 * a.num_kv_heads * D256Lds<G>::WAVE_FLOATS + stage1_score_floats<G>(a));
    auto kern = decode_stage1_d256_kernel<G, decltype(mode)::value, decltype(off32)::value, MAXT>;
    // 5..8 KV heads (and 4 with head-max scores) need more than the 64 KiB of dynamic LDS a kernel may use by default
    static bool wide_lds = false;                    // one per instantiation
    if (shm > 64 * 1024 && !wide_lds) {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds);
      wide_lds = true;
    }
    hipLaunchKernelGGL(kern, grid, block, shm, stream, a);
  });
}

}  // namespace

// validated by svk_flash_decode_stage1 (decode_attention.hip): head_dim 256, 1..8 KV heads, no rotated store
int launch_flash_decode_stage1_d256(const SvkFlashDecodeStage1Args& a, hipStream_t stream) {
  return a.num_kv_heads <= 4 ? launch_d256<512>(a, stream) : launch_d256<1024>(a, stream);
}

}  // namespace svk
