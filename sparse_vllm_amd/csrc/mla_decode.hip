// Multi-head latent attention (MLA) split-KV decode over the latent cache (gfx950).  Replaces the reference's
// kernels/triton/mla/decode_stage1.py:141-255, decode_stage2.py:19-85 and copy_latent.py:17-85.
//
// A token is ONE 512-wide latent row + ONE 64-wide RoPE row shared by all query heads; the key is the 576 values, the
// value the first 512 of them.  Stage 1, per (batch lane, block of block_seq positions, head tile of 32 heads):
//   * workgroup = 4 waves.  The query heads are the MFMA N dimension of S^T = X Q^T (v_mfma_f32_32x32x16_bf16, A = 32
//     tokens x 16 columns out of LDS, B = Q^T held in registers for the whole block), so a lane's 16 accumulator
//     registers are 16 tokens of ONE head: the softmax statistics are in-lane reductions plus one exchange with
//     lane ^ 32, and the packed P registers ARE the A operand of P.V.
//   * a tile of 32 tokens (32 x 1152 B = 36 KiB) is gathered ONCE per workgroup through the slot ids by LDS-DMA
//     (9 groups of four global_load_lds_dwordx4, dealt to the waves) into a double-buffered LDS tile; masked and
//     padding rows are fetched from a zero row, never from the pool.  The 16-byte chunks are swizzled on the DMA source
//     address (mla_pos) so that both the row reads of S^T and the transposed reads of P.V are conflict-free.
//   * the 576-wide contraction is split over the waves (9 k-steps each); the four partial S^T tiles cross a 16 KiB
//     exchange area and EVERY wave adds them in the order 0,1,2,3: all waves hold bit-identical S, P and statistics.
//   * the 512 output columns are split over the waves (128 each = 4 accumulators of 16 registers); V comes token-major
//     out of the same tile by ds_read_b64_tr_b16.
//   * raw S (before softmax_scale) goes to the score buffer by plain stores; the head maximum of the HEADMAX mode is a
//     lane reduction, and with several head tiles the workgroup walks them one after the other and folds the maximum
//     into what IT wrote before - no atomics.  Without HEADMAX the head tiles are a grid dimension.
// No float atomics; every sum has one order that depends on positions only, never on slot addresses.

#include "svk_common.hpp"
#include "lds_dma.hpp"

namespace svk {
namespace {

constexpr int kMlaL = 512;                            // latent width (= value width)
constexpr int kMlaR = 64;                             // RoPE width
constexpr int kMlaTT = 32;                            // tokens per LDS tile
constexpr int kMlaChunks = (kMlaL + kMlaR) / 8;       // 16-byte chunks of a token row (72)
constexpr int kMlaRowB = kMlaChunks * 16;             // 1152
constexpr int kMlaTile = kMlaTT * kMlaRowB;           // 36864
constexpr int kMlaGroups = kMlaTile / 4096;           // DMA groups of four instructions per tile (9)
constexpr int kMlaKS = (kMlaL + kMlaR) / 16 / 4;      // k-steps of S per wave (9)
constexpr int kMlaXchg = 4 * 16 * 64 * 4;             // four partial S^T tiles
constexpr int kMlaShm = 2 * kMlaTile + kMlaXchg + 4 * 32 * 4;

typedef __attribute__((ext_vector_type(4))) short mla_s16x4_t;
typedef __attribute__((ext_vector_type(8))) short mla_s16x8_t;

__device__ uint4 mla_zero_row[kMlaChunks];            // source of masked / padding rows (zero-initialised)

// LDS position (16-byte units inside the row) of chunk c of tile row r; an involution in c, so it also maps a position
// back to the chunk stored there.  Row r starts at bank-chunk 8 (r & 1) (1152 B = 4.5 x 256 B).  Latent chunks: the low
// four bits are XORed with f(r) = swap of the two 2-bit fields of r, ^ 8 (r & 1): 16 consecutive rows reading one chunk
// (S^T) cover the 16 bank-chunks, and 4 consecutive rows reading 4 neighbouring chunks (transposed V reads) land in
// four different 64-byte bank groups.  RoPE chunks (8 per row) are rotated inside their own half of the banks.
__device__ __forceinline__ int mla_pos(int r, int c) {
  const int f = (((r & 3) << 2) | ((r >> 2) & 3)) ^ ((r & 1) << 3);
  return c < 64 ? ((c & ~15) | ((c ^ f) & 15)) : (64 | ((c ^ (r >> 1)) & 7));
}

template <int MODE>
__global__ void __launch_bounds__(256) mla_stage1_kernel(const SvkMlaDecodeStage1Args a, int tiles_per_wg) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  float* xch = reinterpret_cast<float*>(lds_raw + 2 * kMlaTile);
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lq = lane & 31, half = lane >> 5;
  float* fac = xch + kMlaXchg / 4 + w * 32;
  const int blk = blockIdx.x, b = blockIdx.z, H = a.num_heads;
  const int nht = (H + 31) >> 5;
  const int ht0 = blockIdx.y * tiles_per_wg, ht1 = min(nht, ht0 + tiles_per_wg);
  const int req = a.request_indices[b];
  const int len = (req < 0 || req >= a.slot_rows) ? 0 : max(0, min(a.context_lens[b], a.max_context_len));
  const int t_begin = blk * a.block_seq, t_end = min(len, t_begin + a.block_seq);
  float* mo = a.mid_o + (int64_t)b * a.mid_o_stride_b + (int64_t)blk * a.mid_o_stride_s;
  float* ml = a.mid_lse + (int64_t)b * a.mid_lse_stride_b + blk;
  if (t_begin >= len) {                                           // a block without tokens: (0, -inf)
    const int h_lo = ht0 * 32, h_hi = min(H, ht1 * 32);
    for (int e = tid; e < (h_hi - h_lo) * (kMlaL / 4); e += 256) {
      const int h = h_lo + e / (kMlaL / 4), c = (e % (kMlaL / 4)) * 4;
      *reinterpret_cast<float4*>(mo + (int64_t)h * a.mid_o_stride_h + c) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int h = h_lo + tid; h < h_hi; h += 256) ml[(int64_t)h * a.mid_lse_stride_h] = -INFINITY;
    return;
  }
  const int32_t* srow = a.active_slots + (int64_t)req * a.slots_stride;
  const int64_t num_slots = a.num_slots;
  const uint32_t lds0 = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)lds_raw);
  const char* lat = reinterpret_cast<const char*>(a.latent_cache);
  const char* rop = reinterpret_cast<const char*>(a.rope_cache);
  const char* zero = reinterpret_cast<const char*>(mla_zero_row);
  const int64_t lat_bytes = a.latent_slot_stride * 2, rop_bytes = a.rope_slot_stride * 2;
  const float sc = a.softmax_scale * 1.4426950408889634f;

  // ---- token tile -> LDS.  DMA instruction q of a tile fills the LDS bytes [1024 q, 1024 q + 1024): lane -> tile row
  // r = byte / 1152 and position p inside it, which holds chunk mla_pos(r, p).  Group g of four belongs to wave g & 3.
  // The slot ids travel as RAW loaded values (sl: per DMA instruction of the next tile to issue, mraw: of position lq of
  // the next tile to compute) and are only looked at one iteration later, in front of the DMA issue.  vmcnt retires in
  // order and the compiler cannot count the DMA hidden in the asm statement: any use of a freshly loaded id between the
  // DMA issue and the end of the tile would put the compiler's own s_waitcnt vmcnt(0) there and drain the prefetch.
  int sl[12];
  auto load_slots = [&](int t0) __attribute__((always_inline)) {
#pragma unroll
    for (int gi = 0; gi < 3; ++gi) {
      const int g = w + 4 * gi;
      if (g < kMlaGroups) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          int tok = min(t0 + ((g * 4 + j) * 1024 + lane * 16) / kMlaRowB, t_end - 1);
          // (opaque index: an instruction whose 64 lanes share one row would otherwise become a scalarised load whose
          // v_readfirstlane is exactly such an early use)
          asm volatile("" : "+v"(tok));
          sl[gi * 4 + j] = srow[tok];
        }
      }
    }
  };
  auto issue = [&](int buf, int t0) __attribute__((always_inline)) {
#pragma unroll
    for (int gi = 0; gi < 3; ++gi) {
      const int g = w + 4 * gi;
      if (g < kMlaGroups) {
        const char* src[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int L = (g * 4 + j) * 1024 + lane * 16;
          const int r = L / kMlaRowB, c = mla_pos(r, (L % kMlaRowB) >> 4);
          const int64_t s = sl[gi * 4 + j];
          const bool live = t0 + r < t_end && s >= 0 && s < num_slots;      // else: the zero row
          const char* p = !live ? zero + c * 16 : (c < 64 ? lat + (s * lat_bytes + c * 16) : rop + (s * rop_bytes + (c - 64) * 16));
          src[j] = p - 1024 * j;
        }
        pa_dma4x16(src, lds0 + buf * kMlaTile + g * 4096);
      }
    }
  };
  // bit t of the mask: position t0 + t is below the length and its slot lies inside the pool
  auto load_mask_slot = [&](int t0) __attribute__((always_inline)) -> int { return srow[min(t0 + lq, t_end - 1)]; };
  auto tile_mask = [&](int raw, int t0) __attribute__((always_inline)) -> uint32_t {
    return (uint32_t)__ballot(t0 + lq < t_end && raw >= 0 && (int64_t)raw < num_slots);
  };

  // LDS addresses: A fragments of S^T (lane = token row lq, chunk 2 ks + half of this wave's k-steps) and the transposed
  // V reads (lane q of a 16-lane group points at token (q >> 2) + 4 half + 8 eh of a block of 16, columns
  // 128 w + 32 i + 16 (lq >> 4) + 4 (q & 3) .. + 3; it receives column 128 w + 32 i + lq of four tokens)
  uint32_t kaddr[kMlaKS], vaddr[4][2];
#pragma unroll
  for (int u = 0; u < kMlaKS; ++u) kaddr[u] = lds0 + lq * kMlaRowB + mla_pos(lq, 2 * (kMlaKS * w + u) + half) * 16;
  {
    const int q16 = lane & 15;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int eh = 0; eh < 2; ++eh) {
        const int r = (q16 >> 2) + 4 * half + 8 * eh;
        const int c = 16 * w + 4 * i + 2 * (lq >> 4) + ((q16 & 3) >> 1);
        vaddr[i][eh] = lds0 + r * kMlaRowB + mla_pos(r, c) * 16 + 8 * (q16 & 1);
      }
  }
  const int T = (t_end - t_begin + kMlaTT - 1) / kMlaTT;

  for (int ht = ht0; ht < ht1; ++ht) {
    const int h = ht * 32 + lq;
    const bool hok = h < H;
    // Q^T fragments (B operand): lane (head lq, half) holds Q[h][16 ks + 8 half .. + 8]; columns >= 512 are q_rope
    bf16x8_t qb[kMlaKS];
    {
      const uint16_t* ql = a.q_latent + (int64_t)b * a.q_latent_stride_b + (int64_t)(hok ? h : 0) * a.q_latent_stride_h;
      const uint16_t* qr = a.q_rope + (int64_t)b * a.q_rope_stride_b + (int64_t)(hok ? h : 0) * a.q_rope_stride_h;
#pragma unroll
      for (int u = 0; u < kMlaKS; ++u) {
        const int col = (kMlaKS * w + u) * 16 + half * 8;
        uint4 t = make_uint4(0, 0, 0, 0);
        if (hok) t = *reinterpret_cast<const uint4*>(col < kMlaL ? ql + col : qr + (col - kMlaL));
        qb[u] = __builtin_bit_cast(bf16x8_t, t);
      }
    }
    float m_run = -INFINITY, l_part = 0.f;                        // of head lq (both halves keep the same maximum)
    f32x16_t o[4];                                                // o[i][r]: head (r&3) + 8 (r>>2) + 4 half, column 128 w + 32 i + lq
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[i][r] = 0.f;

    load_slots(t_begin);
    issue(0, t_begin);
    int mraw = load_mask_slot(t_begin);
    if (T > 1) load_slots(t_begin + kMlaTT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    for (int k = 0; k < T; ++k) {
      const int buf = k & 1, t0 = t_begin + k * kMlaTT;
      // everything loaded during the previous tile is consumed HERE, then the DMA of tile k + 1 goes out and the raw ids
      // of the tiles behind it follow; nothing below looks at them before the end-of-tile wait
      const uint32_t vm = tile_mask(mraw, t0);
      if (k + 1 < T) {
        issue(buf ^ 1, t0 + kMlaTT);
        mraw = load_mask_slot(t0 + kMlaTT);
      }
      if (k + 2 < T) load_slots(t0 + 2 * kMlaTT);

      // ---- partial S^T over this wave's 144 columns; register r of lane (lq, half) = token (r&3) + 8 (r>>2) + 4 half
      f32x16_t s = {};
      {
        pa_u32x4_t kf[kMlaKS];
#pragma unroll
        for (int u = 0; u < kMlaKS; ++u)
          kf[u] = *reinterpret_cast<const __attribute__((address_space(3))) pa_u32x4_t*>(kaddr[u] + buf * kMlaTile);
#pragma unroll
        for (int u = 0; u < kMlaKS; ++u)
          s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, kf[u]), qb[u], s, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) xch[(w * 16 + r) * 64 + lane] = s[r];
      lds_barrier();
#pragma unroll
      for (int r = 0; r < 16; ++r)
        s[r] = add_rn(add_rn(add_rn(xch[r * 64 + lane], xch[(16 + r) * 64 + lane]), xch[(32 + r) * 64 + lane]),
                      xch[(48 + r) * 64 + lane]);

      // ---- raw scores: wave q publishes the registers [4 q, 4 q + 4) = tokens 8 q + 4 half .. + 3
      if constexpr (MODE != SVK_SCORE_NONE) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if (q == w) {
            const int jr = 8 * q + 4 * half;
            if constexpr (MODE == SVK_SCORE_PERHEAD) {
              float* dst = a.attn_score + (int64_t)b * a.score_stride_b + (int64_t)h * a.score_stride_h + t0 + jr;
#pragma unroll
              for (int e = 0; e < 4; ++e)
                if (hok && ((vm >> (jr + e)) & 1u)) dst[e] = s[4 * q + e];
            } else {
              float* dst = a.attn_score + (int64_t)b * a.score_stride_b + t0 + jr;
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                float v = hok ? s[4 * q + e] : -INFINITY;
#pragma unroll
                for (int x = 1; x < 32; x <<= 1) v = fmaxf(v, __shfl_xor(v, x, 64));
                // (tiles after the first read back what this thread stored: that load is used at once, so its wait
                // also drains the DMA of the next tile - the price of folding the maximum without atomics)
                if (ht > ht0) {
                  if (lq == 0 && ((vm >> (jr + e)) & 1u)) dst[e] = fmaxf(v, dst[e]);
                } else {
                  if (lq == 0 && ((vm >> (jr + e)) & 1u)) dst[e] = v;
                }
              }
            }
          }
        }
      }

      // ---- online softmax of S * softmax_scale (base-2 exponents), identical in the four waves
      float mx = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int jr = (r & 3) + 8 * (r >> 2) + 4 * half;
        s[r] = ((vm >> jr) & 1u) ? s[r] : -INFINITY;
        mx = fmaxf(mx, s[r]);
      }
      mx = fmaxf(mx, lane_xor32(mx));
      const float m_new = fmaxf(m_run, mx);
      const float nms = (m_new == -INFINITY ? 0.f : m_new) * sc;
      const float al = __builtin_amdgcn_exp2f(m_run * sc - nms);  // first tokens of the head: exp2(-inf) = 0
      m_run = m_new;
      float psum = 0.f;
      uint32_t pp[8];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        s[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[r], sc, -nms));
        psum += s[r];
        if (r & 1) pp[r >> 1] = pack_bf16(s[r - 1], s[r]);
      }
      l_part = l_part * al + psum;
      if (k > 0 && __any(al != 1.0f)) {
        // rescale factors: "lane = head" -> "register = head" through the wave's LDS row
        if (half == 0) fac[lq] = al;
        wave_sync();
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          const float4 f4 = *reinterpret_cast<const float4*>(fac + 8 * jj + 4 * half);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            o[i][4 * jj + 0] *= f4.x; o[i][4 * jj + 1] *= f4.y; o[i][4 * jj + 2] *= f4.z; o[i][4 * jj + 3] *= f4.w;
          }
        }
        wave_sync();
      }

      // ---- O += P V: A = P (k index e of half <-> token 16 sp + 8 (e>>2) + 4 half + (e&3)), B = V by transposed reads
#pragma unroll
      for (int sp = 0; sp < 2; ++sp) {
        const bf16x8_t pa = __builtin_bit_cast(bf16x8_t, make_uint4(pp[4 * sp], pp[4 * sp + 1], pp[4 * sp + 2], pp[4 * sp + 3]));
        mla_s16x4_t vr[4][2];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int eh = 0; eh < 2; ++eh)
            vr[i][eh] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(reinterpret_cast<__attribute__((address_space(3))) mla_s16x4_t*>(
                vaddr[i][eh] + (uint32_t)(buf * kMlaTile + sp * 16 * kMlaRowB)));
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const mla_s16x8_t vb = __builtin_shufflevector(vr[i][0], vr[i][1], 0, 1, 2, 3, 4, 5, 6, 7);
          o[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa, __builtin_bit_cast(bf16x8_t, vb), o[i], 0, 0, 0);
        }
      }
      // the next tile has landed for every wave behind this barrier, and nobody reads this tile or the exchange area
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }

    // ---- epilogue: mid_o = acc / sum_exp, mid_lse = max * scale + log(sum_exp); a block of masked slots only: (0, -inf)
    const float l = l_part + lane_xor32(l_part);
    if (half == 0) fac[lq] = l;
    if (half == 0 && hok)
      ml[(int64_t)h * a.mid_lse_stride_h] = l > 0.f ? m_run * a.softmax_scale + logf(l) : -INFINITY;
    wave_sync();
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const float4 f4 = *reinterpret_cast<const float4*>(fac + 8 * jj + 4 * half);
      const float lr[4] = {f4.x, f4.y, f4.z, f4.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int hr = ht * 32 + 8 * jj + 4 * half + e;
        if (hr < H) {
          float* dst = mo + (int64_t)hr * a.mid_o_stride_h + 128 * w + lq;
#pragma unroll
          for (int i = 0; i < 4; ++i) dst[32 * i] = lr[e] > 0.f ? o[i][4 * jj + e] / lr[e] : 0.f;
        }
      }
    }
    wave_sync();
  }
}

// LSE-weighted merge of the block partials.  128 lanes x 16-byte loads cover a 512-float row; the two lane groups walk
// the partials interleaved (even / odd) and are folded in a fixed order.
__global__ void __launch_bounds__(256) mla_stage2_kernel(const SvkMlaDecodeStage2Args a) {
  __shared__ float4 sacc[128];
  __shared__ float sm[128], sl[128];
  const int h = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, g = tid >> 7, t = tid & 127;
  const int len = max(0, min(a.context_lens[b], a.max_context_len));
  const int nb = (len + a.block_seq - 1) / a.block_seq;
  const float* mo = a.mid_o + (int64_t)b * a.mid_o_stride_b + (int64_t)h * a.mid_o_stride_h + t * 4;
  const float* ml = a.mid_lse + (int64_t)b * a.mid_lse_stride_b + (int64_t)h * a.mid_lse_stride_h;
  float m = -INFINITY, l = 0.f;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  auto fold = [&](float lse, const float4& v, float wl) __attribute__((always_inline)) {
    if (lse == -INFINITY) return;
    const float mn = fmaxf(m, lse);
    const float al = expf(m - mn), wg = expf(lse - mn);
    acc.x = acc.x * al + v.x * wg; acc.y = acc.y * al + v.y * wg;
    acc.z = acc.z * al + v.z * wg; acc.w = acc.w * al + v.w * wg;
    l = l * al + wl * wg;
    m = mn;
  };
  for (int j = g; j < nb; j += 2) fold(ml[j], *reinterpret_cast<const float4*>(mo + (int64_t)j * a.mid_o_stride_s), 1.f);
  if (g == 1) { sacc[t] = acc; sm[t] = m; sl[t] = l; }
  __syncthreads();
  if (g == 0) {
    fold(sm[t], sacc[t], sl[t]);
    const float inv = l > 0.f ? 1.f / l : 0.f;                     // a lane of length 0: zeros
    uint2 r;
    r.x = f32_to_bf16_bits(acc.x * inv) | (f32_to_bf16_bits(acc.y * inv) << 16);
    r.y = f32_to_bf16_bits(acc.z * inv) | (f32_to_bf16_bits(acc.w * inv) << 16);
    *reinterpret_cast<uint2*>(a.output + (int64_t)b * a.o_stride_b + (int64_t)h * a.o_stride_h + t * 4) = r;
  }
}

// one 16-byte chunk per thread: 64 latent + 8 RoPE chunks per token
__global__ void __launch_bounds__(256) mla_store_latent_kernel(const SvkMlaStoreLatentArgs a) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t n = idx / kMlaChunks;
  const int c = (int)(idx % kMlaChunks);
  if (n >= a.n_tokens) return;
  const int64_t slot = a.slot_mapping[n];
  if (slot < 0 || slot >= a.num_slots) return;
  if (c < 64)
    *reinterpret_cast<uint4*>(a.latent_cache + slot * a.latent_slot_stride + c * 8) =
        *reinterpret_cast<const uint4*>(a.latent + n * a.latent_stride + c * 8);
  else
    *reinterpret_cast<uint4*>(a.rope_cache + slot * a.rope_slot_stride + (c - 64) * 8) =
        *reinterpret_cast<const uint4*>(a.rope + n * a.rope_stride + (c - 64) * 8);
}

// Prefill gather, one 16-byte chunk per thread as above: packed row packed_start_locs[b] + j <- the cache rows of slot
// active_slots[request_indices[b], j]; a slot outside the pool gives a zero row and is never dereferenced.
__global__ void __launch_bounds__(256) mla_gather_latent_kernel(const SvkMlaGatherLatentArgs a) {
  const int b = blockIdx.y;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t j = idx / kMlaChunks;
  const int c = (int)(idx % kMlaChunks);
  const int64_t r = a.request_indices[b];
  if (r < 0 || r >= a.slot_rows || j >= min(a.context_lens[b], a.max_context_len)) return;
  const int64_t dst = (int64_t)a.packed_start_locs[b] + j;
  if (dst < 0 || dst >= a.out_capacity) return;
  const int64_t slot = a.active_slots[r * a.slots_stride + j];
  const bool live = slot >= 0 && slot < a.num_slots;
  uint4 v = make_uint4(0u, 0u, 0u, 0u);
  if (c < 64) {
    if (live) v = *reinterpret_cast<const uint4*>(a.latent_cache + slot * a.latent_slot_stride + c * 8);
    *reinterpret_cast<uint4*>(a.gathered_latent + dst * a.out_latent_stride + c * 8) = v;
  } else {
    if (live) v = *reinterpret_cast<const uint4*>(a.rope_cache + slot * a.rope_slot_stride + (c - 64) * 8);
    *reinterpret_cast<uint4*>(a.gathered_rope + dst * a.out_rope_stride + (c - 64) * 8) = v;
  }
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <int MODE>
int mla_stage1_launch(const SvkMlaDecodeStage1Args& a, hipStream_t s) {
  static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&mla_stage1_kernel<MODE>),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, kMlaShm);
  if (attr != hipSuccess) {
    set_error("svk_mla_decode_stage1: cannot reserve %d bytes of LDS per workgroup: %s", kMlaShm, hipGetErrorString(attr));
    return SVK_ERR_LAUNCH;
  }
  const int nht = (a.num_heads + 31) / 32;
  const int per_wg = MODE == SVK_SCORE_HEADMAX ? nht : 1;         // HEADMAX: one workgroup folds the tiles' maxima
  const int nblk = (a.max_context_len + a.block_seq - 1) / a.block_seq;
  hipLaunchKernelGGL((mla_stage1_kernel<MODE>), dim3(nblk, nht / per_wg, a.batch), dim3(256), (size_t)kMlaShm, s, a, per_wg);
  return check_launch("svk_mla_decode_stage1");
}

}  // namespace
}  // namespace svk

extern "C" int svk_mla_decode_stage1(const SvkMlaDecodeStage1Args* a, svk_stream_t stream) {
  using namespace svk;
  SVK_REQUIRE(a != nullptr, SVK_ERR_VALUE, "svk_mla_decode_stage1: null args");
  SVK_REQUIRE(a->latent_dim == kMlaL && a->rope_dim == kMlaR, SVK_ERR_LAYOUT,
              "svk_mla_decode_stage1: latent_dim %d / rope_dim %d unsupported (512 / 64)", a->latent_dim, a->rope_dim);
  SVK_REQUIRE(a->num_heads >= 1 && a->num_heads <= 128, SVK_ERR_LAYOUT,
              "svk_mla_decode_stage1: num_heads %d unsupported (1..128)", a->num_heads);
  SVK_REQUIRE(a->block_seq > 0 && a->block_seq % kMlaTT == 0, SVK_ERR_LAYOUT,
              "svk_mla_decode_stage1: block_seq %d must be a positive multiple of %d", a->block_seq, kMlaTT);
  SVK_REQUIRE(a->score_mode == SVK_SCORE_NONE || a->score_mode == SVK_SCORE_HEADMAX || a->score_mode == SVK_SCORE_PERHEAD,
              SVK_ERR_VALUE, "svk_mla_decode_stage1: score_mode %d unknown", a->score_mode);
  SVK_REQUIRE(a->score_mode == SVK_SCORE_NONE || a->attn_score != nullptr, SVK_ERR_VALUE,
              "svk_mla_decode_stage1: score_mode %d needs attn_score", a->score_mode);
  SVK_REQUIRE(__builtin_isfinite(a->softmax_scale) && a->softmax_scale > 0.f, SVK_ERR_VALUE,
              "svk_mla_decode_stage1: softmax_scale must be finite and positive, got %g.", (double)a->softmax_scale);
  SVK_REQUIRE(a->q_latent && a->q_rope && a->latent_cache && a->rope_cache && a->active_slots && a->request_indices &&
                  a->context_lens && a->mid_o && a->mid_lse,
              SVK_ERR_VALUE, "svk_mla_decode_stage1: null tensor pointer");
  SVK_REQUIRE(a->latent_slot_stride >= kMlaL && a->latent_slot_stride % 8 == 0 && a->rope_slot_stride >= kMlaR &&
                  a->rope_slot_stride % 8 == 0 && al16(a->latent_cache) && al16(a->rope_cache),
              SVK_ERR_LAYOUT, "svk_mla_decode_stage1: cache pointers and slot strides (latent %lld, rope %lld elements) must keep 16-byte alignment",
              (long long)a->latent_slot_stride, (long long)a->rope_slot_stride);
  SVK_REQUIRE(a->q_latent_stride_b % 8 == 0 && a->q_latent_stride_h % 8 == 0 && a->q_rope_stride_b % 8 == 0 &&
                  a->q_rope_stride_h % 8 == 0 && al16(a->q_latent) && al16(a->q_rope),
              SVK_ERR_LAYOUT, "svk_mla_decode_stage1: q_latent / q_rope pointers and strides must keep 16-byte alignment");
  SVK_REQUIRE(a->mid_o_stride_b % 4 == 0 && a->mid_o_stride_h % 4 == 0 && a->mid_o_stride_s % 4 == 0 && al16(a->mid_o),
              SVK_ERR_LAYOUT, "svk_mla_decode_stage1: mid_o pointer and strides must keep 16-byte alignment");
  SVK_REQUIRE(a->num_slots > 0 && a->slot_rows > 0 && a->slots_stride >= a->max_context_len, SVK_ERR_VALUE,
              "svk_mla_decode_stage1: empty pool / slot table, or slots_stride %lld below max_context_len %d",
              (long long)a->slots_stride, a->max_context_len);
  SVK_REQUIRE(a->mid_lse_stride_b > 0 && a->mid_lse_stride_h > 0 && a->mid_o_stride_b > 0 && a->mid_o_stride_h > 0 &&
                  a->mid_o_stride_s >= kMlaL,
              SVK_ERR_VALUE, "svk_mla_decode_stage1: mid_o / mid_lse strides must be positive (mid_o block stride >= 512)");
  SVK_REQUIRE(a->score_mode == SVK_SCORE_NONE ||
                  (a->score_stride_b >= a->max_context_len &&
                   (a->score_mode != SVK_SCORE_PERHEAD || a->score_stride_h >= a->max_context_len)),
              SVK_ERR_VALUE, "svk_mla_decode_stage1: score strides (b %lld, h %lld) shorter than max_context_len %d",
              (long long)a->score_stride_b, (long long)a->score_stride_h, a->max_context_len);
  SVK_REQUIRE(a->batch >= 0 && a->batch <= 65535 && a->max_context_len > 0, SVK_ERR_VALUE,
              "svk_mla_decode_stage1: batch %d must lie in 0..65535 and max_context_len %d must be positive", a->batch,
              a->max_context_len);
  if (a->batch == 0) return SVK_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (a->score_mode) {
    case SVK_SCORE_NONE: return mla_stage1_launch<SVK_SCORE_NONE>(*a, s);
    case SVK_SCORE_HEADMAX: return mla_stage1_launch<SVK_SCORE_HEADMAX>(*a, s);
    default: return mla_stage1_launch<SVK_SCORE_PERHEAD>(*a, s);
  }
}

extern "C" int svk_mla_decode_stage2(const SvkMlaDecodeStage2Args* a, svk_stream_t stream) {
  using namespace svk;
  SVK_REQUIRE(a != nullptr, SVK_ERR_VALUE, "svk_mla_decode_stage2: null args");
  SVK_REQUIRE(a->latent_dim == kMlaL, SVK_ERR_LAYOUT, "svk_mla_decode_stage2: latent_dim %d unsupported (512)", a->latent_dim);
  SVK_REQUIRE(a->num_heads >= 1 && a->num_heads <= 128, SVK_ERR_LAYOUT,
              "svk_mla_decode_stage2: num_heads %d unsupported (1..128)", a->num_heads);
  SVK_REQUIRE(a->block_seq > 0 && a->block_seq % kMlaTT == 0, SVK_ERR_LAYOUT,
              "svk_mla_decode_stage2: block_seq %d must be a positive multiple of %d", a->block_seq, kMlaTT);
  SVK_REQUIRE(a->mid_o && a->mid_lse && a->context_lens && a->output, SVK_ERR_VALUE,
              "svk_mla_decode_stage2: null tensor pointer");
  SVK_REQUIRE(a->mid_o_stride_b % 4 == 0 && a->mid_o_stride_h % 4 == 0 && a->mid_o_stride_s % 4 == 0 && al16(a->mid_o) &&
                  a->o_stride_b % 4 == 0 && a->o_stride_h % 4 == 0 && (reinterpret_cast<uintptr_t>(a->output) & 7) == 0,
              SVK_ERR_LAYOUT, "svk_mla_decode_stage2: mid_o needs 16-byte, output 8-byte aligned rows");
  SVK_REQUIRE(a->mid_lse_stride_b > 0 && a->mid_lse_stride_h > 0 && a->mid_o_stride_b > 0 && a->mid_o_stride_h > 0 &&
                  a->mid_o_stride_s >= kMlaL && a->o_stride_b > 0 && a->o_stride_h >= kMlaL,
              SVK_ERR_VALUE, "svk_mla_decode_stage2: mid_o / mid_lse / output strides must be positive (rows >= 512)");
  SVK_REQUIRE(a->batch >= 0 && a->batch <= 65535 && a->max_context_len > 0, SVK_ERR_VALUE,
              "svk_mla_decode_stage2: batch %d must lie in 0..65535 and max_context_len %d must be positive", a->batch,
              a->max_context_len);
  if (a->batch == 0) return SVK_OK;
  hipLaunchKernelGGL(mla_stage2_kernel, dim3(a->num_heads, a->batch), dim3(256), 0, static_cast<hipStream_t>(stream), *a);
  return check_launch("svk_mla_decode_stage2");
}

extern "C" int svk_mla_store_latent(const SvkMlaStoreLatentArgs* a, svk_stream_t stream) {
  using namespace svk;
  SVK_REQUIRE(a != nullptr, SVK_ERR_VALUE, "svk_mla_store_latent: null args");
  SVK_REQUIRE(a->latent_dim == kMlaL && a->rope_dim == kMlaR, SVK_ERR_LAYOUT,
              "svk_mla_store_latent: latent_dim %d / rope_dim %d unsupported (512 / 64)", a->latent_dim, a->rope_dim);
  SVK_REQUIRE(a->latent && a->rope && a->latent_cache && a->rope_cache && a->slot_mapping, SVK_ERR_VALUE,
              "svk_mla_store_latent: null tensor pointer");
  SVK_REQUIRE(a->latent_slot_stride % 8 == 0 && a->rope_slot_stride % 8 == 0 && a->latent_stride % 8 == 0 &&
                  a->rope_stride % 8 == 0 && al16(a->latent) && al16(a->rope) && al16(a->latent_cache) && al16(a->rope_cache),
              SVK_ERR_LAYOUT, "svk_mla_store_latent: pointers and row strides must keep 16-byte alignment");
  SVK_REQUIRE(a->num_slots > 0, SVK_ERR_VALUE, "svk_mla_store_latent: empty pool");
  if (a->n_tokens <= 0) return SVK_OK;
  const int64_t chunks = (int64_t)a->n_tokens * kMlaChunks;
  hipLaunchKernelGGL(mla_store_latent_kernel, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), *a);
  return check_launch("svk_mla_store_latent");
}

extern "C" int svk_mla_gather_latent(const SvkMlaGatherLatentArgs* a, svk_stream_t stream) {
  using namespace svk;
  SVK_REQUIRE(a != nullptr, SVK_ERR_VALUE, "svk_mla_gather_latent: null args");
  SVK_REQUIRE(a->latent_dim == kMlaL && a->rope_dim == kMlaR, SVK_ERR_LAYOUT,
              "svk_mla_gather_latent: latent_dim %d / rope_dim %d unsupported (512 / 64)", a->latent_dim, a->rope_dim);
  SVK_REQUIRE(a->latent_cache && a->rope_cache && a->active_slots && a->request_indices && a->context_lens &&
                  a->packed_start_locs && a->gathered_latent && a->gathered_rope,
              SVK_ERR_VALUE, "svk_mla_gather_latent: null tensor pointer");
  SVK_REQUIRE(a->latent_slot_stride >= kMlaL && a->latent_slot_stride % 8 == 0 && a->rope_slot_stride >= kMlaR &&
                  a->rope_slot_stride % 8 == 0 && a->out_latent_stride >= kMlaL && a->out_latent_stride % 8 == 0 &&
                  a->out_rope_stride >= kMlaR && a->out_rope_stride % 8 == 0 && al16(a->latent_cache) &&
                  al16(a->rope_cache) && al16(a->gathered_latent) && al16(a->gathered_rope),
              SVK_ERR_LAYOUT, "svk_mla_gather_latent: pointers and row strides must keep 16-byte alignment (rows >= 512 / 64)");
  SVK_REQUIRE(a->num_slots > 0 && a->slot_rows > 0 && a->out_capacity >= 0 && a->max_context_len >= 0 &&
                  a->slots_stride >= a->max_context_len,
              SVK_ERR_VALUE, "svk_mla_gather_latent: empty pool / slot table, negative capacity (%lld) or max_context_len (%d), "
              "or slots_stride %lld below max_context_len", (long long)a->out_capacity, a->max_context_len, (long long)a->slots_stride);
  SVK_REQUIRE(a->batch >= 0 && a->batch <= 65535, SVK_ERR_VALUE, "svk_mla_gather_latent: batch %d must lie in 0..65535", a->batch);
  if (a->batch == 0 || a->max_context_len == 0 || a->out_capacity == 0) return SVK_OK;
  const int64_t chunks = (int64_t)a->max_context_len * kMlaChunks;
  hipLaunchKernelGGL(mla_gather_latent_kernel, dim3((unsigned)((chunks + 255) / 256), a->batch), dim3(256), 0,
                     static_cast<hipStream_t>(stream), *a);
  return check_launch("svk_mla_gather_latent");
}
