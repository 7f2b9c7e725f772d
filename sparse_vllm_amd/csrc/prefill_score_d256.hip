// Prefill token scores at head_dim 256 (gfx950): MLA-expanded MHA and the 256-wide GQA models (G = 1, 2, 4, 8).
//
// Same contract and the same arithmetic as prefill_score_kernel_v2 (SvkPrefillScoreArgs; two-pass softmax statistics
// that travel as m c + log2 l, c = 256^-1/2 log2 e; masked value -1e20; integer atomic max across the KV heads), the
// same (128-key block, score range, KV head) workgroup, partial-statistics layout and reduce kernel - with the work
// split by ROWS instead of by query head:
//   * a workgroup always has four waves.  The work is the flattened space (head g of the GQA group, 32-row block rb of
//     the window): G * Wpad32 / 32 items in head-major order, dealt to the waves in contiguous runs of ceil(items / 4).
//     Every wave consumes the same K tile for any G, so the tile is shared four ways in MHA (G = 1) too, where
//     "wave = query head" would leave one wave per tile;
//   * the K tile is 128 keys x 512 B = 64 KiB of LDS, fetched once per workgroup by global_load_lds_dwordx4 (an
//     instruction moves two rows; groups of four behind one M0 write, four groups per wave).  Position p of row `key`
//     holds chunk p ^ (key & 15), applied on the DMA SOURCE address: a 16-byte fragment read of 16 consecutive rows at
//     the 512-byte stride (all rows start on bank 0) then touches 16 different chunks of the 256-byte bank window, for
//     every k-step and both halves (bit 4 of the chunk index passes through the swizzle; it selects a half-row that
//     maps onto the same banks).  Tile + per-wave key partials = 70 KiB: two workgroups per CU, one's K fetch and Q
//     loads under the other's products;
//   * v_mfma_f32_32x32x16_bf16, 16 k-steps per 32 x 32 block: S^T = K Q^T for the statistics pass (a lane holds 16 keys
//     of ONE query row), S = Q K^T for the final pass and the logits mode (a lane holds 16 query rows of ONE key; the
//     per-key accumulator is a register);
//   * two resident workgroups are two waves per SIMD, i.e. 256 registers per wave: the Q fragments of a block (64) and
//     the K fragments of a 32-key sub-block read in ONE batch (64) both fit, see docs/KERNELS.md for the report;
//   * per key: a wave keeps the sum (final pass) or maximum (logits) of the head it is in and writes it to its own LDS
//     row when its run moves to the next head (a run touches at most three heads); one owner thread per key column
//     adds the waves' partials of every head in wave order (no LDS atomics: the sum is deterministic), takes the maximum
//     over the heads and publishes by integer atomicMax.  The pass-0 workgroup of KV head 0 clears its 128 columns;
//   * the mask only on blocks that touch the diagonal, a candidate-range end or padded rows (v2's `fast` predicate).

#include "prefill_score_common.hpp"

namespace svk {
namespace {

constexpr int kD = 256;
constexpr int kRowB = kD * 2;                  // bytes of a K head row
constexpr int kTileB = kPsKeys * kRowB;        // 64 KiB
constexpr int kWaves = 4;
// heads a wave's run can touch: a run of P = ceil(G nrb / 4) items spans at most (P + nrb - 2) / nrb + 1 heads, which is
// <= 3 for G <= 8, nrb <= 4 (the worst cases are P = 7, nrb = 4 and P = 5, nrb = 3; P = 8 runs start on a head boundary)
constexpr int kHeadSlots = 3;
constexpr int kShm = kTileB + kWaves * kHeadSlots * kPsKeys * (int)sizeof(float);
constexpr int kKSteps = kD / 16;
constexpr int kKBatch = 16;                    // k-steps whose K fragments are read together (8: two batches)

typedef __attribute__((address_space(3))) unsigned char lds_byte_t;

// PASS: 0 = partial stats, 1 = final probabilities, 2 = logits
template <int PASS>
__global__ void __launch_bounds__(64 * kWaves, 2) prefill_score_kernel_d256(const SvkPrefillScoreArgs a, int G, int Wpad32, int q_limit,
                                                                            int NKB, float* part_m, float* part_l,
                                                                            const float* glob_ml) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];      // K tile [128][512 B] | hsw[4][3][128] f32
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lq = lane & 31, half = lane >> 5;
  const int kb = blockIdx.x;
  const int h = blockIdx.y % a.num_kv_heads, i = blockIdx.y / a.num_kv_heads;
  const RangeInfo R = load_range(a, i);
  const int k0 = kb * kPsKeys;
  const int key_lo = max(k0, a.candidate_start), key_hi = min(k0 + kPsKeys, R.cand_end);
  const int ROWS = G * Wpad32;
  const int nrb = Wpad32 / 32;
  const int64_t grp = (int64_t)i * a.num_kv_heads + h;
  float* hsw = reinterpret_cast<float*>(lds_raw + kTileB);
  if (PASS == 0 && h == 0) {
    // the score row starts from 0 (pass 1 publishes by atomic max): this range's workgroup of KV head 0 clears its
    // 128 columns here, so the probability mode needs no fill launch
    float* dst = a.attn_score + (int64_t)i * a.score_stride;
    for (int c = k0 + (int)threadIdx.x; c < min(k0 + kPsKeys, a.score_cols); c += blockDim.x) dst[c] = 0.f;
  }
  if (key_lo >= key_hi) {
    if (PASS == 0)
      for (int r = threadIdx.x; r < ROWS; r += blockDim.x) {
        const int64_t o = (grp * NKB + kb) * ROWS + r;
        part_m[o] = kMasked;
        part_l[o] = 0.f;
      }
    return;
  }
  // this wave's run of (head, row block) items
  const int n_items = G * nrb;
  const int per = (n_items + kWaves - 1) / kWaves;
  const int it0 = w * per, it1 = min(n_items, it0 + per);
  const int g_first = it0 / nrb;
  // Q fragments of an item (lane = (row lq of the 32-row block, 8-element half of every 16-wide k-step); the same registers
  // serve as the B operand of K Q^T and the A operand of Q K^T) and, for pass 1, the row constants m c + log2 l in the
  // "register = row" layout of the accumulator.  The first item is requested before the K tile lands.
  bf16x8_t qf[kKSteps];
  float rm[16];
  auto load_block = [&](int g, int rb) __attribute__((always_inline)) {
    const int qi = rb * 32 + lq;
    const int qabs = R.q_start + qi;
    const int rel = qabs - R.cache_len;
    const bool ok = qi < q_limit && qabs < R.q_end && rel >= 0 && rel < R.chunk_len;
    const uint16_t* qp = a.q + (int64_t)(R.start_loc + (ok ? rel : 0)) * a.q_stride_t + (int64_t)(h * G + g) * a.q_stride_h + half * 8;
#pragma unroll
    for (int ds = 0; ds < kKSteps; ++ds) {
      uint4 t = make_uint4(0, 0, 0, 0);
      if (ok) t = *reinterpret_cast<const uint4*>(qp + ds * 16);
      qf[ds] = __builtin_bit_cast(bf16x8_t, t);
    }
    if (PASS == 1) {
      const float* gm = glob_ml + grp * ROWS + g * Wpad32 + rb * 32 + 4 * half;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float4 x = *reinterpret_cast<const float4*>(gm + 8 * j);
        rm[4 * j] = x.x; rm[4 * j + 1] = x.y; rm[4 * j + 2] = x.z; rm[4 * j + 3] = x.w;
      }
    }
  };
  if (it0 < it1) load_block(g_first, it0 - g_first * nrb);
  // ---- K tile -> LDS: 64 DMA instructions (2 keys each) = 16 groups of four behind one M0 write, four groups per wave
  {
    const uint32_t lds0 = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(lds_byte_t*)lds_raw);
    const char* kt = reinterpret_cast<const char*>(a.k_cache) + (int64_t)h * a.kv_head_stride * 2;
    const int64_t slot_bytes = a.kv_slot_stride * 2;
    const int lane_row = lane >> 5, lane_pos = lane & 31;
    for (int g8 = w; g8 < kPsKeys / 8; g8 += kWaves) {
      const char* src[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int key = 8 * g8 + 2 * j + lane_row;
        const int slot = R.row[min(k0 + key, key_hi - 1)];
        src[j] = kt + ((int64_t)slot * slot_bytes + (int64_t)((lane_pos ^ (key & 15)) << 4) - 1024 * j);
      }
      pa_dma4x16(src, lds0 + g8 * 4096);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  const float c2 = 0.0625f * 1.4426950408889634f;                               // logits -> base-2 exponent domain
  const uint32_t kfrag0 = (uint32_t)(uintptr_t)(lds_byte_t*)lds_raw + lq * kRowB;
  float acc[4];                                                                 // pass 1 / 2: per key sub-block, lane = key
#pragma unroll
  for (int sb = 0; sb < 4; ++sb) acc[sb] = PASS == 2 ? -INFINITY : 0.f;
  // the head's partial of this wave: both halves of the rows combined, into the wave's LDS row of the head
  auto flush = [&](int g) __attribute__((always_inline)) {
    float* dst = hsw + (w * kHeadSlots + (g - g_first)) * kPsKeys;
#pragma unroll
    for (int sb = 0; sb < 4; ++sb) {
      const float o = lane_xor32(acc[sb]);
      const float v = PASS == 1 ? acc[sb] + o : fmaxf(acc[sb], o);
      if (half == 0) dst[sb * 32 + lq] = v;
      acc[sb] = PASS == 2 ? -INFINITY : 0.f;
    }
  };

  int g_cur = g_first;
  for (int it = it0; it < it1; ++it) {
    const int g = it / nrb, rb = it - g * nrb;
    if (PASS != 0 && g != g_cur) {
      flush(g_cur);
      g_cur = g;
    }
    // query row rb*32 + lq of head g (lanes lq and lq + 32 hold the two 8-element halves of every 16-wide k-step)
    const int qi = rb * 32 + lq;
    const int qabs = R.q_start + qi;
    const int rel = qabs - R.cache_len;
    const bool ok = qi < q_limit && qabs < R.q_end && rel >= 0 && rel < R.chunk_len;
    const bool rows_ok = __all(ok);
    const int minpos = R.q_start + rb * 32;                                     // position of the block's first row
    if (it > it0) load_block(g, rb);
    float m2 = kMasked, l = 0.f;                                                // pass 0: this lane's (row, key half) pair
#pragma unroll
    for (int sb = 0; sb < 4; ++sb) {
      const int t0 = k0 + sb * 32;
      if (t0 + 32 <= key_lo || t0 >= key_hi) continue;
      f32x16_t s;
#pragma unroll
      for (int b0 = 0; b0 < kKSteps; b0 += kKBatch) {
        pa_u32x4_t kf[kKBatch];
#pragma unroll
        for (int ds = 0; ds < kKBatch; ++ds)
          kf[ds] = *reinterpret_cast<const __attribute__((address_space(3))) pa_u32x4_t*>(
              kfrag0 + sb * 32 * kRowB + ((((b0 + ds) * 2 + half) ^ (lq & 15)) << 4));
#pragma unroll
        for (int ds = 0; ds < kKBatch; ++ds) asm volatile("" : "+v"(kf[ds]));   // one batch of reads, one wait
#pragma unroll
        for (int ds = 0; ds < kKBatch; ++ds) {
          if (PASS == 0) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, kf[ds]), qf[b0 + ds], b0 + ds == 0 ? f32x16_t{} : s, 0, 0, 0);
          else s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qf[b0 + ds], __builtin_bit_cast(bf16x8_t, kf[ds]), b0 + ds == 0 ? f32x16_t{} : s, 0, 0, 0);
        }
      }
      // every logit of the block is live: keys inside the candidate range, rows real, all keys at or before the rows
      const bool fast = t0 >= key_lo && t0 + 32 <= key_hi && rows_ok && t0 + 31 <= minpos;
      if (PASS == 0) {
        // register r = key t0 + (r&3) + 8(r>>2) + 4 half of query row lq
        if (!fast) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int t = t0 + (r & 3) + 8 * (r >> 2) + 4 * half;
            const bool valid = ok && t >= key_lo && t < key_hi && qabs >= t;
            s[r] = valid ? s[r] * c2 : kMasked;
          }
        } else {
#pragma unroll
          for (int r = 0; r < 16; ++r) s[r] *= c2;
        }
        const float nm = vmax(m2, ps_max16(s));
        float psum = 0.f;
        if (!fast) {
#pragma unroll
          for (int r = 0; r < 16; ++r) psum += s[r] > 0.5f * kMasked ? __builtin_amdgcn_exp2f(s[r] - nm) : 0.f;
        } else {
#pragma unroll
          for (int r = 0; r < 16; ++r) psum += __builtin_amdgcn_exp2f(s[r] - nm);
        }
        l = l * __builtin_amdgcn_exp2f(m2 - nm) + psum;
        m2 = nm;
      } else {
        // lane = key t0 + lq, register r = query row rb*32 + (r&3) + 8(r>>2) + 4 half
        const int t = t0 + lq;
        const bool kin = t >= key_lo && t < key_hi;
        if (PASS == 1) {
          float cs = 0.f;
          if (fast) {
#pragma unroll
            for (int r = 0; r < 16; ++r) cs += __builtin_amdgcn_exp2f(__builtin_fmaf(s[r], c2, -rm[r]));
          } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int qr = rb * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
              const int qa_r = R.q_start + qr, rel_r = qa_r - R.cache_len;
              const bool valid = kin && qr < q_limit && qa_r < R.q_end && rel_r >= 0 && rel_r < R.chunk_len && qa_r >= t;
              cs += valid ? __builtin_amdgcn_exp2f(__builtin_fmaf(s[r], c2, -rm[r])) : 0.f;
            }
          }
          acc[sb] += cs;
        } else {
          float cm = -INFINITY;
          if (fast) {
            cm = ps_max16(s);
          } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int qr = rb * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
              const int qa_r = R.q_start + qr, rel_r = qa_r - R.cache_len;
              const bool valid = kin && qr < q_limit && qa_r < R.q_end && rel_r >= 0 && rel_r < R.chunk_len && qa_r >= t;
              cm = fmaxf(cm, valid ? s[r] : kMasked);
            }
          }
          acc[sb] = fmaxf(acc[sb], cm);
        }
      }
    }
    if (PASS == 0) {
      // the two halves of a row saw different keys: (m, l) pairs combine as M = max m, L = sum l 2^(m - M)
      const float mo = lane_xor32(m2), lo = lane_xor32(l);
      const float M = vmax(m2, mo);
      const float L = l * __builtin_amdgcn_exp2f(m2 - M) + lo * __builtin_amdgcn_exp2f(mo - M);
      if (half == 0) {
        const int64_t o = (grp * NKB + kb) * ROWS + g * Wpad32 + rb * 32 + lq;
        part_m[o] = M;
        part_l[o] = L;
      }
    }
  }
  if (PASS == 0) return;
  if (it0 < it1) flush(g_cur);
  __syncthreads();
  // ---- per key: every head's partials in wave order, x 1/W, then the maximum over the heads of the group
  const int c = threadIdx.x;
  const int t = k0 + c;
  if (c >= kPsKeys || t < key_lo || t >= key_hi) return;
  const float inv_len = 1.f / (float)max(R.q_end - R.q_start, 1);
  float best = -INFINITY;
  for (int g = 0; g < G; ++g) {
    float v = PASS == 1 ? 0.f : -INFINITY;
    for (int w2 = 0; w2 < kWaves; ++w2) {
      const int j0 = w2 * per, j1 = min(n_items, j0 + per);
      if (j0 >= j1) break;
      const int gf = j0 / nrb, gl = (j1 - 1) / nrb;
      if (g < gf || g > gl) continue;
      const float x = hsw[(w2 * kHeadSlots + (g - gf)) * kPsKeys + c];
      v = PASS == 1 ? v + x : fmaxf(v, x);
    }
    best = fmaxf(best, PASS == 1 ? v * inv_len : v);
  }
  float* dst = a.attn_score + (int64_t)i * a.score_stride + t;
  if (PASS == 1) atomic_max_nonneg(dst, fmaxf(best, 0.f));
  else atomic_max_any(dst, best);
}

template <int PASS>
int launch_pass(const SvkPrefillScoreArgs& a, int G, int Wpad32, int q_limit, int NKB, float* part_m, float* part_l,
                const float* glob_ml, hipStream_t s) {
  static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(prefill_score_kernel_d256<PASS>),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, kShm);
  if (attr != hipSuccess) {
    set_error("svk_prefill_score: cannot reserve %d bytes of LDS per workgroup: %s", kShm, hipGetErrorString(attr));
    return SVK_ERR_LAUNCH;
  }
  const dim3 grid(NKB, (unsigned)(a.n_ranges * a.num_kv_heads));
  hipLaunchKernelGGL((prefill_score_kernel_d256<PASS>), grid, dim3(64 * kWaves), (size_t)kShm, s, a, G, Wpad32, q_limit, NKB, part_m,
                     part_l, glob_ml);
  return check_launch("svk_prefill_score (head_dim 256)");
}

}  // namespace

// One pass of the head_dim 256 kernel for svk_prefill_score (arguments already validated; G <= 8, Wpad32 <= 128).
int launch_prefill_score_d256(const SvkPrefillScoreArgs& a, int pass, int G, int Wpad32, int q_limit, int NKB, float* part_m,
                              float* part_l, const float* glob_ml, hipStream_t s) {
  if (pass == 0) return launch_pass<0>(a, G, Wpad32, q_limit, NKB, part_m, part_l, glob_ml, s);
  if (pass == 1) return launch_pass<1>(a, G, Wpad32, q_limit, NKB, part_m, part_l, glob_ml, s);
  return launch_pass<2>(a, G, Wpad32, q_limit, NKB, part_m, part_l, glob_ml, s);
}

}  // namespace svk
