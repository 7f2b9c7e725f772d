// Chunked-prefill causal attention at head_dim 256 (gfx950): MLA-expanded MHA and the 256-wide GQA models.
//
// Same contract as the head_dim 128 kernel of prefill_attention.hip (SvkContextAttentionArgs, base-2 online softmax,
// P rounded to bf16, fp32 accumulation), with the work split by ROWS instead of by query head:
//   * workgroup = (sequence, KV head, 128 rows of the flattened (query token, head within the GQA group) space); wave w
//     owns rows [32 w, 32 w + 32), token-major: 128 / G consecutive tokens x G heads.  All four waves walk the same keys,
//     so one K/V block in LDS serves 128 rows even in MHA (G = 1), where "wave = query head" would share nothing;
//   * ONE wave per SIMD (256 threads, one workgroup per CU): the wave has the unified 512-register file.  Q^T stays
//     resident (16 B fragments, 64 registers), O is eight 32x32 accumulators (128 registers), S of two blocks 32;
//   * keys come in blocks of 32 (1 KiB per key: 512 B of K + 512 B of V).  LDS holds a ring of three K blocks and a
//     ring of three V blocks (96 KiB); V trails K by two blocks because the pipeline below reads K(j+1) and V(j-1) in
//     step j.  Rows are fetched by global_load_lds_dwordx4 groups with the conflict-free swizzles applied on the DMA
//     SOURCE address: K position p of row `key` holds chunk p ^ (key & 15), V position p holds chunk p ^ 4 (key & 3);
//     every wave issues one K group (8 rows) and one V group per step.  Slot ids travel by global_load_lds_dword, 64 at
//     a time (two blocks), into a ring of three pairs;
//   * S^T = K Q^T on v_mfma_f32_32x32x16_bf16: a lane's 16 accumulators are 16 keys of ONE query row, the softmax is
//     lane-local plus one v_permlane32_swap, and P goes from the accumulators straight into the A operand of P V; V's B
//     operand comes out of the row-major block by ds_read_b64_tr_b16;
//   * step j of the software pipeline holds C(j-1): O += P V (16 MFMAs), B(j): softmax of S(j), A(j+1): S = K Q^T
//     (16 MFMAs): two products per softmax element, matrix and vector unit busy inside the one wave of the SIMD;
//   * lazy rescaling (the reference point of a row moves only when its maximum grew by more than 2^8), the causal mask
//     only on the blocks that reach a wave's diagonal, longest query tiles first, XCD-aware (tile, KV head) mapping,
//     32-bit row offsets below 4 GiB, epilogue through LDS into 16-byte stores.
// No atomics; a row's result depends on its keys' order in the slot table only, never on where the slots lie.

#include <type_traits>

#include "svk_common.hpp"
#include "lds_dma.hpp"

namespace svk {
namespace {

constexpr int kD = 256;
constexpr int kBlk = 32;                       // query rows per wave = keys per block
constexpr int kRowB = kD * 2;                  // bytes of one K or V head row
constexpr int kBlkB = kBlk * kRowB;            // 16 KiB: the K (or V) rows of one block
constexpr int kRing = 3;
constexpr int kVRing0 = kRing * kBlkB;         // the V ring lies behind the K ring
constexpr int kIds0 = 2 * kRing * kBlkB;       // 3 pairs x 64 slot ids | 4 x 32 floats (rescale factors / 1 / row sum)
constexpr int kShm = kIds0 + 3 * 64 * 4 + 4 * 32 * 4;
constexpr int kWgRows = 128;

typedef __attribute__((ext_vector_type(4))) short d2_s16x4_t;
typedef __attribute__((ext_vector_type(8))) short d2_s16x8_t;
typedef __attribute__((address_space(3))) unsigned char lds_byte_t;

// STATS: the score window's rows also leave their softmax statistics behind and the step-score rows are zeroed (svk.h:
// score_row_stats / score_clear); the instantiation without it is the kernel as it was.
template <bool OFF32, bool STATS>
__global__ void __launch_bounds__(256) context_attention_kernel_d256(const SvkContextAttentionArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int G = a.num_q_heads / a.num_kv_heads;          // 1, 2 or 4 (checked by the dispatcher)
  const int gs = G >> 1;                                 // log2 G
  const int q_tile = kWgRows >> gs;                      // query tokens of a workgroup
  const int b = blockIdx.z;
  // (query tile, KV head) of this workgroup: a KV head is served by 8 / Hkv XCDs when the grid allows it (see the
  // head_dim 128 kernel)
  int qt = blockIdx.x, kvh = blockIdx.y;
  {
    const unsigned nx = gridDim.x, ny = gridDim.y;
    if ((ny == 1 || ny == 2 || ny == 4 || ny == 8) && ((nx * ny) & 7) == 0) {
      const unsigned L = blockIdx.x + nx * blockIdx.y;
      const unsigned xcd = L & 7, j = L >> 3;
      kvh = xcd % ny;
      qt = j * (8 / ny) + xcd / ny;
    }
  }
  const int lq = lane & 31, half = lane >> 5;
  const int pc = a.b_prompt_cache_len[b];
  const int q_len = a.b_seq_len[b] - pc;
  const int m0 = ((int)gridDim.x - 1 - qt) * q_tile;     // longest key ranges first
  if (m0 >= q_len) return;
  const int start_loc = a.b_start_loc[b];
  const int kv_end = min(m0 + q_tile + pc, q_len + pc);  // keys visible to the last row of the workgroup
  const int nblk = (kv_end + kBlk - 1) / kBlk;
  // the lane's query row: flattened row 32 w + lq -> (token, head of the group)
  const int frow = w * kBlk + lq;
  const int qtok = m0 + (frow >> gs);
  const int head = kvh * G + (frow & (G - 1));
  const int wave_tok0 = m0 + ((w * kBlk) >> gs);         // first token of the wave: blocks below its diagonal skip the mask

  int* slot_lds = reinterpret_cast<int*>(lds_raw + kIds0);
  float* fac = reinterpret_cast<float*>(slot_lds + 3 * 64) + w * 32;
  const uint32_t lds0 = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(lds_byte_t*)lds_raw);
  const int32_t* row = a.req_to_tokens + (int64_t)a.b_req_idx[b] * a.req_stride;

  // Q^T fragments (B operand): lane (q = lq, half) holds Q[qtok][head][ds*16 + half*8 .. +8]
  bf16x8_t qb[kD / 16];
  {
    const uint16_t* qp = a.q + (int64_t)(start_loc + min(qtok, q_len - 1)) * a.q_stride_t + (int64_t)head * a.q_stride_h + half * 8;
#pragma unroll
    for (int ds = 0; ds < kD / 16; ++ds) qb[ds] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(qp + ds * 16));
  }
  const float sm_scale = 0.0625f * 1.4426950408889634f;  // 256^-1/2 log2 e
  const float mask_raw = -1.0e8f / sm_scale;
  float m_run = -INFINITY, l_part = 0.f;                 // of query row lq (both halves keep the same maximum)
  f32x16_t o[8];                                         // o[i][r]: query row (r&3) + 8(r>>2) + 4 half, head dim 32 i + lq
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[i][r] = 0.f;

  // ---- DMA: a block is 16 + 16 instructions of 1 KiB (two 512-byte rows each) = 4 K groups + 4 V groups of four
  //      instructions behind one M0 write; wave w issues group w of both: rows 8 w + 2 i + (lane >> 5).  Everything about a
  //      lane's source address except the slot id is a constant (the swizzled chunk, the head, the instruction bias).
  const char* const kt = reinterpret_cast<const char*>(a.k_cache);
  const char* const vt = reinterpret_cast<const char*>(a.v_cache);
  const int64_t slot_bytes = a.kv_slot_stride * 2;
  const uint32_t slot_b32 = (uint32_t)slot_bytes;
  const uint32_t head_bytes = (uint32_t)((int64_t)kvh * a.kv_head_stride * 2);
  const uint32_t lane_row = lane >> 5, lane_pos = lane & 31;
  uint32_t kc[4], vc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t key = 8 * w + 2 * i + lane_row;
    kc[i] = head_bytes + ((lane_pos ^ (key & 15)) << 4) + 3072 - 1024 * i;
    vc[i] = head_bytes + ((lane_pos ^ ((key & 3) << 2)) << 4) + 3072 - 1024 * i;
  }
  auto issue_rows = [&](int blk, auto is_v_c) {
    constexpr bool is_v = decltype(is_v_c)::value;
    const int* ids = slot_lds + ((blk >> 1) % 3) * 64 + (blk & 1) * 32 + 8 * w + lane_row;
    int slot[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) slot[i] = ids[2 * i];
    const uint32_t dst = lds0 + (is_v ? kVRing0 : 0) + (blk % kRing) * kBlkB + w * 4096;
    if constexpr (OFF32) {
      uint32_t voff[4];
      // (slot < 2^24: a slot is >= 512 bytes and the tensor < 4 GiB)
#pragma unroll
      for (int i = 0; i < 4; ++i) voff[i] = __umul24((uint32_t)slot[i], slot_b32) + (is_v ? vc[i] : kc[i]);
      pa_dma4x16_off32(voff, (is_v ? vt : kt) - 3072, dst);
    } else {
      const char* src[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) src[i] = (is_v ? vt : kt) + ((int64_t)slot[i] * slot_bytes + (int64_t)(is_v ? vc[i] : kc[i]) - 3072);
      pa_dma4x16(src, dst);
    }
  };
  // slot ids of blocks 2 p and 2 p + 1 (wave 0): 64 x 4 bytes by LDS-DMA, clamped to the last visible key (a legal row)
  auto issue_ids = [&](int p) {
    if (w == 0) {
      const int32_t* src = row + min(p * 64 + lane, kv_end - 1);
      uint32_t keep;
      const uint32_t dst = __builtin_amdgcn_readfirstlane(
          (uint32_t)(uintptr_t)(__attribute__((address_space(3))) int*)(slot_lds + (p % 3) * 64));
      asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
                   : "=&s"(keep) : "v"(src), "s"(dst) : "memory");
    }
  };
  // K fragment addresses (A operand of S^T = K Q^T): lane (key row lq, k-chunk ds*2 + half) through the K swizzle
  uint32_t kaddr[kD / 16];
#pragma unroll
  for (int ds = 0; ds < kD / 16; ++ds)
    kaddr[ds] = (uint32_t)(uintptr_t)(lds_byte_t*)lds_raw + lq * kRowB + (((ds * 2 + half) ^ (lq & 15)) << 4);
  // transpose-read addresses into V ring slot 0: lane (group member q = lane & 15) points at key (q >> 2) + 4 half of a
  // block of 8 keys, dims 32 i + 16 (lq >> 4) + 4 (q & 3) .. + 3, through the V swizzle
  uint32_t vbase[8];
  {
    const uint32_t q16 = lane & 15;
    const uint32_t v0 = (uint32_t)(uintptr_t)(lds_byte_t*)lds_raw + kVRing0 + ((q16 >> 2) + 4 * half) * kRowB + (lq >> 4) * 32 + (q16 & 3) * 8;
#pragma unroll
    for (int i = 0; i < 8; ++i) vbase[i] = v0 + ((i ^ (q16 >> 2)) << 6);
  }

  // ---- prologue: ids of blocks 0..3, then K(0..2) and V(0); step 0 multiplies the rows of V ring slot 2 by P = 0: finite
  issue_ids(0);
  if (nblk > 2) issue_ids(1);
  for (int i = threadIdx.x; i < kBlkB / 16; i += blockDim.x)
    *reinterpret_cast<uint4*>(lds_raw + kVRing0 + 2 * kBlkB + i * 16) = make_uint4(0u, 0u, 0u, 0u);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  issue_rows(0, std::false_type{});
  issue_rows(0, std::true_type{});
  if (nblk > 1) issue_rows(1, std::false_type{});
  if (nblk > 2) issue_rows(2, std::false_type{});
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
#pragma unroll
  for (int ds = 0; ds < kD / 16; ++ds) asm volatile("" : "+v"(qb[ds]));

  f32x16_t s_a, s_b;                                     // S of the even / odd block
  {
    pa_u32x4_t ka[kD / 16];
#pragma unroll
    for (int ds = 0; ds < kD / 16; ++ds) ka[ds] = *reinterpret_cast<const __attribute__((address_space(3))) pa_u32x4_t*>(kaddr[ds]);
#pragma unroll
    for (int ds = 0; ds < kD / 16; ++ds)
      s_a = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, ka[ds]), qb[ds], ds == 0 ? f32x16_t{} : s_a, 0, 0, 0);
  }
  uint32_t pp_a[8], pp_b[8];                             // P of the even / odd block as bf16 pairs (A operand of P V)
#pragma unroll
  for (int e = 0; e < 8; ++e) pp_a[e] = pp_b[e] = 0u;
  uint32_t k_next = kBlkB, v_prev = 2 * kBlkB;           // ring offsets of K(j+1) and V(j-1)

  // Step j.  Behind its barrier K(j+1) and V(j-1) have landed for every wave (issued two barriers ago; the wait leaves the
  // eight row instructions of the previous step in flight), and K(j), V(j-2) and the ids of blocks < j are dead: K(j+3)
  // takes K(j)'s slot, V(j+1) takes V(j-2)'s, and on even j the ids of blocks j+4, j+5 go out FIRST so that the counted
  // wait of the next step covers them.
  auto step = [&](int j, f32x16_t& s_in, f32x16_t& s_out, const uint32_t (&p_prev)[8], uint32_t (&p_out)[8])
                  __attribute__((always_inline)) {
    if (j + 2 < nblk) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if ((j & 1) == 0 && j + 4 < nblk) issue_ids((j >> 1) + 2);
    if (j + 3 < nblk) issue_rows(j + 3, std::false_type{});
    if (j + 1 < nblk) issue_rows(j + 1, std::true_type{});
    const int k0 = j * kBlk;
    pa_u32x4_t ka[kD / 16];
#pragma unroll
    for (int ds = 0; ds < kD / 16; ++ds) ka[ds] = *reinterpret_cast<const __attribute__((address_space(3))) pa_u32x4_t*>(kaddr[ds] + k_next);
    d2_s16x4_t vr[2][8][2];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const auto* vp = reinterpret_cast<__attribute__((address_space(3))) d2_s16x4_t*>(vbase[i] + v_prev);
#pragma unroll
      for (int sp = 0; sp < 2; ++sp)
#pragma unroll
        for (int eh = 0; eh < 2; ++eh)
          vr[sp][i][eh] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(const_cast<__attribute__((address_space(3))) d2_s16x4_t*>(vp) + (sp * 16 + eh * 8) * kRowB / 8);
    }
    if (k0 + kBlk > wave_tok0 + pc + 1 || k0 + kBlk > kv_end) {
      // only the blocks on the wave's diagonal / at the end of the row: branch-free selects (register r = key k0 +
      // (r&3) + 8(r>>2) + 4 half)
      const int lim = min(qtok + pc, kv_end - 1) - k0 - 4 * half;
#pragma unroll
      for (int r = 0; r < 16; ++r) s_in[r] = ((r & 3) + 8 * (r >> 2) <= lim) ? s_in[r] : mask_raw;
    }
    float mx = vmax(vmax3(vmax3(s_in[0], s_in[1], s_in[2]), vmax3(s_in[3], s_in[4], s_in[5]), s_in[15]),
                    vmax3(vmax3(s_in[6], s_in[7], s_in[8]), vmax3(s_in[9], s_in[10], s_in[11]), vmax3(s_in[12], s_in[13], s_in[14])));
    mx = vmax(mx, lane_xor32(mx));
    const float nm_true = vmax(m_run, mx);
    const bool moved = (nm_true - m_run) * sm_scale > 8.0f;
    const float nm = moved ? nm_true : m_run;
    const float nms = nm * sm_scale;
    const float al = moved ? __builtin_amdgcn_exp2f(m_run * sm_scale - nms) : 1.0f;
    m_run = nm;
    // A(j+1) (a dependent chain), C(j-1) (independent products) and the softmax of one S register alternate; scheduling
    // barriers keep this order.  C product (sp, i) uses the keys of registers [8 sp, 8 sp + 8) and head dims 32 i + lq.
    float psum = 0.f;
    {
      const bf16x8_t pa0 = __builtin_bit_cast(bf16x8_t, make_uint4(p_prev[0], p_prev[1], p_prev[2], p_prev[3]));
      const bf16x8_t pa1 = __builtin_bit_cast(bf16x8_t, make_uint4(p_prev[4], p_prev[5], p_prev[6], p_prev[7]));
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        s_out = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, ka[g]), qb[g], g == 0 ? f32x16_t{} : s_out, 0, 0, 0);
        {
          const int sp = g >> 3, i = g & 7;
          const d2_s16x8_t vb = __builtin_shufflevector(vr[sp][i][0], vr[sp][i][1], 0, 1, 2, 3, 4, 5, 6, 7);
          o[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(sp ? pa1 : pa0, __builtin_bit_cast(bf16x8_t, vb), o[i], 0, 0, 0);
        }
        s_in[g] = __builtin_amdgcn_exp2f(__builtin_fmaf(s_in[g], sm_scale, -nms));
        psum += s_in[g];
        if (g & 1) p_out[g >> 1] = pack_bf16(s_in[g - 1], s_in[g]);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    l_part = l_part * al + psum;
#pragma unroll
    for (int e = 0; e < 8; ++e) asm volatile("" : "+v"(p_out[e]));
    asm volatile("" : "+v"(l_part));
    if (__any(moved)) {
      // O lives in accumulation registers.  Without this pin hipcc hoists the 128 v_accvgpr_read of the rescale above the
      // branch, behind the last product of every accumulator, where they stall the matrix pipe in every step.
#pragma unroll
      for (int i = 0; i < 8; ++i) asm volatile("" : "+a"(o[i]));
      // rescale factors: "lane = query row" -> "register = query row" through the wave's LDS row
      if (half == 0) fac[lq] = al;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const float4 f4 = *reinterpret_cast<const float4*>(fac + 8 * jj + 4 * half);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          o[i][4 * jj + 0] *= f4.x; o[i][4 * jj + 1] *= f4.y; o[i][4 * jj + 2] *= f4.z; o[i][4 * jj + 3] *= f4.w;
        }
      }
      __builtin_amdgcn_wave_barrier();
    }
    k_next = k_next == 2 * kBlkB ? 0 : k_next + kBlkB;
    v_prev = v_prev == 2 * kBlkB ? 0 : v_prev + kBlkB;
  };
  for (int j = 0; j < nblk; j += 2) {
    step(j, s_a, s_b, pp_b, pp_a);
    if (j + 1 < nblk) step(j + 1, s_b, s_a, pp_a, pp_b);
  }
  // C of the last block: its V rows were issued behind the last barrier
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  {
    uint32_t pp[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) pp[e] = (nblk & 1) ? pp_a[e] : pp_b[e];
    d2_s16x4_t vr[2][8][2];
#pragma unroll
    for (int sp = 0; sp < 2; ++sp)
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int eh = 0; eh < 2; ++eh)
          vr[sp][i][eh] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(reinterpret_cast<__attribute__((address_space(3))) d2_s16x4_t*>(
              vbase[i] + v_prev + (uint32_t)((sp * 16 + eh * 8) * kRowB)));
#pragma unroll
    for (int sp = 0; sp < 2; ++sp) {
      const bf16x8_t pa = __builtin_bit_cast(bf16x8_t, make_uint4(pp[4 * sp], pp[4 * sp + 1], pp[4 * sp + 2], pp[4 * sp + 3]));
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const d2_s16x8_t vb = __builtin_shufflevector(vr[sp][i][0], vr[sp][i][1], 0, 1, 2, 3, 4, 5, 6, 7);
        o[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa, __builtin_bit_cast(bf16x8_t, vb), o[i], 0, 0, 0);
      }
    }
  }
  __syncthreads();                                       // (the epilogue stages through the K/V rings)
  // ---- epilogue: row sums across the two halves, 1/l into register-row layout, outputs through LDS as whole rows
  l_part += lane_xor32(l_part);
  if constexpr (STATS) {
    if (a.score_row_stats != nullptr && half == 0) {
      // the base-2 exponent constant of the row, m * c + log2 l, for the token-score pass.  With lazy rescaling m_run is
      // a reference point, not the row maximum: the sum is the same number for any reference point.
      const int qs = a.score_q_start[b];
      const int r = pc + qtok - qs;
      if (qs >= 0 && r >= 0 && r < a.score_wpad && qtok < q_len)
        a.score_row_stats[((int64_t)b * a.num_q_heads + head) * a.score_wpad + r] = m_run * sm_scale + __builtin_amdgcn_logf(l_part);
    }
    if (a.score_clear != nullptr && kvh == 0 && m0 + q_tile >= q_len) {
      // one workgroup per sequence (the tile that holds the chunk's last rows, KV head 0) zeroes the sequence's score row
      float* dst = a.score_clear + (int64_t)b * a.score_clear_stride;
      for (int c = threadIdx.x; c < a.score_clear_cols; c += 256) dst[c] = 0.f;
    }
  }
  if (half == 0) fac[lq] = 1.0f / l_part;
  uint16_t* ost = reinterpret_cast<uint16_t*>(lds_raw + (size_t)w * (kBlk * kRowB));       // [32 rows][256] bf16 per wave
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) {
    const float4 f4 = *reinterpret_cast<const float4*>(fac + 8 * jj + 4 * half);
    const float f[4] = {f4.x, f4.y, f4.z, f4.w};
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int r3 = 0; r3 < 4; ++r3) {
        const int qr = 8 * jj + 4 * half + r3;
        ost[qr * kD + 32 * i + lq] = (uint16_t)f32_to_bf16_bits(o[i][4 * jj + r3] * f[r3]);
      }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  // 32 rows x 512 B: lane -> (row = it*2 + lane/32, 16-byte piece lane%32)
#pragma unroll
  for (int it = 0; it < 16; ++it) {
    const int qr = it * 2 + (lane >> 5);
    const int fr = w * kBlk + qr;
    const int tok = m0 + (fr >> gs);
    if (tok < q_len)
      *reinterpret_cast<uint4*>(a.o + (int64_t)(start_loc + tok) * a.o_stride_t + (int64_t)(kvh * G + (fr & (G - 1))) * a.o_stride_h + (lane & 31) * 8) =
          *reinterpret_cast<const uint4*>(ost + qr * kD + (lane & 31) * 8);
  }
}

}  // namespace

// Launch of the head_dim 256 kernel for svk_context_attention_fwd (arguments already validated; G in {1, 2, 4}).
int launch_context_attention_d256(const SvkContextAttentionArgs& a, int max_input_len, bool off32, hipStream_t s) {
  static const hipError_t attr = [] {
    const void* const kernels[4] = {reinterpret_cast<const void*>(context_attention_kernel_d256<true, false>),
                                    reinterpret_cast<const void*>(context_attention_kernel_d256<false, false>),
                                    reinterpret_cast<const void*>(context_attention_kernel_d256<true, true>),
                                    reinterpret_cast<const void*>(context_attention_kernel_d256<false, true>)};
    for (const void* k : kernels) {
      const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, kShm);
      if (e != hipSuccess) return e;
    }
    return hipSuccess;
  }();
  if (attr != hipSuccess) {
    set_error("svk_context_attention_fwd: cannot reserve %d bytes of LDS per workgroup: %s", kShm, hipGetErrorString(attr));
    return SVK_ERR_LAUNCH;
  }
  const int G = a.num_q_heads / a.num_kv_heads;
  const int q_tile = kWgRows / G;
  const dim3 grid((max_input_len + q_tile - 1) / q_tile, a.num_kv_heads, a.batch);
  const bool stats = a.score_row_stats != nullptr || a.score_clear != nullptr;
  if (stats) {
    if (off32) hipLaunchKernelGGL((context_attention_kernel_d256<true, true>), grid, dim3(256), (size_t)kShm, s, a);
    else hipLaunchKernelGGL((context_attention_kernel_d256<false, true>), grid, dim3(256), (size_t)kShm, s, a);
  } else {
    if (off32) hipLaunchKernelGGL((context_attention_kernel_d256<true, false>), grid, dim3(256), (size_t)kShm, s, a);
    else hipLaunchKernelGGL((context_attention_kernel_d256<false, false>), grid, dim3(256), (size_t)kShm, s, a);
  }
  return check_launch("svk_context_attention_fwd (head_dim 256)");
}

}  // namespace svk
