// Pieces shared by the prefill token-score kernels (prefill_score.hip, prefill_score_d256.hip): the score range
// descriptor, the masked value, the order-preserving float maxima and the 128-key block of the LDS-tile kernels.
#pragma once

#include "svk_common.hpp"
#include "lds_dma.hpp"

namespace svk {
namespace {

constexpr float kMasked = -1.0e20f;
constexpr int kPsKeys = 128;                   // keys of a workgroup of the LDS-tile kernels (v2, head_dim 256)

__device__ __forceinline__ void atomic_max_nonneg(float* p, float v) {
  atomicMax(reinterpret_cast<int*>(p), __builtin_bit_cast(int, v));      // valid for v >= 0, *p >= 0
}
__device__ __forceinline__ void atomic_max_any(float* p, float v) {
  if (v >= 0.f) atomicMax(reinterpret_cast<int*>(p), __builtin_bit_cast(int, v));
  else atomicMin(reinterpret_cast<unsigned int*>(p), __builtin_bit_cast(unsigned int, v));
}

struct RangeInfo {
  int start_loc, cache_len, ctx_len, chunk_len, q_start, q_end, cand_end;
  const int32_t* row;
};

__device__ __forceinline__ RangeInfo load_range(const SvkPrefillScoreArgs& a, int i) {
  RangeInfo r;
  const int s = a.batch_indices ? a.batch_indices[i] : i;
  r.start_loc = a.b_start_loc[s];
  r.cache_len = a.b_prompt_cache_len[s];
  r.ctx_len = a.b_seq_len[s];
  r.chunk_len = r.ctx_len - r.cache_len;
  r.q_start = a.score_q_start[i];
  r.q_end = a.score_q_end[i];
  r.cand_end = min(max(a.candidate_start, r.ctx_len - a.num_recent_tokens), a.score_cols);
  r.row = a.req_to_tokens + (int64_t)a.b_req_idx[s] * a.req_stride;
  return r;
}

__device__ __forceinline__ float ps_max16(const f32x16_t& x) {
  return vmax(vmax3(vmax3(x[0], x[1], x[2]), vmax3(x[3], x[4], x[5]), x[15]),
              vmax3(vmax3(x[6], x[7], x[8]), vmax3(x[9], x[10], x[11]), vmax3(x[12], x[13], x[14])));
}

}  // namespace
}  // namespace svk
