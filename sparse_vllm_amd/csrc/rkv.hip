// R-KV redundancy scores and joint retention scores (gfx950).  Replaces the torch form of
// RKVCacheManager.redundancy_scores_from_keys{,_batch} / joint_retention_scores (engine/cache_manager/rkv.py:617-708).
//
// For the last `n` candidate tokens of a row the reference materialises the [n, n] cosine similarity of the keys
// flattened over all KV heads, a triangle mask, a flipped cumulative sum and a second mask.  Here nothing of size n^2
// exists:
//   1. rkv_rinv_kernel      one wave per token: 1 / max(|f_i|, 1e-6) of the flat key, read from the cache by its slot.
//   2. rkv_sim_kernel       workgroup = 128 tokens i of one row, wave = 32 of them.  The wave's own keys stay in
//        registers as the B operand of v_mfma_f32_32x32x16_bf16 (E/16 fragments); the keys j travel in tiles of 32
//        through a double-buffered LDS tile that all four waves share (one LDS-DMA gather per tile, the 16-byte chunks
//        swizzled on the DMA source address so that the A-fragment reads are conflict-free).  The product is formed as
//        S^T = K_j K_i^T: a lane's 16 accumulator registers are 16 keys j of ONE token i, the other 16 keys of the tile
//        sit in lane ^ 32.  The tiles are walked from the newest token to the oldest, so "forgive the `keep` most recent
//        similar future tokens" is a per-lane counter: the rank of a link = counter + number of links of the tile at or
//        after it = one popcount of the tile's 32-bit link mask (own 16 bits | the other half's, one permlane swap).
//        Scale, diagonal, threshold and the forgive rule are applied to the accumulator; the lane adds what remains to
//        its row sum.  avg[i] = (sum + the other half's sum) / n goes to the workspace.
//   3. rkv_joint_kernel     one workgroup per row: softmax over the n averages (held in registers), optional
//        `redundancy` output, and the joint score alpha * importance - (1 - alpha) * redundancy written into the score
//        row that svk_select_prefix_topk_suffix consumes.
// No float atomics; every sum has one fixed order that depends on token indices only (never on slot addresses).

#include "svk_common.hpp"
#include "lds_dma.hpp"

namespace svk {
namespace {

constexpr int kRkvD = 128;        // head_dim
constexpr int kRkvIB = 128;       // tokens i per workgroup (4 waves x 32)
constexpr int kRkvJT = 32;        // keys j per LDS tile
constexpr int kRkvJointThreads = 1024;
constexpr int kRkvJointVec = 4;   // float4 per thread held in registers: rows up to 16384 tokens are read once

__device__ __forceinline__ int64_t rkv_slot(const int32_t* srow, int tok, int64_t num_slots) {
  const int64_t s = srow[tok];
  return s < 0 ? 0 : (s >= num_slots ? num_slots - 1 : s);      // a corrupt table must not leave the pool
}

__device__ __forceinline__ uint32_t lane_xor32_u(uint32_t x) {
  const auto r = __builtin_amdgcn_permlane32_swap(x, x, false, false);
  return (threadIdx.x & 32) ? r[0] : r[1];
}

template <int H>
__global__ void __launch_bounds__(256) rkv_rinv_kernel(const SvkRkvRedundancyArgs a, float* rinv, int npad) {
  constexpr int CH = H * kRkvD / 8;                               // 16-byte chunks of a flat key
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int tok = blockIdx.x * 4 + w, row = blockIdx.y;
  if (tok >= a.n) return;
  const int64_t slot = rkv_slot(a.slots + (int64_t)row * a.slot_stride, tok, a.kv_num_slots);
  const uint4* kp = reinterpret_cast<const uint4*>(a.k_cache + slot * a.kv_slot_stride);
  float ss = 0.f;
  for (int c = lane; c < CH; c += 64) {
    const uint4 v = kp[c];
    const uint32_t wd[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float lo = bf16_lo(wd[u]), hi = bf16_hi(wd[u]);
      ss += lo * lo;
      ss += hi * hi;
    }
  }
  ss = wave_allsum(ss);
  if (lane == 0) rinv[(int64_t)row * npad + tok] = 1.f / fmaxf(sqrtf(ss), 1.0e-6f);
}

template <int H>
__global__ void __launch_bounds__(256) rkv_sim_kernel(const SvkRkvRedundancyArgs a, const float* rinv, float* avg, int npad) {
  constexpr int E = H * kRkvD;                    // flat key length
  constexpr int RB = E * 2;                       // bytes of a flat key = LDS row
  constexpr int KS = E / 16;                      // MFMA k-steps
  constexpr int TILE = kRkvJT * RB;               // bytes of a j tile
  constexpr int NG = TILE / 4096;                 // groups of four DMA instructions per tile (2 H)
  constexpr int GPW = (NG + 3) / 4;               // groups per wave
  constexpr int KB = KS < 8 ? KS : 8;             // A fragments read from LDS in one batch
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];       // 2 tiles | rinv_j [2][32] f32
  float* rbuf = reinterpret_cast<float*>(lds_raw + 2 * TILE);
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lq = lane & 31, half = lane >> 5;
  const int row = blockIdx.y, n = a.n;
  const int iw0 = blockIdx.x * kRkvIB + w * 32, i = iw0 + lq;
  const bool wave_live = iw0 < n, iok = i < n;
  const int32_t* srow = a.slots + (int64_t)row * a.slot_stride;
  const float* rrow = rinv + (int64_t)row * npad;
  const float thr = a.similarity_threshold;
  const int keep = n > 1 ? a.recent_similar_keep : 0;

  // ---- this lane's token i: B fragments (flat key elements ds*16 + half*8 .. +8) and inverse norm
  bf16x8_t kb[KS];
  {
    const uint16_t* kp = a.k_cache + rkv_slot(srow, iok ? i : 0, a.kv_num_slots) * a.kv_slot_stride + half * 8;
#pragma unroll
    for (int ds = 0; ds < KS; ++ds) {
      uint4 t = make_uint4(0, 0, 0, 0);
      if (iok) t = *reinterpret_cast<const uint4*>(kp + ds * 16);
      kb[ds] = __builtin_bit_cast(bf16x8_t, t);
    }
  }
  const float rinv_i = iok ? rrow[i] : 0.f;

  // ---- j tiles -> LDS.  DMA instruction q of a tile fills the LDS bytes [1024 q, 1024 q + 1024): lane -> tile row
  // r = byte / RB, 16-byte position p inside the row; the chunk stored there is c = p ^ (r & 15) (low four bits).
  const uint32_t lds0 = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)lds_raw);
  const char* kbytes = reinterpret_cast<const char*>(a.k_cache);
  const int64_t slot_bytes = a.kv_slot_stride * 2;
  int sl[GPW * 4];                                                // slots of the next tile to fetch, per DMA instruction
  auto load_slots = [&](int j0) __attribute__((always_inline)) {
#pragma unroll
    for (int gi = 0; gi < GPW; ++gi) {
      const int g = w + 4 * gi;
      if (g < NG) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int r = ((g * 4 + j) * 1024 + lane * 16) / RB;
          sl[gi * 4 + j] = (int)rkv_slot(srow, min(j0 + r, n - 1), a.kv_num_slots);
        }
      }
    }
  };
  auto issue = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int gi = 0; gi < GPW; ++gi) {
      const int g = w + 4 * gi;
      if (g < NG) {
        const char* src[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int L = (g * 4 + j) * 1024 + lane * 16;
          const int r = L / RB, p = (L % RB) >> 4;
          const int c = (p & ~15) | ((p ^ r) & 15);
          src[j] = kbytes + ((int64_t)sl[gi * 4 + j] * slot_bytes + c * 16 - 1024 * j);
        }
        pa_dma4x16(src, lds0 + buf * TILE + g * 4096);
      }
    }
  };
  const int T = (n + kRkvJT - 1) / kRkvJT;
  float rnext = 0.f;                                              // threads 0..31: rinv_j of the next tile
  load_slots((T - 1) * kRkvJT);
  issue(0);
  if (tid < kRkvJT) rbuf[tid] = rrow[min((T - 1) * kRkvJT + tid, n - 1)];
  if (T > 1) {
    load_slots((T - 2) * kRkvJT);
    if (tid < kRkvJT) rnext = rrow[(T - 2) * kRkvJT + tid];
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  float rsum = 0.f;
  int cnt = 0;                                                    // similar future tokens of i seen so far (newer tiles)
  for (int k = 0; k < T; ++k) {
    const int j0 = (T - 1 - k) * kRkvJT, buf = k & 1;
    if (k + 1 < T) {
      issue(buf ^ 1);
      if (tid < kRkvJT) rbuf[(buf ^ 1) * kRkvJT + tid] = rnext;
    }
    if (k + 2 < T) {
      load_slots(j0 - 2 * kRkvJT);
      if (tid < kRkvJT) rnext = rrow[j0 - 2 * kRkvJT + tid];
    }
    if (wave_live) {
      // S^T tile: register r of lane (lq, half) = key j0 + (r&3) + 8 (r>>2) + 4 half against token iw0 + lq
      const uint32_t abase = lds0 + buf * TILE + lq * RB;
      f32x16_t s = {};
#pragma unroll
      for (int d0 = 0; d0 < KS; d0 += KB) {
        pa_u32x4_t kf[KB];
#pragma unroll
        for (int u = 0; u < KB; ++u) {
          const int c = (d0 + u) * 2 + half;
          const int p = (c & ~15) | ((c ^ lq) & 15);
          kf[u] = *reinterpret_cast<const __attribute__((address_space(3))) pa_u32x4_t*>(abase + p * 16);
        }
#pragma unroll
        for (int u = 0; u < KB; ++u)
          s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, kf[u]), kb[d0 + u], s, 0, 0, 0);
      }
      const float* rj = rbuf + buf * kRkvJT + 4 * half;
      const bool future = j0 + kRkvJT - 1 > iw0;                  // the tile holds a j > i for some lane of the wave
      const bool plain = j0 + kRkvJT <= n && (j0 > iw0 + 31 || j0 + kRkvJT <= iw0);   // no ragged end, no diagonal
      float v[16];
      uint32_t hm = 0u;                                           // bit jrel: link (i, j0 + jrel) is a similar future token
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 rq = *reinterpret_cast<const float4*>(rj + 8 * q);
        const float rr[4] = {rq.x, rq.y, rq.z, rq.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * q + e, jrel = 8 * q + 4 * half + e, j = j0 + jrel;
          float x = mul_rn(mul_rn(s[r], rinv_i), rr[e]);
          bool live = plain || (j < n && j != i);
          if (thr > 0.f) live = live && x >= thr;
          x = live ? x : 0.f;
          v[r] = x;
          if (future && x > 0.f && j > i) hm |= 1u << jrel;
        }
      }
      if (keep > 0 && future && !__all(cnt >= keep || !iok)) {
        const uint32_t full = hm | lane_xor32_u(hm);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int jrel = (r & 3) + 8 * (r >> 2) + 4 * half;
          const int rank = cnt + __popc(full >> jrel);            // links of i at or after j, newer tiles included
          if (((hm >> jrel) & 1u) && rank <= keep) v[r] = 0.f;
        }
        cnt += __popc(full);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) rsum = add_rn(rsum, v[r]);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  const float other = lane_xor32(rsum);
  if (half == 0 && iok) avg[(int64_t)row * npad + i] = add_rn(rsum, other) / (float)n;
}

// max / sum over the workgroup, the same value (and the same order of operations) in every thread
__device__ __forceinline__ float rkv_block_max(float x, float* red) {
  x = wave_allmax(x);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
  __syncthreads();
  float m = red[0];
  for (int u = 1; u < kRkvJointThreads / 64; ++u) m = fmaxf(m, red[u]);
  return m;
}
__device__ __forceinline__ float rkv_block_sum(float x, float* red) {
  x = wave_allsum(x);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
  __syncthreads();
  float s = red[0];
  for (int u = 1; u < kRkvJointThreads / 64; ++u) s += red[u];
  return s;
}

__global__ void __launch_bounds__(kRkvJointThreads) rkv_joint_kernel(const SvkRkvJointScoreArgs a, float beta) {
  __shared__ float red[kRkvJointThreads / 64];
  const int row = blockIdx.x, tid = threadIdx.x, n = a.window;
  const float* av = a.avg + (int64_t)row * a.avg_stride;
  const bool vec = (reinterpret_cast<uintptr_t>(av) & 15) == 0;
  constexpr int kHeld = kRkvJointVec * kRkvJointThreads * 4;
  float x[kRkvJointVec][4];
  float m = -INFINITY;
#pragma unroll
  for (int u = 0; u < kRkvJointVec; ++u) {
    const int e0 = (u * kRkvJointThreads + tid) * 4;
    if (vec && e0 + 3 < n) {
      const float4 t = *reinterpret_cast<const float4*>(av + e0);
      x[u][0] = t.x; x[u][1] = t.y; x[u][2] = t.z; x[u][3] = t.w;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) x[u][e] = e0 + e < n ? av[e0 + e] : -INFINITY;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) m = fmaxf(m, x[u][e]);
  }
  for (int e = kHeld + tid; e < n; e += kRkvJointThreads) m = fmaxf(m, av[e]);
  m = rkv_block_max(m, red);
  float sum = 0.f;
#pragma unroll
  for (int u = 0; u < kRkvJointVec; ++u)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      x[u][e] = expf(x[u][e] - m);                               // padding: exp(-inf) = 0
      sum += x[u][e];
    }
  for (int e = kHeld + tid; e < n; e += kRkvJointThreads) sum += expf(av[e] - m);
  sum = rkv_block_sum(sum, red);

  const int first = a.n_candidates - n;                           // candidates before the window keep their importance
  const float* imp = a.importance ? a.importance + (int64_t)row * a.importance_stride + a.candidate_start : nullptr;
  float* sc = a.scores ? a.scores + (int64_t)row * a.score_stride + a.candidate_start : nullptr;
  float* rd = a.redundancy ? a.redundancy + (int64_t)row * a.redundancy_stride : nullptr;
  auto publish = [&](int e, float p) __attribute__((always_inline)) {
    const float r = p / sum;
    if (rd) rd[e] = r;
    if (sc) sc[first + e] = add_rn(mul_rn(a.alpha, imp[first + e]), -mul_rn(beta, r));
  };
#pragma unroll
  for (int u = 0; u < kRkvJointVec; ++u)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int idx = (u * kRkvJointThreads + tid) * 4 + e;
      if (idx < n) publish(idx, x[u][e]);
    }
  for (int e = kHeld + tid; e < n; e += kRkvJointThreads) publish(e, expf(av[e] - m));
  if (sc)
    for (int c = tid; c < first; c += kRkvJointThreads) sc[c] = imp[c];
}

inline int rkv_npad(int n) { return (n + 3) & ~3; }

template <int H>
int rkv_launch(const SvkRkvRedundancyArgs& a, hipStream_t s) {
  constexpr int shm = 2 * kRkvJT * H * kRkvD * 2 + 2 * kRkvJT * (int)sizeof(float);
  static const bool attr_ok = hipFuncSetAttribute(reinterpret_cast<const void*>(&rkv_sim_kernel<H>),
                                                  hipFuncAttributeMaxDynamicSharedMemorySize, shm) == hipSuccess;
  (void)attr_ok;
  const int npad = rkv_npad(a.n);
  float* avg = a.workspace;
  float* rinv = a.workspace + (int64_t)a.rows * npad;
  hipLaunchKernelGGL((rkv_rinv_kernel<H>), dim3((a.n + 3) / 4, a.rows), dim3(256), 0, s, a, rinv, npad);
  hipLaunchKernelGGL((rkv_sim_kernel<H>), dim3((a.n + kRkvIB - 1) / kRkvIB, a.rows), dim3(256), (size_t)shm, s, a, rinv, avg, npad);
  if (a.redundancy != nullptr) {
    SvkRkvJointScoreArgs j = {};
    j.avg = avg;
    j.redundancy = a.redundancy;
    j.avg_stride = npad;
    j.redundancy_stride = a.redundancy_stride;
    j.rows = a.rows;
    j.window = a.n;
    j.n_candidates = a.n;
    hipLaunchKernelGGL(rkv_joint_kernel, dim3(a.rows), dim3(kRkvJointThreads), 0, s, j, 0.f);
  }
  return check_launch("svk_rkv_redundancy");
}

}  // namespace
}  // namespace svk

extern "C" int64_t svk_rkv_redundancy_workspace_bytes(int32_t rows, int32_t n) {
  if (rows <= 0 || n <= 0) return 0;
  return (int64_t)sizeof(float) * 2 * rows * svk::rkv_npad(n);
}

extern "C" int64_t svk_rkv_redundancy_avg_stride(int32_t n) { return n > 0 ? svk::rkv_npad(n) : 0; }

extern "C" int svk_rkv_redundancy(const SvkRkvRedundancyArgs* a, svk_stream_t stream) {
  using namespace svk;
  SVK_REQUIRE(a != nullptr, SVK_ERR_VALUE, "svk_rkv_redundancy: null args");
  SVK_REQUIRE(a->head_dim == kRkvD, SVK_ERR_LAYOUT, "svk_rkv_redundancy: head_dim %d unsupported (128)", a->head_dim);
  SVK_REQUIRE(a->num_kv_heads == 1 || a->num_kv_heads == 2 || a->num_kv_heads == 4 || a->num_kv_heads == 8, SVK_ERR_LAYOUT,
              "svk_rkv_redundancy: num_kv_heads %d unsupported (1, 2, 4, 8)", a->num_kv_heads);
  SVK_REQUIRE(a->recent_similar_keep >= 0, SVK_ERR_VALUE, "R-KV recent_similar_keep must be >= 0, got %d.", a->recent_similar_keep);
  SVK_REQUIRE(a->similarity_threshold >= 0.f && a->similarity_threshold <= 1.f, SVK_ERR_VALUE,
              "R-KV similarity_threshold must be in [0, 1], got %g.", (double)a->similarity_threshold);
  SVK_REQUIRE(a->n <= a->max_tokens, SVK_ERR_STATE,
              "R-KV redundancy scoring is quadratic in candidate tokens: candidate_tokens=%d exceeds max_tokens=%d.", a->n,
              a->max_tokens);
  SVK_REQUIRE(a->rows <= 65535, SVK_ERR_VALUE, "svk_rkv_redundancy: rows %d exceeds 65535 per launch", a->rows);
  if (a->rows <= 0 || a->n <= 0) return SVK_OK;
  const int64_t need = svk_rkv_redundancy_workspace_bytes(a->rows, a->n);
  SVK_REQUIRE(a->workspace != nullptr && a->workspace_bytes >= need, SVK_ERR_VALUE,
              "svk_rkv_redundancy: workspace of %lld bytes is smaller than svk_rkv_redundancy_workspace_bytes = %lld",
              (long long)(a->workspace ? a->workspace_bytes : 0), (long long)need);
  const int E = a->num_kv_heads * kRkvD;
  SVK_REQUIRE(a->kv_slot_stride >= E && a->kv_slot_stride % 8 == 0, SVK_ERR_LAYOUT,
              "svk_rkv_redundancy: kv_slot_stride %lld must be a multiple of 8 and >= Hkv*D = %d (heads contiguous in a slot)",
              (long long)a->kv_slot_stride, E);
  SVK_REQUIRE(a->slot_stride >= a->n && a->redundancy_stride >= (a->redundancy ? a->n : 0), SVK_ERR_VALUE,
              "svk_rkv_redundancy: row strides (slots %lld, redundancy %lld) shorter than n = %d", (long long)a->slot_stride,
              (long long)a->redundancy_stride, a->n);
  SVK_REQUIRE(a->k_cache != nullptr && a->slots != nullptr && a->kv_num_slots > 0, SVK_ERR_VALUE,
              "svk_rkv_redundancy: k_cache / slots missing or empty pool");
  SVK_REQUIRE((reinterpret_cast<uintptr_t>(a->k_cache) & 15) == 0 && (reinterpret_cast<uintptr_t>(a->workspace) & 15) == 0,
              SVK_ERR_LAYOUT, "svk_rkv_redundancy: k_cache and workspace must be 16-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (a->num_kv_heads) {
    case 1: return rkv_launch<1>(*a, s);
    case 2: return rkv_launch<2>(*a, s);
    case 4: return rkv_launch<4>(*a, s);
    default: return rkv_launch<8>(*a, s);
  }
}

extern "C" int svk_rkv_joint_scores(const SvkRkvJointScoreArgs* a, svk_stream_t stream) {
  using namespace svk;
  SVK_REQUIRE(a != nullptr, SVK_ERR_VALUE, "svk_rkv_joint_scores: null args");
  SVK_REQUIRE(a->alpha >= 0.f && a->alpha <= 1.f, SVK_ERR_VALUE, "R-KV alpha must be in [0, 1], got %g.", (double)a->alpha);
  SVK_REQUIRE(a->window >= 0 && a->window <= a->n_candidates && a->candidate_start >= 0, SVK_ERR_VALUE,
              "svk_rkv_joint_scores: window %d must lie inside the %d candidates (candidate_start %d)", a->window,
              a->n_candidates, a->candidate_start);
  if (a->rows <= 0 || a->n_candidates <= 0) return SVK_OK;
  SVK_REQUIRE((a->window == 0 || (a->avg != nullptr && a->avg_stride >= a->window)) &&
                  (a->scores == nullptr || a->importance != nullptr) && (a->scores != nullptr || a->redundancy != nullptr),
              SVK_ERR_VALUE, "svk_rkv_joint_scores: avg (stride >= window), importance with scores, and one output are required");
  SVK_REQUIRE((a->scores == nullptr || (a->score_stride >= a->candidate_start + a->n_candidates &&
                                        a->importance_stride >= a->candidate_start + a->n_candidates)) &&
                  (a->redundancy == nullptr || a->redundancy_stride >= a->window),
              SVK_ERR_VALUE, "svk_rkv_joint_scores: a row stride is shorter than the columns written");
  hipLaunchKernelGGL(rkv_joint_kernel, dim3(a->rows), dim3(kRkvJointThreads), 0, static_cast<hipStream_t>(stream), *a,
                     (float)(1.0 - (double)a->alpha));
  return check_launch("svk_rkv_joint_scores");
}
