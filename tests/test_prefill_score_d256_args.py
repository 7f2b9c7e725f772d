"""CPU, no launch: svk_prefill_score and the statistics of svk_context_attention_fwd take head_dim 256 and keep their
argument checks there."""

import ctypes as C

import pytest

P = 1 << 20           # a well-aligned stand-in for a device pointer: validation never dereferences it


def score(**kw):
    from sparse_vllm_amd import _lib
    base = dict(q=P, k_cache=P, attn_score=P, b_req_idx=P, b_start_loc=P, b_seq_len=P, b_prompt_cache_len=P, req_to_tokens=P,
                score_q_start=P, score_q_end=P, q_stride_t=8 * 256, q_stride_h=256, kv_slot_stride=4 * 256, kv_head_stride=256,
                req_stride=64, score_stride=64, n_ranges=0, num_q_heads=8, num_kv_heads=4, head_dim=256, max_query_len=16,
                score_cols=64, score_mode=_lib.SVK_PREFILL_SCORE_PROBABILITY)
    lib = _lib.load()
    return _lib.check(lib.svk_prefill_score(C.byref(_lib.SvkPrefillScoreArgs(**{**base, **kw})), None), lib)


def test_prefill_score_head_dim_validation():
    score()                                                       # head_dim 256, no ranges: SVK_OK
    with pytest.raises(AssertionError, match=r"head_dim 192 unsupported \(64, 128, 256\)"):
        score(head_dim=192)
    with pytest.raises(ValueError, match="candidate_start = 0"):
        score(n_ranges=1, row_stats=P, candidate_start=4)


def test_context_attention_statistics_need_a_window_start_at_256():
    from sparse_vllm_amd import _lib
    a = _lib.SvkContextAttentionArgs(q=P, k_cache=P, v_cache=P, o=P, b_req_idx=P, b_start_loc=P, b_seq_len=P,
                                     b_prompt_cache_len=P, req_to_tokens=P, q_stride_t=8 * 256, q_stride_h=256,
                                     kv_slot_stride=4 * 256, kv_head_stride=256, o_stride_t=8 * 256, o_stride_h=256,
                                     req_stride=64, batch=1, num_q_heads=8, num_kv_heads=4, head_dim=256, max_input_len=16,
                                     kv_num_slots=64, score_row_stats=P, score_wpad=32)
    lib = _lib.load()
    with pytest.raises(ValueError, match="score_row_stats needs score_q_start"):
        _lib.check(lib.svk_context_attention_fwd(C.byref(a), None), lib)
