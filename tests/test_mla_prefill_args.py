"""CPU: the MLA prefill entry points and the head_dim 256 attention dispatch reject bad arguments before any launch."""

import ctypes as C

import pytest

P = 1 << 20           # a well-aligned stand-in for a device pointer: validation never dereferences it


def gather(**kw):
    from sparse_vllm_amd import _lib
    base = dict(latent_cache=P, rope_cache=P, active_slots=P, request_indices=P, context_lens=P, packed_start_locs=P,
                gathered_latent=P, gathered_rope=P, latent_slot_stride=576, rope_slot_stride=576, num_slots=64,
                slots_stride=128, out_latent_stride=512, out_rope_stride=64, out_capacity=256, batch=0, slot_rows=4,
                max_context_len=128, latent_dim=512, rope_dim=64)
    return _lib.SvkMlaGatherLatentArgs(**{**base, **kw})


def attention(**kw):
    from sparse_vllm_amd import _lib
    base = dict(q=P, k_cache=P, v_cache=P, o=P, b_req_idx=P, b_start_loc=P, b_seq_len=P, b_prompt_cache_len=P,
                req_to_tokens=P, q_stride_t=8 * 256, q_stride_h=256, kv_slot_stride=4 * 256, kv_head_stride=256,
                o_stride_t=8 * 256, o_stride_h=256, req_stride=64, batch=0, num_q_heads=8, num_kv_heads=4, head_dim=256,
                max_input_len=16, kv_num_slots=32)
    return _lib.SvkContextAttentionArgs(**{**base, **kw})


@pytest.mark.parametrize("kw,exc,match", [
    (dict(latent_cache=None), ValueError, "null tensor pointer"),
    (dict(latent_dim=576), AssertionError, "latent_dim 576 / rope_dim 64 unsupported"),
    (dict(latent_slot_stride=580), AssertionError, "16-byte alignment"),
    (dict(out_rope_stride=68), AssertionError, "16-byte alignment"),
    (dict(gathered_latent=P + 8), AssertionError, "16-byte alignment"),
    (dict(out_capacity=-1), ValueError, r"negative capacity \(-1\)"),
    (dict(max_context_len=-3), ValueError, r"max_context_len \(-3\)"),
    (dict(slots_stride=64), ValueError, "slots_stride 64 below max_context_len"),
])
def test_gather_argument_validation_without_gpu(kw, exc, match):
    from sparse_vllm_amd import _lib
    lib = _lib.load()
    with pytest.raises(exc, match=match):
        _lib.check(lib.svk_mla_gather_latent(C.byref(gather(**kw)), None), lib)


def test_head_dim_256_dispatch_validation():
    from sparse_vllm_amd import _lib
    lib = _lib.load()
    assert lib.svk_mla_gather_latent(C.byref(gather(latent_slot_stride=512, rope_slot_stride=64)), None) == _lib.SVK_OK
    for hq, hkv in ((20, 20), (8, 4), (8, 2)):
        assert lib.svk_context_attention_fwd(C.byref(attention(num_q_heads=hq, num_kv_heads=hkv)), None) == _lib.SVK_OK
    with pytest.raises(AssertionError, match=r"head_dim 256 supports GQA group sizes 1, 2, 4, got 8"):
        _lib.check(lib.svk_context_attention_fwd(C.byref(attention(num_q_heads=8, num_kv_heads=1)), None), lib)


@pytest.mark.parametrize("kw", [dict(qk_nope_head_dim=128), dict(value_head_dim=128)])
def test_run_mla_prefill_raises_for_unequal_widths(kw):
    torch = pytest.importorskip("torch")
    from sparse_vllm_amd.kernels import run_mla_prefill
    z, q = torch.zeros(1, dtype=torch.int32), torch.zeros((1, 2, 256), dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="requires equal Q/K/V head widths of 256"):
        run_mla_prefill(q, None, None, None, z, z, z, z, None, q, **kw)
