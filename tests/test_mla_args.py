"""CPU: the MLA decode entry points reject bad arguments before any launch, with the reference's exception classes."""

import ctypes as C

import pytest

P = 1 << 20           # a well-aligned stand-in for a device pointer: validation never dereferences it


def stage1(**kw):
    from sparse_vllm_amd import _lib
    base = dict(q_latent=P, q_rope=P, latent_cache=P, rope_cache=P, active_slots=P, request_indices=P, context_lens=P,
                mid_o=P, mid_lse=P, q_latent_stride_b=512, q_latent_stride_h=512, q_rope_stride_b=64, q_rope_stride_h=64,
                latent_slot_stride=576, rope_slot_stride=576, num_slots=64, slots_stride=128, mid_o_stride_b=2048,
                mid_o_stride_h=2048, mid_o_stride_s=512, mid_lse_stride_b=4, mid_lse_stride_h=4, batch=0, num_heads=16,
                latent_dim=512, rope_dim=64, max_context_len=128, block_seq=32, score_mode=_lib.SVK_SCORE_NONE,
                slot_rows=4, softmax_scale=0.125)
    base.update(kw)
    return _lib.SvkMlaDecodeStage1Args(**base)


@pytest.mark.parametrize("kw,exc,match", [
    (dict(q_latent=None), ValueError, "null tensor pointer"),
    (dict(mid_lse=None), ValueError, "null tensor pointer"),
    (dict(latent_dim=576), AssertionError, "latent_dim 576 / rope_dim 64 unsupported"),
    (dict(rope_dim=128), AssertionError, "rope_dim 128 unsupported"),
    (dict(num_heads=0), AssertionError, "num_heads 0 unsupported"),
    (dict(num_heads=129), AssertionError, "num_heads 129 unsupported"),
    (dict(block_seq=0), AssertionError, "block_seq 0 must be a positive multiple of 32"),
    (dict(block_seq=48), AssertionError, "block_seq 48 must be a positive multiple of 32"),
    (dict(score_mode=1), ValueError, "score_mode 1 unknown"),
    (dict(score_mode=2), ValueError, "score_mode 2 needs attn_score"),
    (dict(score_mode=3), ValueError, "score_mode 3 needs attn_score"),
    (dict(latent_slot_stride=580), AssertionError, "16-byte alignment"),
    (dict(rope_slot_stride=68), AssertionError, "16-byte alignment"),
    (dict(rope_cache=P + 8), AssertionError, "16-byte alignment"),
    (dict(softmax_scale=0.0), ValueError, "softmax_scale must be finite and positive"),
    (dict(softmax_scale=float("inf")), ValueError, "softmax_scale must be finite and positive"),
    (dict(softmax_scale=float("nan")), ValueError, "softmax_scale must be finite and positive"),
    (dict(batch=1, max_context_len=-5), ValueError, "max_context_len -5 must be positive"),
    (dict(mid_lse_stride_h=0), ValueError, "strides must be positive"),
    (dict(score_mode=3, attn_score=P, score_stride_b=2048, score_stride_h=0), ValueError, "score strides"),
])
def test_stage1_argument_validation_without_gpu(kw, exc, match):
    from sparse_vllm_amd import _lib
    lib = _lib.load()
    with pytest.raises(exc, match=match):
        _lib.check(lib.svk_mla_decode_stage1(C.byref(stage1(**kw)), None), lib)


def test_well_formed_blocks_pass_validation_up_to_the_launch():
    """batch / n_tokens = 0: everything is validated, nothing is launched"""
    from sparse_vllm_amd import _lib
    lib = _lib.load()
    for mode in (_lib.SVK_SCORE_NONE, _lib.SVK_SCORE_HEADMAX, _lib.SVK_SCORE_PERHEAD):
        a = stage1(score_mode=mode, attn_score=P, latent_slot_stride=512, rope_slot_stride=64, score_stride_b=2048,
                   score_stride_h=128)
        assert lib.svk_mla_decode_stage1(C.byref(a), None) == _lib.SVK_OK
    s2 = _lib.SvkMlaDecodeStage2Args(mid_o=P, mid_lse=P, context_lens=P, output=P, mid_o_stride_b=2048, mid_o_stride_h=2048,
                                     mid_o_stride_s=512, mid_lse_stride_b=4, mid_lse_stride_h=4, o_stride_b=8192,
                                     o_stride_h=512, batch=0, num_heads=16, latent_dim=512, block_seq=32, max_context_len=128)
    assert lib.svk_mla_decode_stage2(C.byref(s2), None) == _lib.SVK_OK
    s2.latent_dim = 256
    with pytest.raises(AssertionError, match="latent_dim 256 unsupported"):
        _lib.check(lib.svk_mla_decode_stage2(C.byref(s2), None), lib)
    st = _lib.SvkMlaStoreLatentArgs(latent=P, rope=P, latent_cache=P, rope_cache=P, slot_mapping=P, latent_stride=512,
                                    rope_stride=64, latent_slot_stride=576, rope_slot_stride=576, num_slots=8, n_tokens=0,
                                    latent_dim=512, rope_dim=64)
    assert lib.svk_mla_store_latent(C.byref(st), None) == _lib.SVK_OK
    st.rope_stride = 60
    with pytest.raises(AssertionError, match="16-byte alignment"):
        _lib.check(lib.svk_mla_store_latent(C.byref(st), None), lib)


def test_python_wrapper_raises_the_reference_exception_classes():
    torch = pytest.importorskip("torch")
    from sparse_vllm_amd.kernels import mla
    q, qr = torch.zeros((2, 16, 512), dtype=torch.bfloat16), torch.zeros((2, 16, 64), dtype=torch.bfloat16)
    lat, rope = torch.zeros((8, 1, 512), dtype=torch.bfloat16), torch.zeros((8, 1, 64), dtype=torch.bfloat16)
    slots, idx = torch.zeros((2, 64), dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    ws = mla.allocate_mla_decode_workspace(2, 16, 64, "cpu")
    assert ws.block_seq == 32 and tuple(ws.mid_output.shape) == (2, 16, 2, 512)
    assert mla.choose_block_seq(64, 128, 131072) == 131072 and mla.choose_block_seq(1, 16, 131072) == 512
    assert mla.choose_block_seq(8, 128, 4096) == 512 and mla.choose_block_seq(8, 128, 4096, headmax_scores=True) == 128
    out = torch.zeros_like(q)
    call = lambda **kw: mla.run_mla_decode(q, qr, lat, rope, slots, idx, idx, out, ws, **kw)   # noqa: E731
    with pytest.raises(ValueError, match="softmax_scale must be finite and positive"):
        call(softmax_scale=-1.0)
    with pytest.raises(TypeError, match="torch.float32 only"):
        call(softmax_scale=0.1, attn_score=torch.zeros((2, 16, 64), dtype=torch.bfloat16))
    with pytest.raises(ValueError, match=r"must cover \[batch, context\]"):
        call(softmax_scale=0.1, attn_score=torch.zeros((2, 32), dtype=torch.float32))
    with pytest.raises(TypeError, match="output must use torch.bfloat16"):
        mla.run_mla_decode(q, qr, lat, rope, slots, idx, idx, out.float(), ws, softmax_scale=0.1)
