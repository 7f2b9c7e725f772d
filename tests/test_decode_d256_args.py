"""CPU, no launch: the decode entry point takes head_dim 256 and refuses what the 256 kernel does not carry; the MI355X
launch provider offers itself for 256-wide models and counts two waves per KV head."""

import ctypes as C

import pytest

P = 1 << 20           # a well-aligned stand-in for a device pointer: validation never dereferences it


def call(**kw):
    from sparse_vllm_amd import _lib
    base = dict(q=P, k_cache=P, v_cache=P, req_to_tokens=P, b_req_idx=P, b_seqlen=P, mid_o=P, mid_lse=P, q_stride_b=8 * 256,
                q_stride_h=256, kv_slot_stride=4 * 256, kv_head_stride=256, kv_num_slots=64, req_stride=64,
                mid_o_stride_b=8 * 256, mid_o_stride_h=256, mid_o_stride_s=256, mid_lse_stride_b=8, mid_lse_stride_h=1,
                batch=0, num_q_heads=8, num_kv_heads=4, head_dim=256, max_len_in_batch=16, block_seq=32)
    lib = _lib.load()
    return _lib.check(lib.svk_flash_decode_stage1(C.byref(_lib.SvkFlashDecodeStage1Args(**{**base, **kw})), None), lib)


def test_stage1_head_dim_validation():
    call()                                                        # head_dim 256, batch 0: SVK_OK
    with pytest.raises(AssertionError, match=r"head_dim 192 unsupported \(64, 128, 256\)"):
        call(head_dim=192)
    with pytest.raises(AssertionError, match="rotated store is head_dim 64 / 128 only"):
        call(new_cos_sin=P)


def test_launch_provider_takes_head_dim_256():
    torch = pytest.importorskip("torch")
    from sparse_vllm_amd.operators.decode_attention import (DecodeAttentionLaunchSpec, Mi355xDecodeLaunchProvider,
                                                            PreparedDecodeAttentionLaunchOp)
    from sparse_vllm_amd.platforms.interface import DeviceCaps, PlatformEnum
    caps = DeviceCaps(PlatformEnum.ROCM, "cuda", 0, "AMD Instinct MI355X", compute_capability=(9, 5), arch="gfx950")
    spec = DecodeAttentionLaunchSpec(16, 2, 256, torch.bfloat16)
    assert Mi355xDecodeLaunchProvider.supports(spec, caps).supported
    assert not Mi355xDecodeLaunchProvider.supports(DecodeAttentionLaunchSpec(16, 2, 256, torch.float16), caps).supported
    # one wave per SIMD needs 256 workgroups at 2 KV heads x 2 waves, where head_dim 128 (no keyword) needs 512
    cfg = dict(block_seq=256, max_context_len=32768, requires_attention_scores=False, batch_size=1)
    assert PreparedDecodeAttentionLaunchOp(spec, Mi355xDecodeLaunchProvider()).launch_config(**cfg)[0] == 128
    assert Mi355xDecodeLaunchProvider().launch_config(**cfg, num_kv_heads=2)[0] == 64
