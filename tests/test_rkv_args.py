"""CPU: the R-KV entry points reject bad arguments before any launch, with the reference's exception classes."""

import ctypes as C

import pytest


def args(**kw):
    from sparse_vllm_amd import _lib
    base = dict(rows=1, n=8, num_kv_heads=4, head_dim=128, recent_similar_keep=1, max_tokens=4096, similarity_threshold=0.8,
                kv_slot_stride=512, kv_num_slots=64, slot_stride=8, redundancy_stride=8)
    base.update(kw)
    return _lib.SvkRkvRedundancyArgs(**base)


@pytest.mark.parametrize("kw,exc,match", [
    (dict(n=5000), RuntimeError, r"quadratic.*5000.*4096"),
    (dict(head_dim=64), AssertionError, "head_dim 64 unsupported"),
    (dict(num_kv_heads=3), AssertionError, "num_kv_heads 3 unsupported"),
    (dict(recent_similar_keep=-1), ValueError, "recent_similar_keep must be >= 0"),
    (dict(similarity_threshold=1.5), ValueError, r"similarity_threshold must be in \[0, 1\]"),
    (dict(similarity_threshold=-0.1), ValueError, r"similarity_threshold must be in \[0, 1\]"),
    (dict(workspace=1 << 20, workspace_bytes=63), ValueError, "smaller than svk_rkv_redundancy_workspace_bytes = 64"),
])
def test_redundancy_argument_validation_without_gpu(kw, exc, match):
    from sparse_vllm_amd import _lib
    lib = _lib.load()
    assert lib.svk_rkv_redundancy_workspace_bytes(1, 8) == 64
    with pytest.raises(exc, match=match):
        _lib.check(lib.svk_rkv_redundancy(C.byref(args(**kw)), None), lib)


def test_python_wrapper_refuses_a_window_above_the_limit():
    torch = pytest.importorskip("torch")
    from sparse_vllm_amd.kernels import redundancy_scores_from_slots
    k = torch.zeros((16, 4, 128), dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match=r"R-KV redundancy scoring is quadratic.*12.*8"):
        redundancy_scores_from_slots(k, torch.zeros((2, 12), dtype=torch.int32), similarity_threshold=0.8,
                                     recent_similar_keep=1, max_tokens=8)
    assert tuple(redundancy_scores_from_slots(k, torch.zeros((2, 0), dtype=torch.int32), similarity_threshold=0.8,
                                              recent_similar_keep=1, max_tokens=8).shape) == (2, 0)
