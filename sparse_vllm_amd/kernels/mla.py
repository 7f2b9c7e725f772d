"""MLA (multi-head latent attention) over the latent cache on device (libsvk.so): split-KV decode stage 1 with fused
token scores, the LSE merge, the latent store, and the prefill path (ragged gather of the visible rows, the caller's
kv_b_proj, causal attention over the expanded head_dim 256 keys / values).  Names and argument order follow the
reference's kernels/triton/mla/{decode_stage1,decode_stage2,copy_latent,decode_schedule,gather_latent}.py and
layers/mla_attention.py; see include/svk.h (SvkMla*Args).

The cache is either the reference's two tensors (`[slots, 1, 512]`, `[slots, 1, 64]`) or two views of one interleaved
`[slots, 576]` allocation (`buf[:, :512]`, `buf[:, 512:]`, any shape whose last dim is the row and whose first stride is
the slot stride).  `block_seq` is a host integer fixed when the workspace is allocated; nothing here allocates or
synchronises after that, so every call can be captured in a graph."""

from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import torch

from .. import _lib

MLA_LATENT_DIM = 512
MLA_ROPE_DIM = 64
MLA_TOKEN_TILE = 32
_TARGET_WORKGROUPS = 256          # one workgroup per CU of an MI355X


@dataclass
class MlaDecodeWorkspace:
    """Split-KV partials with graph-stable addresses: mid_output f32 [B, H, nblk, 512], mid_logsumexp f32 [B, H, nblk]."""
    mid_output: torch.Tensor
    mid_logsumexp: torch.Tensor
    block_seq: int
    max_context_len: int


def choose_block_seq(batch: int, heads: int, max_context_len: int, *, headmax_scores: bool = False) -> int:
    """Smallest multiple of the token tile for which lanes x blocks x head tiles still covers the CUs (fewer, longer
    blocks once the batch alone fills the machine).  A launch with 2-D head-maximum scores keeps all head tiles of a
    block in one workgroup, so there the head tiles do not count."""
    head_tiles = 1 if headmax_scores else (int(heads) + 31) // 32
    blocks = max(1, -(-_TARGET_WORKGROUPS // max(1, int(batch) * head_tiles)))
    per_block = -(-max(1, int(max_context_len)) // blocks)
    return max(MLA_TOKEN_TILE, -(-per_block // MLA_TOKEN_TILE) * MLA_TOKEN_TILE)


def allocate_mla_decode_workspace(batch: int, heads: int, max_context_len: int, device, *,
                                  block_seq: int | None = None, headmax_scores: bool = False) -> MlaDecodeWorkspace:
    """`headmax_scores`: the workspace serves calls with a 2-D `attn_score` (see choose_block_seq)."""
    if batch <= 0 or not 1 <= heads <= 128 or max_context_len <= 0:
        raise ValueError(f"MLA decode workspace needs batch > 0, 1 <= heads <= 128, max_context_len > 0; got "
                         f"{batch}, {heads}, {max_context_len}")
    block_seq = choose_block_seq(batch, heads, max_context_len, headmax_scores=headmax_scores) if block_seq is None else int(block_seq)
    if block_seq <= 0 or block_seq % MLA_TOKEN_TILE:
        raise ValueError(f"block_seq must be a positive multiple of {MLA_TOKEN_TILE}, got {block_seq}")
    nblk = -(-int(max_context_len) // block_seq)
    return MlaDecodeWorkspace(
        mid_output=torch.empty((batch, heads, nblk, MLA_LATENT_DIM), dtype=torch.float32, device=device),
        mid_logsumexp=torch.empty((batch, heads, nblk), dtype=torch.float32, device=device),
        block_seq=block_seq, max_context_len=int(max_context_len))


def _check_dtypes(expected: torch.dtype, **tensors) -> None:
    """TypeError naming the first tensor whose dtype is not `expected`."""
    for name, t in tensors.items():
        if t.dtype is not expected:
            raise TypeError(f"{name} must use {expected}, got {t.dtype}")


def _cache_rows(name: str, cache: torch.Tensor, width: int) -> int:
    """Slot stride (elements) of a cache tensor `[slots, ..., width]` whose middle dims are 1."""
    if cache.ndim < 2 or cache.shape[-1] != width or cache.stride(-1) != 1 or cache.numel() != cache.shape[0] * width:
        raise ValueError(f"{name} must have shape [slots, 1, {width}] (or [slots, {width}]), got {tuple(cache.shape)}")
    return int(cache.stride(0))


def _score_mode(attn_score, batch: int, heads: int, width: int) -> int:
    """SVK_SCORE_* of a score buffer: None, f32 [>= B, >= W] (head maximum) or f32 [>= B, >= H, >= W] (per head)."""
    if attn_score is None:
        return _lib.SVK_SCORE_NONE
    rank = attn_score.dim()
    if rank not in (2, 3):
        raise ValueError(f"MLA attention score must be [batch, context] or [batch, heads, context], got "
                         f"{tuple(attn_score.shape)}.")
    kind, need = ("Head-reduced", (batch, width)) if rank == 2 else ("Per-head", (batch, heads, width))
    if attn_score.dtype is not torch.float32:
        only = "" if rank == 2 else " only in this build (no bf16 / fp16 score buffers)"
        raise TypeError(f"{kind} MLA attention scores must use torch.float32{only}, got {attn_score.dtype}.")
    if any(have < want for have, want in zip(attn_score.shape, need)):
        names = "[batch, context]" if rank == 2 else "[batch, heads, context]"
        raise ValueError(f"{kind} MLA attention scores must cover {names}={list(need)}, got {tuple(attn_score.shape)}.")
    if attn_score.stride(-1) != 1:
        raise ValueError("MLA attention scores must be contiguous along the context")
    return _lib.SVK_SCORE_HEADMAX if rank == 2 else _lib.SVK_SCORE_PERHEAD


@torch.no_grad()
def decode_stage1(q_latent, q_rope, latent_cache, rope_cache, active_slots, request_indices, context_lens,
                  block_seq: int, mid_output, mid_logsumexp, *, attn_score=None, max_context_len: int | None = None,
                  softmax_scale: float) -> None:
    """Independently normalised attention blocks (decode_stage1.py:277): mid_output [B, H, nblk, 512],
    mid_logsumexp [B, H, nblk], optional raw scores ([B, W] head maximum or [B, H, W] per head, f32).  Score positions
    at or beyond a lane's length, and positions whose slot lies outside the pool, are left untouched."""
    _check_dtypes(torch.bfloat16, q_latent=q_latent, q_rope=q_rope, latent_cache=latent_cache, rope_cache=rope_cache)
    _check_dtypes(torch.int32, active_slots=active_slots, request_indices=request_indices, context_lens=context_lens)
    _check_dtypes(torch.float32, mid_output=mid_output, mid_logsumexp=mid_logsumexp)
    if q_latent.ndim != 3 or q_latent.shape[-1] != MLA_LATENT_DIM:
        raise ValueError(f"q_latent must have shape [batch, heads, 512], got {tuple(q_latent.shape)}")
    if tuple(q_rope.shape) != (*q_latent.shape[:-1], MLA_ROPE_DIM):
        raise ValueError(f"q_rope must have shape [batch, heads, 64], got {tuple(q_rope.shape)}")
    lat_stride = _cache_rows("latent_cache", latent_cache, MLA_LATENT_DIM)
    rope_stride = _cache_rows("rope_cache", rope_cache, MLA_ROPE_DIM)
    if latent_cache.shape[0] != rope_cache.shape[0]:
        raise ValueError("latent_cache and rope_cache must have equal slots")
    if active_slots.ndim != 2 or active_slots.stride(1) != 1:
        raise ValueError("active_slots must have shape [rows, max_context_len]")
    batch, heads = int(q_latent.shape[0]), int(q_latent.shape[1])
    if tuple(request_indices.shape) != (batch,):
        raise ValueError(f"request_indices must have shape ({batch},), got {tuple(request_indices.shape)}")
    if tuple(context_lens.shape) != (batch,):
        raise ValueError(f"context_lens must have shape ({batch},), got {tuple(context_lens.shape)}")
    width = int(active_slots.shape[1]) if max_context_len is None else int(max_context_len)
    if not 0 < width <= int(active_slots.shape[1]):
        raise ValueError(f"MLA decode max_context_len must be within the active-slot width: max_context_len={width} "
                         f"active_slot_width={int(active_slots.shape[1])}.")
    nblk = -(-width // int(block_seq)) if block_seq > 0 else 0
    if mid_output.ndim != 4 or mid_output.shape[3] != MLA_LATENT_DIM or mid_output.stride(3) != 1:
        raise ValueError("mid_output must have shape [batch, heads, blocks, 512]")
    if tuple(mid_logsumexp.shape) != tuple(mid_output.shape[:3]) or mid_logsumexp.stride(2) != 1:
        raise ValueError("mid_logsumexp must match the first three mid_output dimensions")
    if mid_output.shape[0] < batch or mid_output.shape[1] < heads or mid_output.shape[2] < nblk:
        raise ValueError(f"mid_output has capacity {tuple(mid_output.shape[:3])}, but [batch, heads, blocks]="
                         f"[{batch}, {heads}, {nblk}] are required")
    mode = _score_mode(attn_score, batch, heads, width)
    if q_latent.stride(2) != 1 or q_rope.stride(2) != 1:
        raise ValueError("q_latent and q_rope must be contiguous along the last dimension")
    lib = _lib.load()
    a = _lib.SvkMlaDecodeStage1Args(
        q_latent=_lib.ptr(q_latent), q_rope=_lib.ptr(q_rope), latent_cache=_lib.ptr(latent_cache),
        rope_cache=_lib.ptr(rope_cache), active_slots=_lib.ptr(active_slots), request_indices=_lib.ptr(request_indices),
        context_lens=_lib.ptr(context_lens), mid_o=_lib.ptr(mid_output), mid_lse=_lib.ptr(mid_logsumexp),
        attn_score=_lib.ptr(attn_score),
        q_latent_stride_b=q_latent.stride(0), q_latent_stride_h=q_latent.stride(1), q_rope_stride_b=q_rope.stride(0),
        q_rope_stride_h=q_rope.stride(1), latent_slot_stride=lat_stride, rope_slot_stride=rope_stride,
        num_slots=latent_cache.shape[0], slots_stride=active_slots.stride(0),
        mid_o_stride_b=mid_output.stride(0), mid_o_stride_h=mid_output.stride(1), mid_o_stride_s=mid_output.stride(2),
        mid_lse_stride_b=mid_logsumexp.stride(0), mid_lse_stride_h=mid_logsumexp.stride(1),
        score_stride_b=0 if attn_score is None else attn_score.stride(0),
        score_stride_h=attn_score.stride(1) if mode == _lib.SVK_SCORE_PERHEAD else 0,
        batch=batch, num_heads=heads, latent_dim=MLA_LATENT_DIM, rope_dim=MLA_ROPE_DIM, max_context_len=width,
        block_seq=int(block_seq), score_mode=mode, slot_rows=active_slots.shape[0], softmax_scale=float(softmax_scale))
    _lib.check(lib.svk_mla_decode_stage1(C.byref(a), _lib.current_stream_handle()), lib)


@torch.no_grad()
def decode_stage2(block_seq: int, context_lens, mid_output, mid_logsumexp, output, *,
                  max_context_len: int | None = None) -> None:
    """LSE-weighted merge of the block partials into output bf16 [B, H, 512] (decode_stage2.py:88); a lane of length 0
    gets zeros."""
    _check_dtypes(torch.int32, context_lens=context_lens)
    _check_dtypes(torch.float32, mid_output=mid_output, mid_logsumexp=mid_logsumexp)
    _check_dtypes(torch.bfloat16, output=output)
    if output.ndim != 3 or output.shape[2] != MLA_LATENT_DIM or output.stride(2) != 1:
        raise ValueError(f"output must have shape [batch, heads, 512], got {tuple(output.shape)}")
    batch, heads = int(output.shape[0]), int(output.shape[1])
    if mid_output.ndim != 4 or mid_output.shape[0] < batch or mid_output.shape[1] < heads or mid_output.stride(3) != 1:
        raise ValueError("mid_output must have shape [batch, heads, blocks, 512]")
    if tuple(mid_logsumexp.shape) != tuple(mid_output.shape[:3]) or mid_logsumexp.stride(2) != 1:
        raise ValueError("mid_logsumexp must match the first three mid_output dimensions")
    width = int(mid_output.shape[2]) * int(block_seq)
    if max_context_len is not None:
        width = min(width, int(max_context_len))
    lib = _lib.load()
    a = _lib.SvkMlaDecodeStage2Args(
        mid_o=_lib.ptr(mid_output), mid_lse=_lib.ptr(mid_logsumexp), context_lens=_lib.ptr(context_lens),
        output=_lib.ptr(output), mid_o_stride_b=mid_output.stride(0), mid_o_stride_h=mid_output.stride(1),
        mid_o_stride_s=mid_output.stride(2), mid_lse_stride_b=mid_logsumexp.stride(0),
        mid_lse_stride_h=mid_logsumexp.stride(1), o_stride_b=output.stride(0), o_stride_h=output.stride(1),
        batch=batch, num_heads=heads, latent_dim=MLA_LATENT_DIM, block_seq=int(block_seq), max_context_len=width)
    _lib.check(lib.svk_mla_decode_stage2(C.byref(a), _lib.current_stream_handle()), lib)


@torch.no_grad()
def copy_latent_to_cache(latent, rope, slot_mapping, latent_cache, rope_cache) -> None:
    """latent [N, 1, 512] / rope [N, 1, 64] rows to the caches at slot_mapping[n]; -1 skips (copy_latent.py:132)."""
    _check_dtypes(torch.bfloat16, latent=latent, rope=rope, latent_cache=latent_cache, rope_cache=rope_cache)
    _check_dtypes(torch.int32, slot_mapping=slot_mapping)
    lat_stride = _cache_rows("latent", latent, MLA_LATENT_DIM)
    rope_stride = _cache_rows("rope", rope, MLA_ROPE_DIM)
    n = int(latent.shape[0])
    if rope.shape[0] != n or tuple(slot_mapping.shape) != (n,):
        raise ValueError(f"latent, rope and slot_mapping must agree on the token count, got {n}, {rope.shape[0]}, "
                         f"{tuple(slot_mapping.shape)}")
    lib = _lib.load()
    a = _lib.SvkMlaStoreLatentArgs(
        latent=_lib.ptr(latent), rope=_lib.ptr(rope), latent_cache=_lib.ptr(latent_cache), rope_cache=_lib.ptr(rope_cache),
        slot_mapping=_lib.ptr(slot_mapping), latent_stride=lat_stride, rope_stride=rope_stride,
        latent_slot_stride=_cache_rows("latent_cache", latent_cache, MLA_LATENT_DIM),
        rope_slot_stride=_cache_rows("rope_cache", rope_cache, MLA_ROPE_DIM), num_slots=latent_cache.shape[0],
        n_tokens=n, latent_dim=MLA_LATENT_DIM, rope_dim=MLA_ROPE_DIM)
    _lib.check(lib.svk_mla_store_latent(C.byref(a), _lib.current_stream_handle()), lib)


@torch.no_grad()
def run_mla_decode(q_latent, q_rope, latent_cache, rope_cache, active_slots, request_indices, context_lens, output,
                   workspace: MlaDecodeWorkspace, *, softmax_scale: float, attn_score=None,
                   max_context_len: int | None = None) -> torch.Tensor:
    """MLA decode attention in latent space (decode_schedule.py:416-513): output bf16 [B, H, 512].  `attn_score` is
    filled with -1e20 inside the call, so a graph replay never inherits a previous step's scores, then receives the raw
    scores of the valid positions."""
    if q_latent.ndim != 3:
        raise ValueError("q_latent must have shape [batch, heads, 512]")
    batch, heads = int(q_latent.shape[0]), int(q_latent.shape[1])
    if context_lens.numel() != batch:
        raise ValueError(f"q_latent batch size and context_lens length must match: {batch} != {context_lens.numel()}")
    if tuple(output.shape) != tuple(q_latent.shape):
        raise ValueError(f"output must have shape {tuple(q_latent.shape)}, got {tuple(output.shape)}")
    if output.device != q_latent.device:
        raise ValueError(f"output is on {output.device}, expected {q_latent.device}")
    _check_dtypes(torch.bfloat16, output=output)
    if workspace.mid_output.shape[0] < batch or workspace.mid_output.shape[1] < heads:
        raise ValueError(f"MLA decode workspace is too small: [batch, heads]={tuple(workspace.mid_output.shape[:2])}, "
                         f"required=[{batch}, {heads}]")
    softmax_scale = float(softmax_scale)
    if not math.isfinite(softmax_scale) or softmax_scale <= 0:
        raise ValueError(f"softmax_scale must be finite and positive, got {softmax_scale}.")
    width = int(active_slots.shape[1]) if max_context_len is None else int(max_context_len)
    if width > workspace.max_context_len:
        raise ValueError(f"MLA decode workspace covers {workspace.max_context_len} positions, {width} required")
    if attn_score is not None:
        _score_mode(attn_score, batch, heads, width)            # f32 and wide enough before anything is written
        if not attn_score.is_contiguous():
            raise ValueError("attn_score must be contiguous")
        lib = _lib.load()
        _lib.check(lib.svk_fill_f32(_lib.ptr(attn_score), attn_score.numel(), -1.0e20, _lib.current_stream_handle()), lib)
    mid_o, mid_lse = workspace.mid_output[:batch, :heads], workspace.mid_logsumexp[:batch, :heads]
    decode_stage1(q_latent, q_rope, latent_cache, rope_cache, active_slots, request_indices, context_lens,
                  workspace.block_seq, mid_o, mid_lse, attn_score=attn_score, max_context_len=width,
                  softmax_scale=softmax_scale)
    decode_stage2(workspace.block_seq, context_lens, mid_o, mid_lse, output, max_context_len=width)
    return output


@torch.no_grad()
def gather_latent_history(latent_cache, rope_cache, active_slots, request_indices, context_lens, packed_start_locs,
                          gathered_latent, gathered_rope, *, max_context_len: int) -> None:
    """Rows active_slots[request_indices[b], j], j < context_lens[b], of both caches to packed rows
    packed_start_locs[b] + j of gathered_latent [capacity, 512] / gathered_rope [capacity, 64] (gather_latent.py:268-336).
    A slot outside the pool gives a zero row; a negative request index has length 0."""
    _check_dtypes(torch.bfloat16, latent_cache=latent_cache, rope_cache=rope_cache, gathered_latent=gathered_latent,
                  gathered_rope=gathered_rope)
    _check_dtypes(torch.int32, active_slots=active_slots, request_indices=request_indices, context_lens=context_lens,
                  packed_start_locs=packed_start_locs)
    lat_stride = _cache_rows("latent_cache", latent_cache, MLA_LATENT_DIM)
    rope_stride = _cache_rows("rope_cache", rope_cache, MLA_ROPE_DIM)
    if latent_cache.shape[0] != rope_cache.shape[0]:
        raise ValueError("latent_cache and rope_cache must have equal slots")
    if active_slots.ndim != 2 or active_slots.stride(1) != 1:
        raise ValueError("active_slots must have shape [rows, max_context_len]")
    if context_lens.ndim != 1 or context_lens.numel() == 0:
        raise ValueError("context_lens must be a non-empty one-dimensional tensor")
    batch = int(context_lens.numel())
    for name, t in (("request_indices", request_indices), ("packed_start_locs", packed_start_locs)):
        if tuple(t.shape) != (batch,):
            raise ValueError(f"{name} must have shape ({batch},), got {tuple(t.shape)}")
    if gathered_latent.ndim != 2 or gathered_latent.shape[1] != MLA_LATENT_DIM or gathered_latent.stride(1) != 1:
        raise ValueError("gathered_latent must have shape [capacity, 512]")
    if gathered_rope.ndim != 2 or gathered_rope.shape[1] != MLA_ROPE_DIM or gathered_rope.stride(1) != 1:
        raise ValueError("gathered_rope must have shape [capacity, 64]")
    if gathered_latent.shape[0] != gathered_rope.shape[0]:
        raise ValueError("gathered_latent and gathered_rope capacities must match")
    width = int(max_context_len)
    if width < 0 or width > active_slots.shape[1]:
        raise ValueError(f"max_context_len must be within active_slots capacity: {width} > {active_slots.shape[1]}")
    lib = _lib.load()
    a = _lib.SvkMlaGatherLatentArgs(
        latent_cache=_lib.ptr(latent_cache), rope_cache=_lib.ptr(rope_cache), active_slots=_lib.ptr(active_slots),
        request_indices=_lib.ptr(request_indices), context_lens=_lib.ptr(context_lens),
        packed_start_locs=_lib.ptr(packed_start_locs), gathered_latent=_lib.ptr(gathered_latent),
        gathered_rope=_lib.ptr(gathered_rope), latent_slot_stride=lat_stride, rope_slot_stride=rope_stride,
        num_slots=latent_cache.shape[0], slots_stride=active_slots.stride(0), out_latent_stride=gathered_latent.stride(0),
        out_rope_stride=gathered_rope.stride(0), out_capacity=gathered_latent.shape[0], batch=batch,
        slot_rows=active_slots.shape[0], max_context_len=width, latent_dim=MLA_LATENT_DIM, rope_dim=MLA_ROPE_DIM)
    _lib.check(lib.svk_mla_gather_latent(C.byref(a), _lib.current_stream_handle()), lib)


@torch.no_grad()
def run_mla_prefill(q, latent_cache, rope_cache, active_slots, request_indices, context_lens, b_start_loc, chunk_lens,
                    project_latent, output, *, qk_nope_head_dim: int = 192, value_head_dim: int = 256) -> torch.Tensor:
    """MLA chunked prefill over the explicit view (layers/mla_attention.py:374-822, 944-984): q bf16 [tokens, H, 256]
    (192 no-position dims | 64 RoPE dims) -> output bf16 [tokens, H, 256].  The chunk's own latent / RoPE rows are
    already in the caches; `context_lens` counts them, `chunk_lens` are the query rows per sequence and `b_start_loc`
    their first row in q.  `project_latent` is the caller's kv_b_proj: bf16 [visible, 512] -> [visible, H * 448]
    (per head 192 key dims | 256 value dims).  The lengths are read on the host (one synchronisation per call)."""
    qk_head_dim = int(qk_nope_head_dim) + MLA_ROPE_DIM
    if qk_head_dim != 256 or int(value_head_dim) != 256:
        raise ValueError(f"MLA explicit prefill requires equal Q/K/V head widths of 256, got qk={qk_head_dim} "
                         f"(nope {qk_nope_head_dim} + rope {MLA_ROPE_DIM}) v={value_head_dim}.")
    if q.ndim != 3 or q.shape[2] != qk_head_dim:
        raise ValueError(f"MLA prefill q must have shape [tokens, local_heads, 256], got {tuple(q.shape)}.")
    if tuple(output.shape) != (q.shape[0], q.shape[1], int(value_head_dim)):
        raise ValueError(f"output must have shape {(q.shape[0], q.shape[1], int(value_head_dim))}, got {tuple(output.shape)}")
    _check_dtypes(torch.bfloat16, q=q, output=output)
    _check_dtypes(torch.int32, context_lens=context_lens, b_start_loc=b_start_loc, chunk_lens=chunk_lens)
    batch, heads, dev = int(context_lens.numel()), int(q.shape[1]), q.device
    for name, t in (("b_start_loc", b_start_loc), ("chunk_lens", chunk_lens)):
        if tuple(t.shape) != (batch,):
            raise ValueError(f"{name} must have shape ({batch},), got {tuple(t.shape)}.")
    contexts, chunks = [int(x) for x in context_lens.tolist()], [int(x) for x in chunk_lens.tolist()]
    if any(c <= 0 or c > n for c, n in zip(chunks, contexts)):
        raise ValueError(f"MLA prefill chunk lengths must be positive and no larger than their contexts: "
                         f"chunks={chunks} contexts={contexts}.")
    visible, width = sum(contexts), max(contexts)
    # packed offsets and the slot table packed_offsets[b] + j of the explicit view
    offsets = [0] * batch
    for i in range(1, batch):
        offsets[i] = offsets[i - 1] + contexts[i - 1]
    packed_offsets = torch.tensor(offsets, dtype=torch.int32, device=dev)
    packed_slots = packed_offsets[:, None] + torch.arange(width, dtype=torch.int32, device=dev)[None, :]
    gathered_latent = torch.empty((visible, MLA_LATENT_DIM), dtype=torch.bfloat16, device=dev)
    gathered_rope = torch.empty((visible, MLA_ROPE_DIM), dtype=torch.bfloat16, device=dev)
    gather_latent_history(latent_cache, rope_cache, active_slots, request_indices, context_lens, packed_offsets,
                          gathered_latent, gathered_rope, max_context_len=width)
    expanded = project_latent(gathered_latent)
    projected = int(qk_nope_head_dim) + int(value_head_dim)
    if expanded.dtype is not torch.bfloat16 or expanded.numel() != visible * heads * projected:
        raise RuntimeError(f"project_latent must return bf16 [{visible}, {heads} * {projected}], got "
                           f"{expanded.dtype} {tuple(expanded.shape)}")
    expanded = expanded.view(visible, heads, projected)
    k = torch.empty((visible, heads, qk_head_dim), dtype=torch.bfloat16, device=dev)
    k[..., :qk_nope_head_dim].copy_(expanded[..., :qk_nope_head_dim])
    k[..., qk_nope_head_dim:].copy_(gathered_rope[:, None, :])
    v = expanded[..., qk_nope_head_dim:].contiguous()
    from .context_flashattention_nopad import context_attention_fwd
    context_attention_fwd(q, k, v, output, torch.arange(batch, dtype=torch.int32, device=dev), b_start_loc, context_lens,
                          context_lens - chunk_lens, max(chunks), packed_slots)
    return output
