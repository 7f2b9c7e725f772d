"""R-KV scoring on device (libsvk.so): redundancy scores straight from the paged K cache and the joint
importance / redundancy selection.  Device restatement of RKVCacheManager.redundancy_scores_from_keys_batch,
joint_retention_scores and select_rkv_indices_batch (engine/cache_manager/rkv.py:617-842); see include/svk.h."""

from __future__ import annotations

import ctypes as C

import torch

from .. import _lib
from .h2o_ops import select_prefix_topk_suffix


class RkvWorkspace:
    """Grow-only device scratch of the R-KV launches (similarity averages, inverse norms, the joint score rows).  The
    capacity is rounded up to a power of two, so a caller whose window or batch changes from call to call allocates a
    handful of times over the life of the process and never per call."""

    def __init__(self):
        self.buf = None

    def take(self, nbytes: int, device) -> torch.Tensor:
        if self.buf is None or self.buf.numel() < nbytes or self.buf.device != torch.device(device):
            cap = 1 << max(12, (int(nbytes) - 1).bit_length())
            self.buf = torch.empty((cap,), dtype=torch.uint8, device=device)
        return self.buf


_WORKSPACES: dict = {}


def _default_workspace(device) -> RkvWorkspace:
    return _WORKSPACES.setdefault(torch.device(device), RkvWorkspace())


def _check_tokens(n: int, max_tokens: int):
    if n > int(max_tokens):
        raise RuntimeError(
            f"R-KV redundancy scoring is quadratic in the candidate tokens: {n} tokens exceed the limit max_tokens="
            f"{int(max_tokens)}. Shorten the redundancy window or raise the limit explicitly.")


def _redundancy_launch(lib, k_cache, slots, n, ws_buf, redundancy, *, similarity_threshold, recent_similar_keep, max_tokens):
    assert k_cache.dim() == 3 and k_cache.dtype == torch.bfloat16 and k_cache.stride(2) == 1
    assert k_cache.stride(1) == k_cache.shape[2], "the KV heads of a slot must be contiguous"
    assert slots.dim() == 2 and slots.dtype == torch.int32 and slots.stride(1) == 1 and slots.shape[1] >= n
    rows = int(slots.shape[0])
    a = _lib.SvkRkvRedundancyArgs(
        k_cache=_lib.ptr(k_cache), slots=_lib.ptr(slots), redundancy=_lib.ptr(redundancy), workspace=_lib.ptr(ws_buf),
        workspace_bytes=0 if ws_buf is None else ws_buf.numel() * ws_buf.element_size(),
        kv_slot_stride=k_cache.stride(0), kv_num_slots=k_cache.shape[0], slot_stride=slots.stride(0),
        redundancy_stride=0 if redundancy is None else redundancy.stride(0), rows=rows, n=int(n),
        num_kv_heads=k_cache.shape[1], head_dim=k_cache.shape[2], recent_similar_keep=int(recent_similar_keep),
        max_tokens=int(max_tokens), similarity_threshold=float(similarity_threshold))
    _lib.check(lib.svk_rkv_redundancy(C.byref(a), _lib.current_stream_handle()), lib)


def redundancy_scores_from_slots(k_cache: torch.Tensor, slots: torch.Tensor, *, similarity_threshold: float,
                                 recent_similar_keep: int, max_tokens: int, out: torch.Tensor | None = None,
                                 workspace: RkvWorkspace | None = None) -> torch.Tensor:
    """redundancy_scores_from_keys_batch (rkv.py:656-697) of the keys `k_cache[slots[row, c]]` (int32 [rows, n], oldest
    token first, any slot order, row stride >= n): f32 [rows, n], each row a softmax over its n tokens."""
    rows, n = int(slots.shape[0]), int(slots.shape[1])
    if n == 0:
        return torch.empty((rows, 0), dtype=torch.float32, device=slots.device)
    _check_tokens(n, max_tokens)
    lib = _lib.load()
    if out is None:
        out = torch.empty((rows, n), dtype=torch.float32, device=slots.device)
    assert out.dtype == torch.float32 and tuple(out.shape) == (rows, n) and out.stride(1) == 1
    ws = (workspace or _default_workspace(slots.device)).take(lib.svk_rkv_redundancy_workspace_bytes(rows, n), slots.device)
    _redundancy_launch(lib, k_cache, slots, n, ws, out, similarity_threshold=similarity_threshold,
                       recent_similar_keep=recent_similar_keep, max_tokens=max_tokens)
    return out


def select_rkv_indices_batch(k_cache: torch.Tensor, slot_table_rows: torch.Tensor, importance: torch.Tensor, *, kv_len: int,
                             budget: int, num_sink: int, num_recent: int, alpha: float, similarity_threshold: float,
                             recent_similar_keep: int, redundancy_window: int, max_tokens: int,
                             out: torch.Tensor | None = None, workspace: RkvWorkspace | None = None) -> torch.Tensor:
    """select_rkv_indices_batch (rkv.py:767-842) for rows of one uniform `kv_len`: `slot_table_rows` int32 [rows, >= kv_len]
    are the rows' slot-table entries, `importance` f32 [rows, >= kv_len] their importance by cache position.  Returns
    ascending int64 [rows, keep]: sink ++ top-k of the joint score ++ recent (the index SET of the reference, ties to
    the lowest index).  Enqueues launches only: no host synchronisation."""
    assert slot_table_rows.dim() == 2 and slot_table_rows.dtype == torch.int32 and slot_table_rows.stride(1) == 1
    assert importance.dim() == 2 and importance.dtype == torch.float32 and importance.stride(1) == 1
    rows, kv_len, budget = int(slot_table_rows.shape[0]), int(kv_len), int(budget)
    assert importance.shape[0] == rows and importance.shape[1] >= kv_len and slot_table_rows.shape[1] >= kv_len
    dev = slot_table_rows.device
    if kv_len <= budget:
        return torch.arange(kv_len, dtype=torch.long, device=dev).unsqueeze(0).expand(rows, -1).contiguous()
    num_sink = min(int(num_sink), kv_len)
    num_recent = min(int(num_recent), max(0, kv_len - num_sink))
    cand_end = max(num_sink, kv_len - num_recent)
    num_top = max(0, budget - num_sink - num_recent)
    n_cand = cand_end - num_sink
    if num_top <= 0 or n_cand <= 0:
        keep = torch.cat((torch.arange(0, num_sink, dtype=torch.long, device=dev),
                          torch.arange(kv_len - num_recent, kv_len, dtype=torch.long, device=dev)))
        return keep.unsqueeze(0).expand(rows, -1).contiguous()
    window = n_cand if int(redundancy_window) == 0 else min(int(redundancy_window), n_cand)
    _check_tokens(window, max_tokens)
    lib = _lib.load()
    red_bytes = (int(lib.svk_rkv_redundancy_workspace_bytes(rows, window)) + 255) & ~255
    buf = (workspace or _default_workspace(dev)).take(red_bytes + rows * kv_len * 4, dev)
    scores = buf[red_bytes: red_bytes + rows * kv_len * 4].view(torch.float32).view(rows, kv_len)
    if window > 0:
        _redundancy_launch(lib, k_cache, slot_table_rows[:, cand_end - window: cand_end], window, buf[:red_bytes], None,
                           similarity_threshold=similarity_threshold, recent_similar_keep=recent_similar_keep,
                           max_tokens=max_tokens)
    j = _lib.SvkRkvJointScoreArgs(
        avg=_lib.ptr(buf), importance=_lib.ptr(importance), scores=_lib.ptr(scores), redundancy=None,
        avg_stride=lib.svk_rkv_redundancy_avg_stride(window), importance_stride=importance.stride(0),
        score_stride=scores.stride(0), redundancy_stride=0, rows=rows, window=window, n_candidates=n_cand,
        candidate_start=num_sink, alpha=float(alpha))
    _lib.check(lib.svk_rkv_joint_scores(C.byref(j), _lib.current_stream_handle()), lib)
    return select_prefix_topk_suffix(scores, kv_len=kv_len, prefix=num_sink, topk=min(num_top, n_cand), suffix=num_recent,
                                     out=out)
