"""GPU parity of svk_prefill_score at head_dim 256 (rows-split LDS-tile kernel, generic fallback at G = 9, statistics
from the attention launch) against the oracle, at the tolerances of tests/test_gpu_prefill_score.py: probability rtol 2e-2 /
atol 2e-4 and max abs < 1e-3; logits the same -inf pattern, rtol 1e-4 / atol 2e-3 on the finite entries."""

import numpy as np
import pytest

from oracle import bf16_round, f32_to_bf16_bits
from oracle import prefill_score as ops

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
D, DEV = 256, "cuda:0"


def t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def to_bf16(x):
    return t(f32_to_bf16_bits(x).view(np.int16)).view(torch.bfloat16)


def paged_batch(rng, Hq, Hkv, seqs, window, n_tensors):
    """bf16-representable q and K (V) over a permuted slot table; -> tensors, (b_req, b_start, b_seq, b_cache, req, qs, qe)"""
    ctx = [c + n for c, n in seqs]
    nb, slots, off = len(seqs), sum(ctx) + 64, 0
    kv = [bf16_round((rng.standard_normal((slots, Hkv, D)) * 0.4).astype(np.float32)) for _ in range(n_tensors)]
    q = bf16_round((rng.standard_normal((sum(n for _, n in seqs), Hq, D)) * 0.4).astype(np.float32))
    req = np.zeros((nb + 2, max(ctx) + 5), dtype=np.int32)
    perm = rng.permutation(slots).astype(np.int32)
    rows = rng.permutation(nb + 2)[:nb].astype(np.int32)
    for i, L in enumerate(ctx):
        req[rows[i], :L] = perm[off: off + L]
        off += L
    b_start = np.concatenate(([0], np.cumsum([n for _, n in seqs])[:-1])).astype(np.int32)
    b_seq, b_cache = np.array(ctx, np.int32), np.array([c for c, _ in seqs], np.int32)
    qs = np.array([max(L - window, c) for L, (c, n) in zip(ctx, seqs)], np.int32)
    return q, kv, (rows, b_start, b_seq, b_cache, req, qs, b_seq.copy())


def compare(out, ref, logits):
    if logits:
        assert np.array_equal(np.isneginf(out), np.isneginf(ref))
        fin = np.isfinite(ref)
        np.testing.assert_allclose(out[fin], ref[fin], rtol=1e-4, atol=2e-3)
    else:
        np.testing.assert_allclose(out, ref, rtol=2e-2, atol=2e-4)
        assert np.abs(out - ref).max() < 1e-3


@pytest.mark.parametrize("cfg", [
    # Hq, Hkv, [(cached, chunk)], window, candidate_start, num_recent, mode
    (4, 4, [(130, 190), (0, 17)], 17, 3, 40, "probability"),     # G = 1, window < one row block, range ends inside a key block
    (8, 4, [(255, 129), (640, 1)], 128, 0, 0, "probability"),    # G = 2, diagonal across a block boundary, one-token chunk
    (16, 4, [(64, 65)], 90, 70, 30, "probability"),              # G = 4, window not a multiple of 32, longer than the chunk
    (16, 2, [(511, 513)], 128, 130, 200, "probability"),         # G = 8, nine key blocks, masked and mask-free blocks
    (8, 2, [(300, 260), (5, 130)], 128, 0, 0, "logits"),         # G = 4 logits, two ranges
    (5, 5, [(90, 70)], 48, 16, 0, "logits"),                     # G = 1, odd head count, partial last row block
    (18, 2, [(100, 200)], 64, 0, 0, "probability"),              # G = 9: the generic kernel at 256
])
def test_prefill_score_d256_vs_oracle(cfg):
    from sparse_vllm_amd.kernels.prefill_score import prefill_score_fwd
    Hq, Hkv, seqs, window, cstart, nrecent, mode = cfg
    q, (k,), (rows, b_start, b_seq, b_cache, req, qs, qe) = paged_batch(np.random.default_rng(Hq + window), Hq, Hkv, seqs, window, 1)
    max_q = int((qe - qs).max())
    tq, tk = to_bf16(q), to_bf16(k)
    orders = [None] if len(seqs) == 1 else [None, np.arange(len(seqs) - 1, -1, -1).astype(np.int32)]
    for bi in orders:                                            # range i <-> sequence i, then the ranges reversed
        s, e = (qs, qe) if bi is None else (qs[bi], qe[bi])
        ref = np.empty((len(seqs), int(b_seq.max())), np.float32)
        ops.prefill_score_fwd(q, k, ref, rows, b_start, b_seq, b_cache, max_q, req, s, e, candidate_start=cstart,
                              num_recent_tokens=nrecent, score_mode=mode, batch_indices=bi)
        out = torch.full(ref.shape, 777.0, dtype=torch.float32, device=DEV)      # an unwritten column shows
        prefill_score_fwd(tq, tk, out, t(rows), t(b_start), t(b_seq), t(b_cache), max_q, t(req), t(s), t(e),
                          candidate_start=cstart, num_recent_tokens=nrecent, score_mode=mode,
                          batch_indices=None if bi is None else t(bi))
        compare(out.cpu().numpy(), ref, mode == "logits")


@pytest.mark.parametrize("cfg", [
    # Hq, Hkv, [(cached, chunk)], window
    (8, 4, [(100, 300), (700, 65)], 48),
    (20, 20, [(0, 20)], 16),
    (16, 4, [(500, 700), (0, 333), (64, 40)], 128),
])
def test_prefill_score_d256_from_attention_statistics(cfg):
    """context_attention_fwd(score_stats=...) leaves the window rows' statistics and a cleared score row at head_dim 256,
    prefill_score_fwd(row_stats=...) runs its final pass only: the scores of the three-launch form (the same row sums in
    another order, the bar of the head_dim 128 test: rtol 1e-4) and of the oracle; the attention output is untouched."""
    from sparse_vllm_amd.kernels.context_flashattention_nopad import context_attention_fwd
    from sparse_vllm_amd.kernels.prefill_score import prefill_score_fwd, prefill_score_window_pad
    Hq, Hkv, seqs, window = cfg
    q, (k, v), (rows, b_start, b_seq, b_cache, req, qs, qe) = paged_batch(np.random.default_rng(Hq + window), Hq, Hkv, seqs, window, 2)
    nb, max_q, max_in = len(seqs), int((qe - qs).max()), max(n for _, n in seqs)
    tq, tk, tv = to_bf16(q), to_bf16(k), to_bf16(v)
    meta = (t(rows), t(b_start), t(b_seq), t(b_cache))
    ref3 = torch.full((nb, int(b_seq.max())), 7.0, dtype=torch.float32, device=DEV)
    prefill_score_fwd(tq, tk, ref3, *meta, max_q, t(req), t(qs), t(qe))
    o_plain, o_stats = torch.empty_like(tq), torch.empty_like(tq)
    context_attention_fwd(tq, tk, tv, o_plain, *meta, max_in, t(req))
    wpad = prefill_score_window_pad(Hq, Hkv, max_q)
    stats = torch.full((nb * Hq * wpad,), float("nan"), dtype=torch.float32, device=DEV)
    got = torch.full_like(ref3, 7.0)
    context_attention_fwd(tq, tk, tv, o_stats, *meta, max_in, t(req), score_stats=(stats, t(qs), wpad, got))
    torch.cuda.synchronize()
    assert torch.equal(o_plain.view(torch.int16), o_stats.view(torch.int16))
    assert not got.any()                                                        # cleared by the attention launch
    st = stats.view(nb, Hq, wpad).cpu().numpy()
    for i in range(nb):
        assert np.isfinite(st[i, :, : qe[i] - qs[i]]).all() and np.isnan(st[i, :, qe[i] - qs[i]:]).all()
    prefill_score_fwd(tq, tk, got, *meta, max_q, t(req), t(qs), t(qe), row_stats=stats)
    a, b = got.cpu().numpy(), ref3.cpu().numpy()
    print("fused vs three-launch: max relative difference", float((np.abs(a - b) / np.maximum(np.abs(b), 1e-30))[b > 0].max()))
    np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-8)
    out = np.empty_like(b)
    ops.prefill_score_fwd(q, k, out, rows, b_start, b_seq, b_cache, max_q, req, qs, qe)
    compare(a, out, False)
