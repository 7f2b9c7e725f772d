"""head_dim 256 split-KV decode through the public wrappers against `oracle.decode_attention`.  The project's bars
(partials / outputs rtol = atol = 2e-2 against the tiled oracle, raw scores atol 1e-4 + rtol 1e-5) and one sharper bar
against the float64 dense ground truth: max|o - o_dense| <= 4 e_ref + 2^-9 max|o_dense|, e_ref = the tiled oracle's own
error on the same inputs (summation order, 32- instead of 16-token max tile, hardware exp: each of the order of its bf16-P
error, plus half an output ulp; a dropped or doubled token of a 17- or 33-token row, ~1e-2, does not fit under it)."""

import numpy as np
import pytest

from oracle import bf16_round, f32_to_bf16_bits
from oracle import decode_attention as oda

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
D = 256
TOL = dict(rtol=2e-2, atol=2e-2)


def _case(seed, B, Hq, Hkv, lens, place=0, page=1):
    """bf16 values at scale 0.3 from `seed`; their slots (a permuted table with spare rows, or pages) from `place`."""
    rng, prng = np.random.default_rng(seed), np.random.default_rng(1000 + place)
    draw = lambda *s: bf16_round((rng.standard_normal(s) * 0.3).astype(np.float32))
    lens = np.asarray(lens, dtype=np.int32)
    npg = -(-lens // page)
    pperm = prng.permutation(int(npg.sum()) + 8).astype(np.int32)
    rows = rng.permutation(B + 3)[:B].astype(np.int32)
    req = np.zeros((B + 3, int(lens.max()) + 7), dtype=np.int32)
    preq = np.zeros_like(req)
    q, k, v = draw(B, Hq, D), np.zeros((pperm.size * page, Hkv, D), np.float32), np.zeros((pperm.size * page, Hkv, D), np.float32)
    off = 0
    for b in range(B):
        pg, t = pperm[off: off + npg[b]], np.arange(lens[b])
        off += npg[b]
        preq[rows[b], : npg[b]] = pg
        req[rows[b], : lens[b]] = pg[t // page] * page + t % page
        k[req[rows[b], : lens[b]]], v[req[rows[b], : lens[b]]] = draw(lens[b], Hkv, D), draw(lens[b], Hkv, D)
    return q, k, v, req, rows, lens, preq


_t = lambda x: torch.from_numpy(x).to("cuda:0")
_bf = lambda x: _t(f32_to_bf16_bits(x).view(np.int16).copy()).view(torch.bfloat16)


def _run(q, k, v, req, rows, lens, block_seq, mode=0, score_init=-1e20, caches=None, **kw):
    from sparse_vllm_amd.kernels import flash_decode_stage1, flash_decode_stage1_with_score, flash_decode_stage2
    (B, Hq, _), max_len = q.shape, int(lens.max())
    nblk = -(-max_len // block_seq)
    tq, (tk, tv), tl = _bf(q), caches or (_bf(k), _bf(v)), _t(lens)
    mid = torch.full((B, Hq, nblk, D), 7.0, device="cuda:0")
    lse = torch.full((B, Hq, nblk), 7.0, device="cuda:0")
    args, score = (tq, tk, tv, _t(req), _t(rows), tl, max_len, mid, lse), None
    if mode:
        score = torch.full((B, max_len) if mode == 2 else (B, Hq, max_len), score_init, device="cuda:0")
        flash_decode_stage1_with_score(*args, score, block_seq, **kw)
    else:
        flash_decode_stage1(*args, block_seq, **kw)
    o = kw.get("direct_out")
    if o is None:
        o = torch.empty_like(tq)
        flash_decode_stage2(mid, lse, tl, o, block_seq)
    torch.cuda.synchronize()
    return mid.cpu().numpy(), lse.cpu().numpy(), None if score is None else score.cpu().numpy(), o.float().cpu()


@pytest.mark.parametrize("mode", [0, 2, 3])
@pytest.mark.parametrize("shape", [
    (2, 8, 4, (100, 33), 32),          # G = 2, ragged last tile, empty blocks for the short lane
    (3, 8, 1, (300, 257, 1), 64),      # one KV head, G = 8 (two accumulator row groups), 1-token row
    (1, 6, 2, (545,), 544),            # G = 3, > 256 tokens in one block: the head-max chunk combine mid-block and at the end
    (2, 4, 4, (95, 17), 48),           # G = 1, block_seq not a multiple of 32
    (2, 16, 8, (70, 64), 32),          # 8 KV heads: the 1024-thread form
])
def test_decode_d256_vs_oracle(shape, mode):
    B, Hq, Hkv, lens, block_seq = shape
    q, k, v, req, rows, lens, _ = _case(4321 + B + Hq + mode, B, Hq, Hkv, lens)
    max_len = int(lens.max())
    score_ref = {0: None, 2: np.full((B, max_len), -1e20, np.float32), 3: np.full((B, Hq, max_len), -1e20, np.float32)}[mode]
    mid_ref, lse_ref = oda.flash_decode_stage1(q, k, v, req, rows, lens, max_len, block_seq, attn_score=score_ref)
    o_ref = bf16_round(oda.flash_decode_stage2(mid_ref, lse_ref, lens, block_seq))
    o_dense = oda.decode_attention_dense(q, k, v, req, rows, lens)[0]
    mid, lse, score, o = _run(q, k, v, req, rows, lens, block_seq, mode)
    np.testing.assert_allclose(lse, lse_ref, **TOL)
    np.testing.assert_allclose(mid, mid_ref, **TOL)
    np.testing.assert_allclose(o.numpy(), o_ref, **TOL)
    if mode:
        np.testing.assert_allclose(score, score_ref, rtol=1e-5, atol=1e-4)      # beyond a lane's length: still -1e20
    e_ref, err = np.abs(o_ref - o_dense).max(), np.abs(o.numpy() - o_dense).max()
    bound = 4 * e_ref + 2.0 ** -9 * np.abs(o_dense).max()
    print(f"d256 {shape} mode {mode}: err {err:.3e} e_ref {e_ref:.3e} err / bound {err / bound:.3f}")
    assert err <= bound


def test_equivalent_launch_forms_are_bit_equal():
    from sparse_vllm_amd.kernels import store_kvcache
    B, Hq, Hkv, lens, bs = 2, 8, 4, (30, 9), 32
    q, k, v, req, rows, lens, preq = c = _case(77, B, Hq, Hkv, lens, page=16)
    base = _run(*c[:6], bs)[3]
    # (b) page slots of 16 tokens address the same rows as the token-slot table
    assert torch.equal(_run(q, k, v, preq, rows, lens, bs, slot_page_size=16)[3], base)
    # (c) the same logical rows in other slots
    assert torch.equal(_run(*_case(77, B, Hq, Hkv, lens, place=1)[:6], bs)[3], base)
    # (a) fused store + direct output in one launch == store_kvcache, stage 1, stage 2.  Lane 0's newest row is missing
    # from the cache and arrives as new_kv; lane 1 (slot_mapping -1) offers other values that must not be stored.
    newest = req[rows, lens - 1]
    other = np.array([0, 1], np.float32)[:, None, None]
    nk, nv = _bf(k[newest] + other), _bf(v[newest] + other)
    sm = _t(np.array([newest[0], -1], np.int32))
    k0, v0 = k.copy(), v.copy()
    k0[newest[0]] = v0[newest[0]] = 0
    fused, plain = (_bf(k0), _bf(v0)), (_bf(k0), _bf(v0))
    o_fused = _run(*c[:6], bs, caches=fused, new_kv=(nk, nv, sm), direct_out=torch.empty_like(_bf(q)))[3]
    store_kvcache(nk, nv, *plain, sm)
    o_plain = _run(*c[:6], bs, caches=plain)[3]
    assert torch.equal(o_fused, o_plain) and torch.equal(o_fused, base)
    assert torch.equal(fused[0], plain[0]) and torch.equal(fused[1], plain[1]) and torch.equal(fused[0], _bf(k))


def test_score_overwrite_needs_no_prefill():
    B, Hq, Hkv, lens, bs = 2, 8, 4, (100, 33), 32
    c = _case(9, B, Hq, Hkv, lens)
    ref = np.full((B, 100), -1e20, np.float32)
    oda.flash_decode_stage1(*c[:6], 100, bs, attn_score=ref)
    score = _run(*c[:6], bs, 2, score_init=7.0, score_overwrite=True)[2]
    for b, n in enumerate(lens):
        np.testing.assert_allclose(score[b, :n], ref[b, :n], rtol=1e-5, atol=1e-4)
        assert (score[b, n:] == 7.0).all()


@pytest.mark.parametrize("nblk,split", [(132, False), (300, True)])      # the 1024-thread form, the two-level form
def test_stage2_wide_and_split_forms(nblk, split):
    from sparse_vllm_amd.kernels import flash_decode_stage2
    from sparse_vllm_amd.kernels.flash_decoding_stage2 import split_workspace
    rng = np.random.default_rng(nblk)
    mid = rng.standard_normal((1, 2, nblk, D)).astype(np.float32)
    lse = (rng.standard_normal((1, 2, nblk)) * 2).astype(np.float32)
    lens = np.array([nblk * 16], np.int32)
    ws = split_workspace(1, 2, D, nblk, "cuda:0") if split else None
    assert (ws is not None) == split
    o = torch.empty((1, 2, D), dtype=torch.bfloat16, device="cuda:0")
    flash_decode_stage2(_t(mid), _t(lse), _t(lens), o, 16, workspace=ws)
    torch.cuda.synchronize()
    np.testing.assert_allclose(o.float().cpu().numpy(), bf16_round(oda.flash_decode_stage2(mid, lse, lens, 16)), **TOL)
    assert not split or int(ws[1].abs().sum()) == 0
