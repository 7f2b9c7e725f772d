"""GPU: MLA latent-cache decode (svk_mla_decode_stage1/2, svk_mla_store_latent) against float64 softmax attention over
the gathered bf16 rows.  Observed on an MI355X: see the figures in docs/KERNELS.md (MLA section)."""

from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

L, R, PAD = 512, 64, 8
SCALE = 1.0 / 24.0            # 576 ** -0.5: unit-variance q and rows give scaled logits of standard deviation 1
SENTINEL = 7.5


def build(H, lens, layout, *, perm_seed=1, masked=()):
    """Seeded inputs.  The caches are views into the middle of larger allocations of finite values; the slot table is
    wider than the batch and `request_indices` walks it backwards.  `masked` = (lane, position, slot id) overrides."""
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(1234)
    B, W, n = len(lens), max(max(lens), 1), sum(lens)
    q = torch.randn(B, H, L + R, generator=g).bfloat16()
    rows = torch.randn(n, L + R, generator=g).bfloat16()
    pool = n + 37
    slots = torch.randperm(pool, generator=torch.Generator().manual_seed(perm_seed))[:n].to(torch.int32)
    big = torch.randn(pool + 2 * PAD, L + R, generator=g).bfloat16()
    big[PAD + slots.long()] = rows
    if layout == "interleaved":
        buf = big.to(dev)[PAD:PAD + pool]
        lat, rope = buf[:, :L], buf[:, L:]
    else:
        lat = big[:, :L].contiguous().to(dev)[PAD:PAD + pool].unsqueeze(1)
        rope = big[:, L:].contiguous().to(dev)[PAD:PAD + pool].unsqueeze(1)
    table = torch.zeros(B + 2, W, dtype=torch.int32)
    req = torch.tensor([B + 1 - i for i in range(B)], dtype=torch.int32)
    per_lane, keep, o = [], [], 0
    for i, n_i in enumerate(lens):
        table[req[i], :n_i] = slots[o:o + n_i]
        ok = torch.ones(n_i, dtype=torch.bool)
        for lane, pos, sid in masked:
            if lane == i:
                table[req[i], pos] = pool if sid == "pool" else sid
                ok[pos] = False
        per_lane.append(rows[o:o + n_i])
        keep.append(ok)
        o += n_i
    return SimpleNamespace(H=H, lens=lens, B=B, W=W, q=q, per_lane=per_lane, keep=keep, lat=lat, rope=rope,
                           q_lat=q[..., :L].contiguous().to(dev), q_rope=q[..., L:].contiguous().to(dev),
                           table=table.to(dev), req=req.to(dev), ctx=torch.tensor(lens, dtype=torch.int32, device=dev))


def reference(c):
    """float64: raw scores per lane ([H, len]) and softmax attention output [B, H, 512] over the unmasked positions."""
    out, scores = torch.zeros(c.B, c.H, L, dtype=torch.float64), []
    for i in range(c.B):
        x = c.per_lane[i].double()
        s = c.q[i].double() @ x.T
        scores.append(s)
        if c.keep[i].any():
            p = torch.softmax(s[:, c.keep[i]] * SCALE, dim=-1)
            out[i] = p @ x[c.keep[i], :L]
    return out, scores


def run(c, block_seq, score=None):
    from sparse_vllm_amd.kernels import allocate_mla_decode_workspace, run_mla_decode
    ws = allocate_mla_decode_workspace(c.B, c.H, c.W, "cuda", block_seq=block_seq)
    out = torch.full((c.B, c.H, L), 3.0, dtype=torch.bfloat16, device="cuda")
    run_mla_decode(c.q_lat, c.q_rope, c.lat, c.rope, c.table, c.req, c.ctx, out, ws, softmax_scale=SCALE, attn_score=score)
    torch.cuda.synchronize()
    return out, ws


def check_scores(c, got, ref_scores, headmax, rest):
    """valid positions within the raw-score contract 1e-4 + 1e-5 |x|; every other position holds `rest`"""
    got, rest = got.cpu().double(), float(torch.tensor(rest, dtype=torch.float32))
    for i in range(c.B):
        want = ref_scores[i].max(dim=0).values if headmax else ref_scores[i]
        mine = got[i] if headmax else got[i, :c.H]
        n_i, ok = c.lens[i], c.keep[i]
        err = (mine[..., :n_i][..., ok] - want[..., ok]).abs()
        print(f"lane {i}: max score error {err.max().item() if err.numel() else 0.0:.3e}")
        assert bool((err <= 1e-4 + 1e-5 * want[..., ok].abs()).all())
        assert bool((mine[..., :n_i][..., ~ok] == rest).all()) and bool((mine[..., n_i:] == rest).all())


@pytest.mark.parametrize("layout", ["split", "interleaved"])
@pytest.mark.parametrize("H", [1, 5, 16, 40, 128])
@pytest.mark.parametrize("block_seq,lens", [(64, [0, 1, 33, 2 * 64 + 17]), (32, [31, 32, 31, 32, 33]),
                                            (128, [97, 128 + 17, 3 * 128 + 5])])      # 4 tiles per block: the ring reuses both buffers
def test_output_and_partials_match_float64(H, block_seq, lens, layout):
    c = build(H, lens, layout)
    want, ref_scores = reference(c)
    out, ws = run(c, block_seq)
    err = (out.cpu().double() - want).abs()
    print(f"H={H} block_seq={block_seq} {layout}: max output error {err.max().item():.3e}")
    assert bool((err <= 2e-2 + 2e-2 * want.abs()).all())
    for i, n_i in enumerate(lens):
        if n_i == 0:
            assert bool((out[i] == 0).all())
        else:       # first block's log-sum-exp of the scaled logits
            lse = torch.logsumexp(ref_scores[i][:, :block_seq] * SCALE, dim=-1)
            assert torch.allclose(ws.mid_logsumexp[i, :, 0].cpu().double(), lse, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("block_seq", [64, 128])
@pytest.mark.parametrize("headmax", [True, False])
@pytest.mark.parametrize("H", [5, 40])
def test_scores_match_float64_and_leave_the_rest_alone(H, headmax, block_seq):
    from sparse_vllm_amd.kernels import decode_stage1
    c = build(H, [0, 1, 33, 2 * 64 + 17], "split")
    _, ref_scores = reference(c)
    shape = (c.B, c.W) if headmax else (c.B, H, c.W)
    score = torch.zeros(shape, dtype=torch.float32, device="cuda")
    _, ws = run(c, block_seq, score)
    check_scores(c, score, ref_scores, headmax, -1.0e20)
    score.fill_(SENTINEL)                                     # the bare stage 1 writes the valid positions only
    decode_stage1(c.q_lat, c.q_rope, c.lat, c.rope, c.table, c.req, c.ctx, block_seq, ws.mid_output, ws.mid_logsumexp,
                  attn_score=score, softmax_scale=SCALE)
    check_scores(c, score, ref_scores, headmax, SENTINEL)


@pytest.mark.parametrize("headmax", [True, False])
def test_slots_outside_the_pool_are_masked(headmax):
    from sparse_vllm_amd.kernels import decode_stage1, decode_stage2
    c = build(40, [50, 70], "interleaved", masked=((0, 3, -1), (0, 40, "pool")))
    want, ref_scores = reference(c)
    from sparse_vllm_amd.kernels import allocate_mla_decode_workspace
    ws = allocate_mla_decode_workspace(c.B, c.H, c.W, "cuda", block_seq=32)
    score = torch.full((c.B, c.W) if headmax else (c.B, c.H, c.W), SENTINEL, dtype=torch.float32, device="cuda")
    out = torch.empty((c.B, c.H, L), dtype=torch.bfloat16, device="cuda")
    decode_stage1(c.q_lat, c.q_rope, c.lat, c.rope, c.table, c.req, c.ctx, 32, ws.mid_output, ws.mid_logsumexp,
                  attn_score=score, softmax_scale=SCALE)
    decode_stage2(32, c.ctx, ws.mid_output, ws.mid_logsumexp, out)
    torch.cuda.synchronize()
    assert bool(((out.cpu().double() - want).abs() <= 2e-2 + 2e-2 * want.abs()).all())
    check_scores(c, score, ref_scores, headmax, SENTINEL)


def test_result_does_not_depend_on_slot_order_and_graph_replay_is_exact():
    from sparse_vllm_amd.kernels import allocate_mla_decode_workspace, copy_latent_to_cache, run_mla_decode
    lens, got = [0, 1, 33, 145], []
    for perm_seed in (1, 2):
        c = build(40, lens, "split", perm_seed=perm_seed)
        score = torch.zeros((c.B, c.W), dtype=torch.float32, device="cuda")
        out, ws = run(c, 64, score)
        got.append((out, ws.mid_logsumexp.clone(), score))
    for x, y in zip(*got):
        assert torch.equal(x, y)
    # graph of the decode step (store the new token's row, then attend) against the eager result
    new_lat = torch.randn(c.B, 1, L, device="cuda").bfloat16()
    new_rope = torch.randn(c.B, 1, R, device="cuda").bfloat16()
    new_slots = c.table[c.req.long(), (c.ctx - 1).clamp(min=0).long()].masked_fill(c.ctx == 0, -1)
    out_g, score_g = torch.empty_like(out), torch.empty_like(score)
    ws_g = allocate_mla_decode_workspace(c.B, c.H, c.W, "cuda", block_seq=64)

    def step(o, s, w):
        copy_latent_to_cache(new_lat, new_rope, new_slots, c.lat, c.rope)
        run_mla_decode(c.q_lat, c.q_rope, c.lat, c.rope, c.table, c.req, c.ctx, o, w, softmax_scale=SCALE, attn_score=s)
    step(out, score, ws)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(out_g, score_g, ws_g)
    for _ in range(2):
        out_g.zero_()
        score_g.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out_g, out) and torch.equal(score_g, score)
        assert torch.equal(ws_g.mid_logsumexp, ws.mid_logsumexp)


def test_copy_latent_to_cache_is_indexed_assignment():
    from sparse_vllm_amd.kernels import copy_latent_to_cache
    g = torch.Generator().manual_seed(5)
    lat = torch.randn(7, 1, L, generator=g).bfloat16().cuda()
    rope = torch.randn(7, 1, R, generator=g).bfloat16().cuda()
    mapping = torch.tensor([9, 2, -1, 30, 0, 17, 5], dtype=torch.int32, device="cuda")
    buf = torch.randn(31, L + R, generator=g).bfloat16().cuda()
    want = buf.clone()
    live = mapping >= 0
    want[mapping[live].long(), :L] = lat[live, 0]
    want[mapping[live].long(), L:] = rope[live, 0]
    copy_latent_to_cache(lat, rope, mapping, buf[:, :L], buf[:, L:])
    torch.cuda.synchronize()
    assert torch.equal(buf, want)
