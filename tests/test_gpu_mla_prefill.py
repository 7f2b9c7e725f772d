"""GPU: MLA latent-cache prefill (svk_mla_gather_latent, run_mla_prefill over the head_dim 256 attention kernel) against
index_select, float64 causal attention over the same bf16 K/V, and the latent-space decode of the chunk's last token."""

import pytest
import torch

pytestmark = pytest.mark.gpu

L, R, NOPE, DV, TOL = 512, 64, 192, 256, 2e-2


def ints(x):
    return torch.tensor(x, dtype=torch.int32, device="cuda")


def caches(pool, layout, seed):
    """latent / RoPE caches of unit-variance rows in either layout, plus the [pool, 576] rows they hold"""
    rows = torch.randn(pool, L + R, generator=torch.Generator().manual_seed(seed)).bfloat16().cuda()
    if layout == "interleaved":
        buf = rows.clone()
        return buf[:, :L], buf[:, L:], rows
    return rows[:, :L].contiguous().unsqueeze(1), rows[:, L:].contiguous().unsqueeze(1), rows


def slot_table(lens, pool, seed):
    """[B + 1, max len + 2] table of distinct slots (row 0 unused), request rows walked backwards"""
    B, W = len(lens), max(lens) + 2
    perm = torch.randperm(pool, generator=torch.Generator().manual_seed(seed))[: (B + 1) * W].to(torch.int32)
    return perm.view(B + 1, W).cuda(), ints([B - i for i in range(B)])


def kv_b_proj(H, seed):
    """bf16 [H * 448, 512], unit gain: per head 192 key rows | 256 value rows"""
    return (torch.randn(H * (NOPE + DV), L, generator=torch.Generator().manual_seed(seed)) / L ** 0.5).bfloat16().cuda()


@pytest.mark.parametrize("layout", ["split", "interleaved"])
def test_gather_is_index_select(layout):
    from sparse_vllm_amd.kernels import gather_latent_history
    lens, pool, n = [70, 0, 1, 33], 400, 104
    lat, rope, rows = caches(pool, layout, 1)
    table, req = slot_table(lens, pool, 2)
    table[req[0], 5] = pool                                     # outside the pool: a zero row
    out_lat = torch.full((n + 3, L), 9.0, dtype=torch.bfloat16, device="cuda")
    out_rope = torch.full((n + 3, R), 9.0, dtype=torch.bfloat16, device="cuda")
    gather_latent_history(lat, rope, table, req, ints(lens), ints([0, 70, 70, 71]), out_lat, out_rope, max_context_len=70)
    torch.cuda.synchronize()
    ids = torch.cat([table[req[i], :n_i] for i, n_i in enumerate(lens)]).long()
    want = rows.index_select(0, ids.clamp(max=pool - 1))
    want[5] = 0
    assert torch.equal(out_lat[:n], want[:, :L]) and torch.equal(out_rope[:n], want[:, L:])
    assert bool((out_lat[n:] == 9.0).all()) and bool((out_rope[n:] == 9.0).all())


@pytest.mark.parametrize("H", [1, 5])
def test_run_mla_prefill_matches_float64(H):
    from sparse_vllm_amd.kernels import run_mla_prefill
    contexts, chunks, pool = [150, 47], [50, 47], 500            # a cached prefix of 100, and a fresh prompt
    lat, rope, rows = caches(pool, "interleaved", 3)
    table, req = slot_table(contexts, pool, 4)
    w = kv_b_proj(H, 5)
    q = torch.randn(sum(chunks), H, NOPE + R, generator=torch.Generator().manual_seed(6)).bfloat16().cuda()
    out = torch.full((sum(chunks), H, DV), 3.0, dtype=torch.bfloat16, device="cuda")
    run_mla_prefill(q, lat, rope, table, req, ints(contexts), ints([0, chunks[0]]), ints(chunks), lambda x: x @ w.T, out)
    torch.cuda.synchronize()
    seen = rows.index_select(0, torch.cat([table[req[i], :n] for i, n in enumerate(contexts)]).long())
    expanded = (seen[:, :L].contiguous() @ w.T).view(-1, H, NOPE + DV)      # the same GEMM call
    k = torch.cat([expanded[..., :NOPE], seen[:, None, L:].expand(-1, H, -1)], dim=-1).cpu().double()
    v, qd, want, ko, qo = expanded[..., NOPE:].cpu().double(), q.cpu().double(), [], 0, 0
    for n, c in zip(contexts, chunks):                                      # float64 causal attention, scale 256^-1/2
        s = torch.einsum("qhd,khd->hqk", qd[qo:qo + c], k[ko:ko + n]) / 16.0
        mask = torch.arange(c)[:, None] + (n - c) >= torch.arange(n)[None, :]
        p = torch.softmax(s.masked_fill(~mask, float("-inf")), dim=-1)
        want.append(torch.einsum("hqk,khd->qhd", p, v[ko:ko + n]))
        ko, qo = ko + n, qo + c
    err = (out.cpu().double() - (want := torch.cat(want))).abs()
    print(f"H={H}: max error {err.max().item():.3e}")
    assert bool((err <= TOL + TOL * want.abs()).all())


def test_prefill_agrees_with_the_latent_space_decode_of_the_last_token():
    """A chunk stored by copy_latent_to_cache and prefilled, against run_mla_decode of its last token through the
    absorbed weights (q_latent = q_nope W_uk, output = W_uv o_latent): same scale (256^-1/2), same RoPE placement.
    Bound: the sum of the two paths' bounds, 2 x (2e-2 + 2e-2 |x|); the decode bound holds per latent element and W_uv
    has unit-norm rows of independent signs, so it carries over to the projected values as a root-mean-square bound."""
    from sparse_vllm_amd.kernels import allocate_mla_decode_workspace, copy_latent_to_cache, run_mla_decode, run_mla_prefill
    H, prefix, chunk, pool, n = 5, 37, 20, 128, 57
    lat, rope, _ = caches(pool, "split", 7)
    table, req = slot_table([n], pool, 8)
    new = torch.randn(chunk, L + R, generator=torch.Generator().manual_seed(9)).bfloat16().cuda()
    copy_latent_to_cache(new[:, None, :L].contiguous(), new[:, None, L:].contiguous(), table[req[0], prefix:n].contiguous(),
                         lat, rope)
    w = kv_b_proj(H, 10)
    q = torch.randn(chunk, H, NOPE + R, generator=torch.Generator().manual_seed(11)).bfloat16().cuda()
    out = torch.empty((chunk, H, DV), dtype=torch.bfloat16, device="cuda")
    run_mla_prefill(q, lat, rope, table, req, ints([n]), ints([0]), ints([chunk]), lambda x: x @ w.T, out)
    wh = w.view(H, NOPE + DV, L).double()
    q_lat = torch.einsum("hn,hnl->hl", q[-1, :, :NOPE].double(), wh[:, :NOPE]).bfloat16()[None].contiguous()
    ws = allocate_mla_decode_workspace(1, H, n, "cuda", block_seq=32)
    o_lat = torch.empty((1, H, L), dtype=torch.bfloat16, device="cuda")
    run_mla_decode(q_lat, q[-1:, :, NOPE:].contiguous(), lat, rope, table, req, ints([n]), o_lat, ws,
                   softmax_scale=1.0 / 16.0, max_context_len=n)
    torch.cuda.synchronize()
    via_decode = torch.einsum("hvl,hl->hv", wh[:, NOPE:], o_lat[0].double()).cpu()
    err = (out[-1].cpu().double() - via_decode).abs()
    print(f"max |prefill - decode| = {err.max().item():.3e}")
    assert bool((err <= 2 * (TOL + TOL * via_decode.abs())).all())
