"""GPU parity of the head_dim 256 chunked-prefill attention (prefill_attention_d256.hip) through the public wrapper.
Tolerance rtol = atol = 2e-2, the bar of tests/test_gpu_prefill_attention.py; observed: docs/KERNELS.md (head_dim 256)."""

import numpy as np
import pytest

from oracle import bf16_bits_to_f32, bf16_round, f32_to_bf16_bits
from oracle import prefill_attention as opa

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOL, D, FILL = 2e-2, 256, 7.0


def t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def make_case(Hq, Hkv, chunks, pcs, *, perm_seed=0, extra_tokens=0, scale=0.5):
    """Seeded bf16 bit patterns.  The logical K/V rows depend on the shapes only; `perm_seed` moves them around in a pool
    with holes, through a slot table with padded rows that `req` walks in a shuffled order."""
    rng = np.random.default_rng(Hq * 1000 + Hkv * 10 + len(chunks))
    B, lens = len(chunks), [c + p for c, p in zip(chunks, pcs)]
    width, rows = max(lens) + 3, B + 2
    slots = rows * width + 11
    draw = lambda *shape: f32_to_bf16_bits((rng.standard_normal(shape) * scale).astype(np.float32))      # noqa: E731
    q, k_rows, v_rows = draw(sum(chunks) + extra_tokens, Hq, D), draw(rows * width, Hkv, D), draw(rows * width, Hkv, D)
    req = rng.permutation(rows)[:B].astype(np.int32)
    table = np.random.default_rng(100 + perm_seed).permutation(slots)[: rows * width].astype(np.int32)
    k = f32_to_bf16_bits(np.full((slots, Hkv, D), 3.0, np.float32))
    v = k.copy()
    k[table], v[table] = k_rows, v_rows
    start = np.concatenate(([0], np.cumsum(chunks)[:-1])).astype(np.int32)
    c = dict(q=q, k=k, v=v, req=req, start=start, seq_len=np.array(lens, np.int32), pcl=np.array(pcs, np.int32),
             table=table.reshape(rows, width))
    return {**c, "oracle": tuple(bf16_bits_to_f32(c[n]) for n in "qkv") + tuple(c[n] for n in list(c)[3:])}


def run(c, max_input_len, attn_score=None):
    from sparse_vllm_amd.kernels.context_flashattention_nopad import context_attention_fwd
    q, k, v = (t(c[n].view(np.int16)).view(torch.bfloat16) for n in "qkv")
    o = torch.full(q.shape, FILL, dtype=torch.bfloat16, device="cuda:0")
    context_attention_fwd(q, k, v, o, t(c["req"]), t(c["start"]), t(c["seq_len"]), t(c["pcl"]), int(max_input_len),
                          t(c["table"]), attn_score=attn_score)
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("Hq,Hkv,chunks,pcs", [
    (4, 4, [300, 33, 1], [200, 0, 64]),     # MHA as MLA expands it: several query blocks, the ring wraps, ragged prefixes
    (20, 20, [129], [7]),                   # one row past a 128-row block
    (8, 4, [70, 64], [5, 130]),             # G = 2: a wave's rows straddle two heads
    (8, 2, [40], [17]),                     # G = 4
])
def test_prefill_attention_d256_random(Hq, Hkv, chunks, pcs):
    c = make_case(Hq, Hkv, chunks, pcs)
    o = run(c, max(chunks)).float().cpu().numpy()
    dense = opa.context_attention_dense(*c["oracle"])
    ref = bf16_round(opa.context_attention_fwd(*c["oracle"]))
    print(f"Hq={Hq} Hkv={Hkv}: max |o - dense| = {np.abs(o - dense).max():.3e}, max |o - tiled| = {np.abs(o - ref).max():.3e}")
    np.testing.assert_allclose(o, dense, rtol=TOL, atol=TOL)
    np.testing.assert_allclose(o, ref, rtol=TOL, atol=TOL)


def test_rows_outside_the_chunks_keep_their_fill_value():
    """trailing tokens that belong to no sequence, and max_input_len larger than either chunk"""
    c = make_case(4, 2, [5, 150], [0, 40], extra_tokens=4)
    o = run(c, 300).float().cpu().numpy()
    assert (o[155:] == FILL).all()
    np.testing.assert_allclose(o[:155], opa.context_attention_dense(*c["oracle"])[:155], rtol=TOL, atol=TOL)


@pytest.mark.parametrize("dim", [3, 2])
def test_score_forms_are_reachable_at_d256(dim):
    """tolerances of the head_dim 128 score test's random case (fp32 sums in another order)"""
    c = make_case(8, 4, [200, 40], [150, 0], scale=0.4)
    shape, init = ((2, 8, 350), 0.0) if dim == 3 else ((2, 350), -1.0e20)
    got = torch.full(shape, init, dtype=torch.float32, device="cuda:0")
    o = run(c, 200, attn_score=got)
    ref = opa.context_attention_scores(c["oracle"][0], c["oracle"][1], *c["oracle"][3:], np.full(shape, init, np.float32))
    np.testing.assert_allclose(got.cpu().numpy(), ref, rtol=1e-4, atol=2e-3)
    assert torch.equal(o, run(c, 200))                  # the attention output does not depend on the score form


def test_output_is_independent_of_slot_placement():
    args = (8, 4, [70, 64], [5, 130])
    assert torch.equal(run(make_case(*args, perm_seed=0), 70), run(make_case(*args, perm_seed=1), 70))
