"""A 256-wide GQA model (4 / 2 heads x 256), vanilla: one prefill chunk, then decode steps through `Attention.forward` with
the `mi355x_hip_gqa` provider, eager and in a hipGraph, against the oracle chained over a mirror of the slot state
(the shape of tests/test_gpu_vanilla_e2e.py): outputs rtol = atol = 2e-2, slot state and cache contents bit-exact."""

import numpy as np
import pytest

from oracle import bf16_round, decode_attention as oda, h2o as oh

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
_f = lambda t: t.float().cpu().numpy()


@pytest.mark.parametrize("graph", [False, True])
def test_vanilla_d256_prefill_then_decode_matches_oracle(graph):
    from sparse_vllm_amd.config import Config
    from sparse_vllm_amd.engine.sequence import Sequence
    from tools.synthetic import SyntheticDecodeDriver
    L, Hq, Hkv, D, prompts, steps = 2, 4, 2, 256, (150, 40), 4
    conf = Config.from_kwargs(sparse_method="vanilla", num_hidden_layers=L, num_attention_heads=Hq, num_key_value_heads=Hkv,
                              head_dim=D, max_model_len=256, max_num_seqs_in_gpu=3, num_kvcache_slots=512,
                              engine_prefill_chunk_size=256)
    drv = SyntheticDecodeDriver(conf)
    cm = drv.cache_manager
    assert drv.attn.decode_launch_op.name == "mi355x_hip_gqa"
    cm.permute_free_slots(5)
    seqs = [Sequence(num_prompt_tokens=n) for n in prompts]
    st = oh.SlotState(cm.buffer_req_to_token_slots_tensor.cpu().numpy().copy(), cm.free_slots_stack_tensor.cpu().numpy().copy(),
                      np.asarray(cm._num_free_slots, dtype=np.int64), np.stack(cm.row_seq_lens).astype(np.int32))
    kc, vc = _f(cm.kv_cache[0]).copy(), _f(cm.kv_cache[1]).copy()

    def check_state():
        np.testing.assert_array_equal(np.stack(cm.row_seq_lens), st.row_len)
        np.testing.assert_array_equal(np.asarray(cm._num_free_slots), st.free_ptr)
        np.testing.assert_array_equal(cm.buffer_req_to_token_slots_tensor.cpu().numpy(), st.slot_table)
        np.testing.assert_array_equal(_f(cm.kv_cache[0]), kc)            # prefill store and fused decode store: exact copies
        np.testing.assert_array_equal(_f(cm.kv_cache[1]), vc)

    g = torch.Generator().manual_seed(11)
    mk = lambda h: (torch.randn(L, sum(prompts), h, D, generator=g) * 0.4).to(torch.bfloat16).to(drv.device)
    for s in seqs:
        s.current_chunk_size = s.num_prompt_tokens
    q, k, v = mk(Hq), mk(Hkv), mk(Hkv)
    drv.prefill_chunk(seqs, q, k, v, outputs=torch.zeros_like(q))
    torch.cuda.synchronize()
    rows = [cm.seq_id_to_row[0][s.seq_id] for s in seqs]
    for l in range(L):
        for r, n, s0 in zip(rows, prompts, (0, prompts[0])):
            new = oh.allocate(st, l, r, n)
            kc[l][new], vc[l][new] = _f(k[l, s0:s0 + n]), _f(v[l, s0:s0 + n])
    check_state()
    for s in seqs:
        s.num_tokens = s.num_prompt_tokens
    drv.seqs = seqs
    if graph:
        drv.enable_decode_graph()
    outs = torch.zeros((L, len(seqs), Hq, D), dtype=torch.bfloat16, device=drv.device)
    for step in range(steps):
        q, k, v = drv.random_step_inputs(seed=100 + step, scale=0.4)
        drv.step(q, k, v, outputs=outs)
        torch.cuda.synchronize()
        new_slots = oh.decode_allocate_batch_layers(st, range(L), rows)
        lens = np.array([st.row_len[0, r] for r in rows], dtype=np.int32)
        for l in range(L):
            kc[l][new_slots[l]], vc[l][new_slots[l]] = _f(k[l]), _f(v[l])
            mid, lse = oda.flash_decode_stage1(_f(q[l]), kc[l], vc[l], st.slot_table[l], np.array(rows, np.int32), lens,
                                               int(lens.max()), 256)
            np.testing.assert_allclose(_f(outs[l]), bf16_round(oda.flash_decode_stage2(mid, lse, lens, 256)), rtol=2e-2, atol=2e-2)
        check_state()
