"""H2O chunked prefill of a 256-wide model on the GPU: the accumulated token scores after the last chunk against the
oracle chain prefill_score_fwd -> accumulate_score, with the statistics from the attention launch and with the three-launch
form.  Budgets above the prompt: nothing is evicted and no selection is compared."""

import numpy as np
import pytest

from oracle import h2o as oh
from oracle import prefill_score as ops

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.mark.parametrize("fuse", ["0", "1"])
def test_h2o_prefill_scores_head_dim_256(monkeypatch, fuse):
    monkeypatch.setenv("SVK_PREFILL_SCORE_FUSE", fuse)
    from sparse_vllm_amd.config import Config
    from sparse_vllm_amd.engine.sequence import Sequence
    from tools.synthetic import SyntheticDecodeDriver
    Hq, Hkv, D, prompt, chunk, window = 8, 4, 256, 150, 64, 16
    conf = Config.from_kwargs(sparse_method="h2o", head_dim=D, num_attention_heads=Hq, num_key_value_heads=Hkv,
                              num_hidden_layers=1, max_model_len=512, max_num_seqs_in_gpu=2, num_kvcache_slots=400,
                              h2o_decode_budget=256, h2o_decode_eviction_interval=64, h2o_prefill_budget=256,
                              h2o_prefill_score_window=window, engine_prefill_chunk_size=chunk)
    drv = SyntheticDecodeDriver(conf)
    cm = drv.cache_manager
    cm.permute_free_slots(2)
    st = oh.SlotState(cm.buffer_req_to_token_slots_tensor.cpu().numpy().copy(), cm.free_slots_stack_tensor.cpu().numpy().copy(),
                      np.asarray(cm._num_free_slots, dtype=np.int64), np.stack(cm.row_seq_lens).astype(np.int32))
    kc = cm.kv_cache[0].float().cpu().numpy().copy()
    seq = Sequence(num_prompt_tokens=prompt)
    g = torch.Generator().manual_seed(1)
    score = None
    while seq.num_prefilled_tokens < prompt:
        n = seq.current_chunk_size = min(chunk, prompt - seq.num_prefilled_tokens)
        q, k, v = ((torch.randn(1, n, h, D, generator=g) * 0.4).to(torch.bfloat16).to(drv.device) for h in (Hq, Hkv, Hkv))
        drv.prefill_chunk([seq], q, k, v)
        row = cm.seq_id_to_row[0][seq.seq_id]
        prev = int(st.row_len[0, row])
        kc[0][oh.allocate(st, 0, row, n)] = k[0].float().cpu().numpy()
        ctx, cache = np.array([prev + n], np.int32), np.array([prev], np.int32)
        qs = np.maximum(cache, ctx - window).astype(np.int32)
        step = np.empty((1, prev + n), np.float32)
        ops.prefill_score_fwd(q[0].float().cpu().numpy(), kc[0], step, np.array([row], np.int32), np.zeros(1, np.int32), ctx,
                              cache, int((ctx - qs).max()), st.slot_table[0], qs, ctx)
        score = oh.accumulate_score(score, step[0], new_len=prev + n, weight=float(ctx[0] - qs[0]))
    got = cm.h2o_score_tensor[0, row].cpu().numpy()
    np.testing.assert_allclose(got[:prompt], score, rtol=2e-2, atol=2e-3)
    assert (got[prompt:] == 0).all()
