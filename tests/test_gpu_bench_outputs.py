"""`bench.py`: a plain run reports the headline line alone, `--dump-outputs DIR` writes what the last timed step computed.

The benchmark's `main()` runs in this process at a small batch (2 sequences; context, budget, interval, layers
and heads are the headline's): one priming interval + 2 warm-up + 3 timed steps, twice with the same arguments."""

import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

STEPS, BATCH = 3, 2


def _run(monkeypatch, capsys, out_dir):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", str(STEPS), "--warmup", "2", "--batch", str(BATCH),
                                      "--dump-outputs", str(out_dir)])
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        monkeypatch.delenv(k, raising=False)
    capsys.readouterr()
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0]), {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}


def test_plain_line_and_dumped_outputs(monkeypatch, capsys, tmp_path):
    line, arrays = _run(monkeypatch, capsys, tmp_path / "a")
    _, again = _run(monkeypatch, capsys, tmp_path / "b")
    # the line of a plain run: the headline's keys, K timed steps, none of the legs that `--full` adds
    assert line["steps"] == STEPS and line["unit"] == "tokens/s" and line["higher_is_better"] is True and line["dtype"] == "bf16"
    assert line["ms_per_step"] > 0.0
    assert abs(line["value"] * line["ms_per_step"] * 1e-3 - BATCH) < 1e-6 * BATCH       # value = tokens of a step / its time
    assert not [k for k in ("burst", "roofline", "cpu_baseline", "paths", "e2e") if k in line]
    # the arrays: float32 / float64, within the size bound
    assert sorted(arrays) == ["attn_out", "h2o_scores", "row_len"]
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 * 2 ** 20
    # rows of 4096 tokens; the priming interval (130 steps) ends 2 steps after its burst at 4224, then 2 warm-up + 3 timed steps
    n = 4096 + 2 + 2 + STEPS
    assert arrays["row_len"].tolist() == [n] * BATCH
    assert arrays["attn_out"].shape == (28, BATCH, 28, 128) and arrays["h2o_scores"].shape == (28, BATCH, n)
    assert np.isfinite(arrays["attn_out"]).all() and np.abs(arrays["attn_out"]).max() > 0.0
    # cumulative scores are sums of softmax probabilities: finite, not negative; the newest token has this step's own
    scores = arrays["h2o_scores"]
    assert np.isfinite(scores).all() and scores.min() >= 0.0 and (scores[:, :, n - 1] > 0.0).all()
    # same arguments -> same inputs -> same outputs: the attention outputs to one bf16 ulp (2^-8 relative), the fp32 scores
    # to the rounding of a differently ordered sum
    np.testing.assert_array_equal(again["row_len"], arrays["row_len"])
    np.testing.assert_allclose(again["attn_out"], arrays["attn_out"], rtol=2.0 ** -7, atol=1e-6)
    np.testing.assert_allclose(again["h2o_scores"], arrays["h2o_scores"], rtol=1e-5, atol=1e-7)
