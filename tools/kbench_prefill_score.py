#!/usr/bin/env python3
"""prefill_score micro-benchmark (development tool, GPU only): the last `--window` queries of an 8 k chunk against
`--keys` compressed keys of one sequence, Qwen2.5-7B heads, randomly permuted paged K (W=128, Lc=16384 ->
2 x 15.0 GFLOP for the two Q.K^T passes of the probability mode, 15.0 for the logits mode).
FLOPs counted = 2 * W * Hq * Lc * D per Q.K^T pass; the bound is the dense bf16 MFMA peak (2.5 PFLOP/s).
`--head-dim 256 --heads 16/8` times the 256-wide kernels; `--final` adds the final pass alone on the statistics a prefill
attention launch left (`row_stats`); `--repeats N` times N windows of `--iters` calls and prints their median and minimum.
SVK_PREFILL_SCORE_VARIANT=1 in the environment selects the generic kernel at head_dim 256 (the A/B baseline)."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from sparse_vllm_amd.kernels.prefill_score import PrefillScoreWorkspace, prefill_score_fwd, prefill_score_window_pad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=int, default=128)
    ap.add_argument("--keys", default="16384,8192")
    ap.add_argument("--chunk", type=int, default=8192)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--head-dim", type=int, default=128)
    ap.add_argument("--heads", default="28/4", help="query heads / KV heads")
    ap.add_argument("--final", action="store_true", help="also time the final pass alone (row_stats from the attention launch)")
    ap.add_argument("--repeats", type=int, default=1)
    args = ap.parse_args()
    from _warm import warm
    warm()                                  # clocks settled before the first timed configuration (tools/_warm.py)
    d = torch.device("cuda:0")
    Hq, Hkv = (int(x) for x in args.heads.split("/"))
    D, W = args.head_dim, args.window
    torch.manual_seed(0)
    for Lc in [int(x) for x in args.keys.split(",")]:
        chunk = min(args.chunk, Lc)
        slots = Lc + 1024
        q = (torch.randn(chunk, Hq, D, device=d) * 0.3).bfloat16()
        k = (torch.randn(slots, Hkv, D, device=d) * 0.3).bfloat16()
        table = torch.randperm(slots, device=d)[:Lc].to(torch.int32).view(1, Lc)
        z = torch.zeros(1, dtype=torch.int32, device=d)
        seq = torch.tensor([Lc], dtype=torch.int32, device=d)
        pcl = torch.tensor([Lc - chunk], dtype=torch.int32, device=d)
        qs = torch.tensor([Lc - W], dtype=torch.int32, device=d)
        qe = torch.tensor([Lc], dtype=torch.int32, device=d)
        score = torch.zeros(1, Lc, dtype=torch.float32, device=d)
        ws = PrefillScoreWorkspace()
        modes = [("probability", 2, None), ("logits", 1, None)]
        if args.final:
            from sparse_vllm_amd.kernels.context_flashattention_nopad import context_attention_fwd
            wpad = prefill_score_window_pad(Hq, Hkv, W)
            stats = torch.zeros(Hq * wpad, dtype=torch.float32, device=d)
            context_attention_fwd(q, k, torch.randn_like(k), torch.empty_like(q), z, z, seq, pcl, chunk, table,
                                  score_stats=(stats, qs, wpad, score))
            modes.insert(1, ("probability", 1, stats))
        for mode, passes, stats in modes:
            def run():
                prefill_score_fwd(q, k, score, z, z, seq, pcl, W, table, qs, qe, candidate_start=0, num_recent_tokens=0,
                                  score_mode=mode, workspace=ws, row_stats=stats)
            for _ in range(3):
                run()
            torch.cuda.synchronize()
            times = []
            for _ in range(args.repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.iters):
                    run()
                e1.record()
                torch.cuda.synchronize()
                times.append(e0.elapsed_time(e1) * 1e3 / args.iters)
            us = statistics.median(times)
            flops = passes * 2.0 * W * Hq * Lc * D
            name = "final pass" if stats is not None else mode
            spread = f"  (min {min(times):.1f} us of {args.repeats})" if args.repeats > 1 else ""
            print(f"prefill_score {name:11s} W={W} keys={Lc:6d}: {us:8.1f} us  {flops / us / 1e6:7.1f} TFLOP/s "
                  f"({flops / us / 1e6 / 2500 * 100:4.1f}% of 2.5 PF dense bf16; {passes} Q.K^T pass{'es' if passes > 1 else ''}){spread}")


if __name__ == "__main__":
    main()
