#!/usr/bin/env python3
"""R-KV redundancy micro-benchmark (development tool, GPU only): svk_rkv_redundancy over `rows` windows of `n` tokens,
Qwen2.5-7B keys (4 KV heads x 128), randomly permuted paged K.  The launch is captured in a hipGraph over `--pools`
rotating K pools (so a replay does not find the previous replay's keys in the caches) and replayed.
FLOPs counted = 2 n^2 Hkv D per row (the full similarity matrix, as the torch form computes it); the bound is the dense
bf16 MFMA peak (2.5 PFLOP/s).  Where the [rows, n, n] temporaries fit, the torch form of the same formulas
(include/svk.h, SvkRkvRedundancyArgs) is timed on the same GPU."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from sparse_vllm_amd.kernels.rkv_ops import RkvWorkspace, redundancy_scores_from_slots


def torch_form(keys, thr, keep):
    """keys bf16 [rows, n, Hkv, D] -> f32 [rows, n]"""
    rows, n = keys.shape[:2]
    f = torch.nn.functional.normalize(keys.float().reshape(rows, n, -1), p=2, dim=-1, eps=1e-6)
    sim = torch.bmm(f, f.transpose(1, 2))
    sim.diagonal(dim1=1, dim2=2).zero_()
    if thr > 0:
        sim = torch.where(sim >= thr, sim, torch.zeros_like(sim))
    if keep > 0 and n > 1:
        high = (sim > 0) & torch.ones((n, n), dtype=torch.bool, device=keys.device).triu(1)
        rank = high.flip(2).to(torch.int32).cumsum(2).flip(2)
        sim = sim.masked_fill(high & (rank <= keep), 0.0)
    return torch.softmax(sim.mean(dim=2), dim=1)


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="512,2048,4096")
    ap.add_argument("--rows", default="1,28,256")
    ap.add_argument("--pools", type=int, default=4)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--torch-bytes", type=float, default=24e9, help="largest torch-form temporary footprint to attempt")
    args = ap.parse_args()
    from _warm import warm
    warm()                                  # clocks settled before the first timed configuration (tools/_warm.py)
    d = torch.device("cuda:0")
    Hkv, D, thr, keep = 4, 128, 0.8, 1
    torch.manual_seed(0)
    ws = RkvWorkspace()
    for n in [int(x) for x in args.n.split(",")]:
        for rows in [int(x) for x in args.rows.split(",")]:
            slots = rows * n + 1024
            pools = [(torch.randn(slots, Hkv, D, device=d) * 0.3).bfloat16() for _ in range(args.pools)]
            table = torch.randperm(slots, device=d)[: rows * n].to(torch.int32).view(rows, n)
            out = torch.empty((rows, n), dtype=torch.float32, device=d)

            def run_all():
                for k in pools:
                    redundancy_scores_from_slots(k, table, similarity_threshold=thr, recent_similar_keep=keep, max_tokens=n,
                                                 out=out, workspace=ws)
            run_all()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                run_all()
            us = timed(graph.replay, args.iters) / args.pools
            flops = 2.0 * n * n * Hkv * D * rows
            line = (f"rkv_redundancy n={n:5d} rows={rows:4d}: {us:9.1f} us  {flops / us / 1e6:7.1f} TFLOP/s "
                    f"({flops / us / 1e6 / 2500 * 100:4.1f}% of 2.5 PF dense bf16)")
            if rows * n * n * 14.0 <= args.torch_bytes:          # f32 sim + where copy + int32 ranks + masks
                keys = pools[0][table.long()]
                redundancy_scores_from_slots(pools[0], table, similarity_threshold=thr, recent_similar_keep=keep, max_tokens=n,
                                             out=out, workspace=ws)
                ref = torch_form(keys, thr, keep)
                t_us = timed(lambda: torch_form(keys, thr, keep), max(2, args.iters // 2))
                err = ((out - ref).abs() / ref).max().item()
                line += f"  torch form {t_us:10.1f} us = {t_us / us:6.1f}x  (max rel diff {err:.1e})"
            else:
                line += "  torch form: temporaries do not fit"
            print(line, flush=True)
            del pools, graph


if __name__ == "__main__":
    main()
