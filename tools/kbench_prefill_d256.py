#!/usr/bin/env python3
"""head_dim 256 prefill attention micro-benchmark (development tool, GPU only): one chunk of `--chunk` query tokens of a
sequence with `--prefix` cached tokens, randomly permuted paged KV, for (a) 20-head MHA as MLA expands it and (b) 16
query / 8 KV heads.  The call is captured in a hipGraph over `--pools` rotating K/V pools (a replay does not find the
previous replay's rows in the caches) and replayed.  FLOPs = 4 * D * Hq * sum_i (prefix + i + 1).  Beside each line the
torch form on the same GPU: scaled_dot_product_attention over the gathered keys with the causal-with-prefix mask."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from sparse_vllm_amd.kernels.context_flashattention_nopad import context_attention_fwd

D = 256


def timed(fn, iters):
    """(min, median) milliseconds of `iters` separately timed calls"""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[0], ts[len(ts) // 2]


def torch_form(q, k, v, table, pc):
    """q [chunk, Hq, D], k / v [slots, Hkv, D], table int64 [L] -> [chunk, Hq, D]"""
    chunk, L, G = q.shape[0], table.shape[0], q.shape[1] // k.shape[1]
    kk = k[table].transpose(0, 1).repeat_interleave(G, dim=0)[None]
    vv = v[table].transpose(0, 1).repeat_interleave(G, dim=0)[None]
    keep = torch.arange(chunk, device=q.device)[:, None] + pc >= torch.arange(L, device=q.device)[None, :]
    return F.scaled_dot_product_attention(q.transpose(0, 1)[None], kk, vv, attn_mask=keep)[0].transpose(0, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunk", type=int, default=8192)
    ap.add_argument("--prefixes", default="0,8192,57344")
    ap.add_argument("--heads", default="20:20,16:8", help="Hq:Hkv pairs")
    ap.add_argument("--pools", type=int, default=3)
    ap.add_argument("--iters", type=int, default=7, help="separately timed graph replays (min and median are reported)")
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    from _warm import warm
    warm()                                  # clocks settled before the first timed configuration (tools/_warm.py)
    d = torch.device("cuda:0")
    torch.manual_seed(0)
    for Hq, Hkv in [tuple(int(x) for x in p.split(":")) for p in args.heads.split(",")]:
        for pc in [int(x) for x in args.prefixes.split(",")]:
            L = pc + args.chunk
            slots = L + 1024
            q = (torch.randn(args.chunk, Hq, D, device=d) * 0.3).bfloat16()
            pools = [((torch.randn(slots, Hkv, D, device=d) * 0.3).bfloat16(), (torch.randn(slots, Hkv, D, device=d) * 0.3).bfloat16())
                     for _ in range(args.pools)]
            o = torch.empty_like(q)
            table = torch.randperm(slots, device=d)[:L].to(torch.int32).view(1, L)
            z = torch.zeros(1, dtype=torch.int32, device=d)
            seq = torch.tensor([L], dtype=torch.int32, device=d)
            pcl = torch.tensor([pc], dtype=torch.int32, device=d)

            def run_all():
                for k, v in pools:
                    context_attention_fwd(q, k, v, o, z, z, seq, pcl, args.chunk, table)
            run_all()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                run_all()
            ms, ms_med = (t / args.pools for t in timed(graph.replay, args.iters))
            flops = 4.0 * D * Hq * (args.chunk * pc + args.chunk * (args.chunk + 1) / 2)
            line = (f"prefill attention d256 Hq={Hq} Hkv={Hkv} chunk={args.chunk} prefix={pc:6d}: min {ms:8.3f} ms  median "
                    f"{ms_med:8.3f} ms  {flops / ms_med / 1e9:7.1f} TFLOP/s ({flops / ms_med / 1e9 / 2500 * 100:4.1f}% of 2.5 PF dense bf16)")
            if not args.no_torch:
                k, v = pools[-1]
                tl = table[0].long()
                try:
                    ref = torch_form(q, k, v, tl, pc)
                    err = (o.float() - ref.float()).abs().max().item()
                    _, t_ms = timed(lambda: torch_form(q, k, v, tl, pc), 3)
                    line += f"  torch form median {t_ms:9.3f} ms = {t_ms / ms_med:5.2f}x  (max abs diff {err:.1e})"
                    del ref
                except torch.cuda.OutOfMemoryError:
                    line += "  torch form: temporaries do not fit"
            print(line, flush=True)
            del pools, graph
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
