#!/usr/bin/env python3
"""MLA decode micro-benchmark (development tool, GPU only): run_mla_decode (stage 1 + stage 2) over `batch` lanes of
`context` tokens with `heads` query heads, interleaved [slots, 576] latent cache, randomly permuted slots.  The call is
captured in a hipGraph over `--pools` rotating caches (so a replay does not find the previous replay's rows in the
caches) and replayed.  Bytes counted = sum of lengths x 1152 B + the f32 partials written and read + outputs; FLOPs =
2 H 1088 per token.  Where its temporaries fit, the same math in torch (index-gather of the rows, two bmm, softmax in
f32) is timed on the same GPU.  A 4096-token context stands for a selected-token view, the longer ones are dense."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from sparse_vllm_amd.kernels.mla import allocate_mla_decode_workspace, run_mla_decode

L, R = 512, 64


def torch_form(q, buf, table, scale):
    """q bf16 [B, H, 576], buf bf16 [slots, 576], table int64 [B, n] -> bf16 [B, H, 512]"""
    rows = buf[table]                                             # [B, n, 576]
    s = torch.bmm(q, rows.transpose(1, 2)).float() * scale
    p = torch.softmax(s, dim=-1).to(torch.bfloat16)
    return torch.bmm(p, rows[..., :L])


def timed(fn, iters):
    """(min, median) microseconds of `iters` separately timed calls"""
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
        ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    return ts[0], ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--heads", default="16,128")
    ap.add_argument("--context", default="4096,32768,131072")
    ap.add_argument("--batch", default="1,8,64")
    ap.add_argument("--pools", type=int, default=3)
    ap.add_argument("--iters", type=int, default=15, help="separately timed graph replays (min and median are reported)")
    ap.add_argument("--score", choices=["none", "headmax", "perhead"], default="none",
                    help="also emit token scores; headmax keeps all head tiles of a block in one workgroup")
    ap.add_argument("--pool-bytes", type=float, default=40e9, help="largest footprint of the rotating caches")
    ap.add_argument("--torch-bytes", type=float, default=40e9, help="largest torch-form temporary footprint to attempt")
    args = ap.parse_args()
    from _warm import warm
    warm()                                  # clocks settled before the first timed configuration (tools/_warm.py)
    d = torch.device("cuda:0")
    scale = 576 ** -0.5
    torch.manual_seed(0)
    for H in [int(x) for x in args.heads.split(",")]:
        for n in [int(x) for x in args.context.split(",")]:
            for B in [int(x) for x in args.batch.split(",")]:
                slots = B * n + 1024
                npools = max(1, min(args.pools, int(args.pool_bytes // (slots * 1152))))
                pools = [torch.randn(slots, L + R, device=d, dtype=torch.bfloat16) for _ in range(npools)]
                table = torch.randperm(slots, device=d)[: B * n].to(torch.int32).view(B, n)
                req = torch.arange(B, dtype=torch.int32, device=d)
                lens = torch.full((B,), n, dtype=torch.int32, device=d)
                q = torch.randn(B, H, L + R, device=d, dtype=torch.bfloat16)
                q_lat, q_rope = q[..., :L].contiguous(), q[..., L:].contiguous()
                out = torch.empty((B, H, L), dtype=torch.bfloat16, device=d)
                ws = allocate_mla_decode_workspace(B, H, n, d, headmax_scores=args.score == "headmax")
                score = {"none": None, "headmax": torch.empty((B, n), dtype=torch.float32, device=d)}.get(args.score)
                if args.score == "perhead":
                    score = torch.empty((B, H, n), dtype=torch.float32, device=d)

                def run_all():
                    for buf in pools:
                        run_mla_decode(q_lat, q_rope, buf[:, :L], buf[:, L:], table, req, lens, out, ws, softmax_scale=scale,
                                       attn_score=score)
                run_all()
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    run_all()
                us, us_med = (t / npools for t in timed(graph.replay, args.iters))
                nblk = ws.mid_output.shape[2]
                nbytes = B * n * 1152.0 + 2.0 * B * H * nblk * (L + 1) * 4 + B * H * L * 2
                flops = 2.0 * H * (2 * L + R) * B * n
                if score is not None:
                    nbytes += 2.0 * score.numel() * 4                      # the -1e20 fill and the score stores
                line = (f"mla_decode score={args.score} H={H:3d} ctx={n:6d} B={B:2d} block_seq={ws.block_seq:6d} pools={npools}: "
                        f"min {us:9.1f} us  median {us_med:9.1f} us  {nbytes / us_med / 1e6:5.2f} TB/s  "
                        f"{flops / us_med / 1e6:6.1f} TFLOP/s")
                if B * n * (1152.0 * 2 + H * 6.0) <= args.torch_bytes:     # gathered rows + their slice, f32 S + bf16 P
                    tl = table.long()
                    ref = torch_form(q, pools[-1], tl, scale)
                    err = (out.float() - ref.float()).abs().max().item()
                    _, t_us = timed(lambda: torch_form(q, pools[-1], tl, scale), max(3, args.iters // 3))
                    line += f"  torch form median {t_us:10.1f} us = {t_us / us_med:6.1f}x  (max abs diff {err:.1e})"
                    del ref
                else:
                    line += "  torch form: temporaries do not fit"
                print(line, flush=True)
                del pools, graph
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
