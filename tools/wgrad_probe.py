"""Times one weight-gradient launch alone (one stream, nothing beside it) for the training step's weight-gradient shapes: what the
planners' split-K choice costs per layer.
usage: python tools/wgrad_probe.py [--kind {h16,h2,planes}] [--half {bf16,fp16}] [--iters N] [--only TEXT]
  h16     16-bit operands (rcf_conv2d_wgrad_bf16; --half picks the library), the default
  h2      fp32 operands with their ranges (igemm_wgrad_h2t_kernel)
  planes  both operands as fp16 pair planes (igemm_wgrad_h2d_kernel)
(profiles/r05_wgrad_split_probe.txt holds a sweep over forced split counts taken with a temporary override)"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rcf_amd  # noqa
from rcf_amd import ops

ap = argparse.ArgumentParser()
ap.add_argument("--kind", choices=("h16", "h2", "planes"), default="h16")
ap.add_argument("--half", choices=("bf16", "fp16"), default="bf16")
ap.add_argument("--iters", type=int, default=20, help="timed launches per figure")
ap.add_argument("--only", default="", help="only the shapes whose 'Cin->Cout kK' label contains this text")
args = ap.parse_args()

dev = torch.device("cuda", 0)
# N, H, W, Cin, Cout, k, dilation, RCF_CONV_WGRAD_TILE_128 (the overlapped launches of the step take that tile)
shapes = [(16, 60, 107, 1024, 256, 1), (16, 60, 107, 2048, 512, 1), (16, 60, 107, 256, 1024, 1), (16, 60, 107, 512, 2048, 1),
          (16, 120, 214, 64, 64, 3), (16, 120, 214, 64, 256, 1), (16, 120, 214, 64, 64, 1), (16, 60, 107, 128, 512, 1),
          (16, 120, 214, 256, 64, 1), (16, 60, 107, 512, 128, 1), (16, 60, 107, 256, 256, 3), (16, 60, 107, 512, 512, 3),
          (16, 60, 107, 256, 256, 1), (16, 60, 107, 512, 512, 1)]
shapes = [s + (1, False) for s in shapes] + [(16, 120, 214, 256, 256, 3, 6, False), (16, 120, 214, 64, 64, 3, 1, True)]


def timeit(f, n=20):
    for _ in range(3):
        f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def to_planes(x, bound_bits):
    """fp32 [N,H,W,C] -> the fp32-typed buffer of its fp16 pair planes ([pixel][h | m]), scaled by 2^(14 - floor(log2(bound))).
    The tool's own, in fp32 on the device: a timing needs the layout, not tests/wgrad_cases.to_planes' float64 rounding, and a
    float64 copy of the step's largest tensors (16 x 120 x 214 x 256) is 0.8 GB each; tools do not import from tests/."""
    k = 14 - int(torch.floor(torch.log2(bound_bits.view(torch.float32))))
    t = x * 2.0 ** k
    h = t.to(torch.float16)
    m = (t - h.float()).to(torch.float16)
    return torch.stack([h, m], dim=3).contiguous().view(torch.float32).reshape(x.shape)


dt = torch.float16 if args.half == "fp16" else torch.bfloat16
print(f"kind {args.kind}" + (f" ({args.half})" if args.kind == "h16" else ""))
with ops.half_storage(dt):
    for (N, H, W, cin, cout, k, dil, tile128) in shapes:
        if (tile128 and args.kind != "h2") or args.only not in f"{cin}->{cout} k{k}":
            continue
        x = torch.randn(N, H, W, cin, device=dev)
        dy = torch.randn(N, H, W, cout, device=dev)
        dw = torch.zeros(cout, k, k, cin, device=dev).permute(0, 3, 1, 2)
        pad = dil * (k // 2)
        if args.kind == "h16":
            xh, dyh = x.to(dt), dy.to(dt)
            f = lambda: ops.conv2d_wgrad_bf16(xh, dyh, dw, dw, 1, pad, dil, beta=0)
        else:
            ax, ag = ops.absmax(x), ops.absmax(dy)
            if args.kind == "planes":
                x, dy = to_planes(x, ax), to_planes(dy, ag)
            f = lambda: ops.conv2d_wgrad(x, dy, dw, dw, 1, pad, dil, beta=0, amax=(ax, ag), small_tile=tile128, planes=args.kind == "planes")
        t = timeit(f, args.iters)
        flops = 2.0 * N * H * W * cin * cout * k * k
        byt = (2.0 if args.kind == "h16" else 4.0) * N * H * W * (cin + cout)
        passes = 1 if args.kind == "h16" else 3
        print(f"{cin}->{cout} k{k}{f' d{dil}' if dil > 1 else ''}{' tile128' if tile128 else ''} {N}x{H}x{W}: {t * 1e3:.1f} us  {flops / t / 1e9:.0f} TF/s  "
              f"(additive model {passes * flops / 1.1e15 * 1e6 + byt / 6e12 * 1e6:.1f} us)", flush=True)
