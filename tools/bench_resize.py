"""The bilinear resize kernels (csrc/spatial.hip) on the decode heads' tensors, [16,60,107,C] <-> [16,120,214,C]: one line per
kernel path, `key<TAB>us`, so that two builds' outputs can be laid side by side.  Per storage type and channel count: the
exact-2x kernels on the whole tensor (what the step runs), the general row-grid kernels on the same tensor (frame = -1), the
border-frame forms at the thickness layers.commuted_concat_conv passes for decode_head2 (forward; backward accumulating), and
the row-grid frame forms on a resize that is no exact 2x (119 x 213).  Last: the grid-stride fallbacks, which the step never
reaches, at the sweep's fb_up / fb_down shapes.  usage: python tools/bench_resize.py"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rcf_amd  # noqa
from rcf_amd import ops

DEV = "cuda:0"
D = 6                           # decode_head2's dilation (config.py)
BI = 2 * D + 1                  # layers.commuted_concat_conv: bi = bw + d, bw = d + 1


def timeit(fn, n=200):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e-3


def line(key, t):
    print(f"{key}\t{t * 1e6:.1f}", flush=True)


def pair(tag, N, small, large, C, dt, frame, beta=0):
    """forward small -> large and backward large -> small of one (shape, frame) choice; an accumulating backward adds zeros"""
    x = torch.randn(N, *small, C, device=DEV).to(dt)
    dy = torch.randn(N, *large, C, device=DEV).to(dt)
    if beta:
        dy.zero_()
    y, dx = torch.zeros_like(dy), torch.zeros_like(x)
    line(f"{tag} fwd", timeit(lambda: ops.resize_nhwc_fwd(x, large, False, out=y, frame=frame)))
    line(f"{tag} bwd" + (" beta=1" if beta else ""), timeit(lambda: ops.resize_nhwc_bwd(dy, small, False, out=dx, beta=beta, frame=frame)))


for dt in (torch.float32, torch.bfloat16):
    for C in (256, 512):
        tag = f"{str(dt)[6:]} C={C}"
        pair(f"{tag} 2x whole", 16, (60, 107), (120, 214), C, dt, 0)
        pair(f"{tag} rows whole (frame=-1)", 16, (60, 107), (120, 214), C, dt, -1)
        pair(f"{tag} 2x frame={BI}", 16, (60, 107), (120, 214), C, dt, BI, beta=1)
        pair(f"{tag} rows 119x213 frame={BI}", 16, (60, 107), (119, 213), C, dt, BI, beta=1)

# N * Ho > 65535 (forward), N * Hi > 65535 (backward): tests/spatial_cases.py fb_up, fb_down
x, y = torch.randn(8192, 3, 3, 4, device=DEV), torch.zeros(8192, 8, 8, 4, device=DEV)
line("float32 fallback fwd [8192,3,3,4] -> 8x8", timeit(lambda: ops.resize_nhwc_fwd(x, (8, 8), False, out=y)))
dy, dx = torch.randn(8192, 4, 4, 4, device=DEV), torch.zeros(8192, 8, 8, 4, device=DEV)
line("float32 fallback bwd [8192,4,4,4] -> 8x8", timeit(lambda: ops.resize_nhwc_bwd(dy, (8, 8), False, out=dx)))
