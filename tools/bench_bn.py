"""batch-norm launches on the step's three largest tensors: microseconds per call and TB/s of the bytes they must move.
One line per launch, `key<TAB>us<TAB>TB/s`, so that two builds' outputs can be laid side by side."""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
import rcf_amd
from rcf_amd import ops

DEV = "cuda:0"

def timeit(fn, n=200):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e-3

def line(key, t, nbytes=0):
    print(f"{key}\t{t * 1e6:.1f}\t{nbytes / t / 1e12:.2f}" if nbytes else f"{key}\t{t * 1e6:.1f}\t-", flush=True)

for dt in (torch.bfloat16, torch.float32):
    for (N, H, W, C) in [(16, 120, 214, 256), (16, 60, 107, 1024), (16, 60, 107, 512)]:
        tag = f"{str(dt)[6:]} [{N},{H},{W},{C}]"
        mk = lambda: torch.randn(N, H, W, C, device=DEV).to(dt)
        x, x2, res, dy = mk(), mk(), mk(), mk()
        mean = torch.zeros(C, device=DEV); invstd = torch.ones(C, device=DEV)
        g = torch.ones(C, device=DEV); b = torch.zeros(C, device=DEV)
        es = x.element_size(); n = x.numel(); rows = N * H * W
        mask = torch.empty(n // 4, dtype=torch.uint8, device=DEV)
        y = torch.empty_like(x)
        line(f"{tag} stats", timeit(lambda: ops.bn_stats(x)), n * es)
        line(f"{tag} apply", timeit(lambda: ops.bn_apply(x, mean, invstd, g, b, True, out=y, relu_mask=mask, out_dtype=dt)), 2 * n * es + n // 4)
        line(f"{tag} apply+res", timeit(lambda: ops.bn_apply(x, mean, invstd, g, b, True, residual=res, out=y, relu_mask=mask, out_dtype=dt)),
             3 * n * es + n // 4)
        line(f"{tag} bwd reduce", timeit(lambda: ops.bn_bwd_reduce(dy, x, y, mean, invstd, True, relu_mask=mask)), 2 * n * es + n // 4)
        s2 = ops.bn_bwd_reduce(dy, x, y, mean, invstd, True, relu_mask=mask)
        dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
        dx, dx2 = torch.empty_like(x), torch.empty_like(x)
        line(f"{tag} bwd apply", timeit(lambda: ops.bn_bwd_apply(dy, x, y, mean, invstd, g, True, s2, rows, dg, db, dx=dx, relu_mask=mask)),
             3 * n * es + n // 4)
        # the shared passes of a stage's first join and its downsample norm
        line(f"{tag} bwd reduce2", timeit(lambda: ops.bn_bwd_reduce2(dy, x, x2, mean, invstd, mean, invstd, mask)), 3 * n * es + n // 4)
        s4 = ops.bn_bwd_reduce2(dy, x, x2, mean, invstd, mean, invstd, mask)
        ap2 = lambda **kw: ops.bn_bwd_apply2(dy, x, mean, invstd, g, mask, s4[:2 * C], rows, dg, db, dx, x2, mean, invstd, g, s4[2 * C:],
                                             dg, db, dx2, **kw)
        line(f"{tag} bwd apply2", timeit(ap2), 5 * n * es + n // 4)
        if dt == torch.float32:
            # fp16 pair planes: the planes take the bytes of the fp32 tensor they replace
            ax, ag, bound, bound2 = ops.absmax(x), ops.absmax(dy), ops.new_amax(DEV), ops.new_amax(DEV)
            line(f"{tag} apply planes only", timeit(lambda: ops.bn_apply(x, mean, invstd, g, b, True, relu_mask=mask, amax_out=bound, planes=y,
                                                                          planes_only=True, amax_x=ax)), 2 * n * es + n // 4)
            line(f"{tag} bwd apply dx planes", timeit(lambda: ops.bn_bwd_apply(dy, x, None, mean, invstd, g, True, s2, rows, dg, db, dx=dx,
                                                                               relu_mask=mask, amax_out=bound, dx_planes=True, amax_x=ax, amax_dy=ag)),
                 3 * n * es + n // 4)
            line(f"{tag} bwd apply2 dx planes", timeit(lambda: ap2(amax_out=bound, amax_out2=bound2, dx_planes=True, amax_x=ax, amax_x2=ax, amax_dy=ag)),
                 5 * n * es + n // 4)

# the fused finalize (rcf_sum_partials_bn) behind a 1x1 64 -> 64 conv with 300 and 3210 row tiles of 128 pixels: the conv is the
# same code in every build of this library, what differs between two builds is the reduction of its partial rows
for tiles in (300, 3210):
    x = torch.randn(1, tiles, 128, 64, device=DEV)
    w = (torch.randn(64, 64, 1, 1, device=DEV) / 8).contiguous(memory_format=torch.channels_last)
    bn = torch.nn.BatchNorm2d(64).to(DEV)
    line(f"f32 conv 1x1 64->64 + fused finalize, {tiles} row tiles", timeit(lambda: ops.conv2d_fwd_stats(x, w, bn=bn)))
