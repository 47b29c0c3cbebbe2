#!/usr/bin/env python3
"""Time the native flow loss (rcf_amd.unFlowLoss, csrc/unflow.hip) against the same loss composed from torch ops on the device
(models/amd/flow_loss.py + loss_blocks.py + utils/warp_utils.py restated in plain torch, float32, with torch autograd), in one
process.

The workload's own shape: 8 frame pairs of 384 x 640, a five-level pyramid, the configuration of models/fcn_head.py:73-85 (L1 + SSIM
with a 3 x 3 window, masks from the backward flow, both directions, the last level's weight 0).  Per weighted level, both
directions, on the same area-resized frames and the same level-0 masks: forward alone, and forward + backward to the flow
(gradients cleared before every call) of the native pair of autograd Functions and of the composition; and the forward of the
existing unfused route (ops.flow_warp + ops.photometric_loss, which stores the warped frame and has no gradient).  Then the whole
module against the whole composition.  Native and composition are ALTERNATED, `--reps` repetitions each; every repetition is a
window of device events around `--iters` / `--torch-iters` calls, after a warm-up of both.  "faster beyond the spread": the slowest
native repetition is faster than the fastest composition repetition.

Algorithmic bytes of one direction of a level: three image planes, two flow planes, one mask plane and three gathered planes of
the other frame, 4 B h w each; the backward reads them again and stores two planes of dflow.  Their rate is printed as a fraction of
STREAM_TBS, the streaming rate profiles/ records for this box class (4.6 TB/s: the lower end of the 4.6 - 6.0 TB/s of the
streaming kernels in profiles/correlation_time.txt and LABNOTES 4.4).  Writes the table to --out (default profiles/unflow_time.txt)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import rcf_amd  # noqa: E402
from rcf_amd import ops  # noqa: E402
from rcf_amd.unflow_loss import _PhotoFn  # noqa: E402

B, H, W, LEVELS = 8, 384, 640, 5
STREAM_TBS = 4.6


class Cfg(dict):
    __getattr__ = dict.__getitem__


CFG = Cfg(alpha=10, ssim_sz=1, occ_from_back=True, type="unflow", w_l1=0.15, w_scales=[1.0, 1.0, 1.0, 1.0, 0.0],
          w_sm_scales=[1.0, 0.0, 0.0, 0.0, 0.0], w_real_smooth=0., w_ssim=0.85, w_ternary=0.0, warp_pad="border", with_bk=True)


# ------------------------------------------------------------------------------------------ the composition, plain torch
def t_flow_warp(x, flow):
    b, _, h, w = x.shape
    xs = torch.arange(w, device=x.device, dtype=x.dtype).view(1, 1, w).expand(b, h, w)
    ys = torch.arange(h, device=x.device, dtype=x.dtype).view(1, h, 1).expand(b, h, w)
    gx = 2.0 * (xs + flow[:, 0]) / (w - 1) - 1.0
    gy = 2.0 * (ys + flow[:, 1]) / (h - 1) - 1.0
    return F.grid_sample(x, torch.stack([gx, gy], 3), mode="bilinear", padding_mode="border", align_corners=True)


def t_ssim(x, y, md):
    k = 2 * md + 1
    pool = lambda a: F.avg_pool2d(a, k, 1, 0)
    mx, my = pool(x), pool(y)
    sx, sy, sxy = pool(x * x) - mx * mx, pool(y * y) - my * my, pool(x * y) - mx * my
    n = (2 * mx * my + 0.01 ** 2) * (2 * sxy + 0.03 ** 2)
    d = (mx * mx + my * my + 0.01 ** 2) * (sx + sy + 0.03 ** 2)
    return torch.clamp((1 - n / d) / 2, 0, 1)


def t_photo(im, other, flow, occ, cfg):
    rec = t_flow_warp(other, flow)
    loss = cfg.w_l1 * ((im - rec).abs() * occ).mean() + cfg.w_ssim * t_ssim(rec * occ, im * occ, cfg.ssim_sz).mean()
    return loss / occ.mean()


def t_level(flow, im1, im2, occ1, occ2, cfg):
    return (t_photo(im1, im2, flow[:, :2], occ1, cfg) + t_photo(im2, im1, flow[:, 2:], occ2, cfg)) / 2.


def t_module(flows, target, cfg):
    total = 0
    for i, flow in enumerate(flows):
        if cfg.w_scales[i] == 0:
            continue
        h, w = flow.shape[2:]
        im1, im2 = F.interpolate(target[:, :3], (h, w), mode="area"), F.interpolate(target[:, 3:], (h, w), mode="area")
        if i == 0:
            with torch.no_grad():
                m1, m2 = 1 - ops.occu_mask_backward(flow[:, 2:]), 1 - ops.occu_mask_backward(flow[:, :2])
            o1, o2 = m1, m2
        else:
            o1, o2 = F.interpolate(m1, (h, w), mode="nearest"), F.interpolate(m2, (h, w), mode="nearest")
        total = total + t_level(flow, im1, im2, o1, o2, cfg) * cfg.w_scales[i]
    return total


# ------------------------------------------------------------------------------------------------------------ the native
def n_level(flow, im1, im2, m1, m2, cfg):
    wts = (cfg.ssim_sz, cfg.w_l1, cfg.w_ssim, cfg.w_ternary)
    return (_PhotoFn.apply(flow[:, :2], im1, im2, m1, *wts) + _PhotoFn.apply(flow[:, 2:], im2, im1, m2, *wts)) / 2.


def unfused_level(flow, im1, im2, o1, o2, cfg):
    a = ops.photometric_loss(im1, ops.flow_warp(im2, flow[:, :2]), o1, cfg.w_l1, cfg.w_ssim)
    b = ops.photometric_loss(im2, ops.flow_warp(im1, flow[:, 2:]), o2, cfg.w_l1, cfg.w_ssim)
    return (a + b) / 2.


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3           # microseconds per call


def inputs(dev, b, h, w, levels):
    g = torch.Generator().manual_seed(384640)
    y, x = torch.arange(h).float()[:, None], torch.arange(w).float()[None, :]
    ph = 6.283 * torch.rand(b, 6, 1, 1, generator=g)
    target = (0.5 + 0.3 * torch.sin(0.05 * x + 0.03 * y + ph) + 0.04 * torch.randn(b, 6, h, w, generator=g)).clamp(0, 1)
    ph = 6.283 * torch.rand(b, 4, 1, 1, generator=g)
    full = 3.0 * torch.sin(0.011 * x + 0.017 * y + ph) + 0.2 * torch.randn(b, 4, h, w, generator=g)
    flows = [(F.interpolate(full, (h >> l, w >> l), mode="bilinear", align_corners=False) / 2 ** l if l else full).contiguous()
             for l in range(levels)]
    return [f.to(dev).requires_grad_(True) for f in flows], target.to(dev)


def measure(legs, args, lines):
    """legs: name -> (native callable, composition callable or None, bytes or None)"""
    out = {}
    for leg, (kern, comp, nbytes) in legs.items():
        for _ in range(3):
            kern()
            if comp:
                comp()
        torch.cuda.synchronize()
        tk, tc = [], []
        for _ in range(args.reps):
            tk.append(window(kern, args.iters))
            if comp:
                tc.append(window(comp, args.torch_iters))
        tk.sort()
        tc.sort()
        mk = tk[len(tk) // 2]
        line = f"  {leg:28s}: native {mk:9.1f} [{tk[0]:9.1f} .. {tk[-1]:9.1f}]"
        if comp:
            mc = tc[len(tc) // 2]
            verdict = "native faster beyond the spread" if tk[-1] < tc[0] else "NOT faster beyond the spread"
            line += f"   composition {mc:9.1f} [{tc[0]:9.1f} .. {tc[-1]:9.1f}]   ratio {mc / mk:6.1f}x   {verdict}"
            out[leg] = tk[-1] < tc[0]
        if nbytes:
            rate = nbytes / (mk * 1e-6) / 1e12
            line += f"\n  {'':28s}  algorithmic bytes {nbytes / 1e6:.2f} MB -> {rate:.2f} TB/s = {rate / STREAM_TBS:.2f} of the {STREAM_TBS} TB/s streaming rate"
        lines.append(line)
        print(line, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--torch-iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--size", type=int, nargs=3, default=[B, H, W], metavar=("B", "H", "W"))
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "unflow_time.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_unflow.py measures on the GPU; there is none here")
    dev = "cuda:0"
    b, h, w = args.size
    flows, target = inputs(dev, b, h, w, LEVELS)
    mod = rcf_amd.unFlowLoss(CFG)
    lines = [f"unFlowLoss, {b} pairs of {h} x {w}, {LEVELS} levels, FCNHead configuration (L1 + SSIM 3 x 3, both directions), float32; "
             f"{torch.cuda.get_device_name(0)}; microseconds per call, median [min .. max] of {args.reps} alternated repetitions "
             f"({args.iters} native / {args.torch_iters} composition calls each)"]
    with torch.no_grad():
        m1, m2 = 1 - ops.occu_mask_backward(flows[0][:, 2:]), 1 - ops.occu_mask_backward(flows[0][:, :2])
    verdicts = {}
    for i, flow in enumerate(flows):
        if CFG.w_scales[i] == 0:
            continue
        lh, lw = flow.shape[2:]
        im1, im2 = ops.area_resize(target[:, :3], (lh, lw)), ops.area_resize(target[:, 3:], (lh, lw))
        o1, o2 = F.interpolate(m1, (lh, lw), mode="nearest"), F.interpolate(m2, (lh, lw), mode="nearest")

        def train(f):
            flow.grad = None
            f().backward()

        def fwd(f):
            with torch.no_grad():
                f()
        nat = lambda: n_level(flow, im1, im2, m1, m2, CFG)
        comp = lambda: t_level(flow, im1, im2, o1, o2, CFG)
        train(nat)
        gn, ln = flow.grad.clone(), float(nat().detach())
        train(comp)
        lc = float(comp().detach())
        diff, top = (gn - flow.grad).abs(), float(gn.abs().max())
        # the composition's sample position is rounded differently (torch's division on the device): where that moves a position
        # across an integer the two take different bilinear cells -- a few elements, not an error of either
        lines.append(f"level {i}, {lh} x {lw}: loss native {ln:.6f} composition {lc:.6f}; dflow: max |g| {top:.1e}, median abs difference "
                     f"{float(diff.median()):.1e}, max {float(diff.max()):.1e}, share of elements over 1e-3 max |g| {float((diff > 1e-3 * top).float().mean()):.1e}")
        print(lines[-1], flush=True)
        fb = 2 * 9 * 4 * b * lh * lw                       # both directions
        got = measure({"forward": (lambda: fwd(nat), lambda: fwd(comp), fb),
                       "forward + backward": (lambda: train(nat), lambda: train(comp), 2 * fb + 2 * 2 * 4 * b * lh * lw),
                       "forward, unfused warp + loss": (lambda: fwd(lambda: unfused_level(flow, im1, im2, o1, o2, CFG)), None, None)}, args, lines)
        verdicts[i] = got["forward + backward"]

    def train_all(f):
        for fl in flows:
            fl.grad = None
        f().backward()
    measure({"module forward": (lambda: torch.no_grad()(lambda: mod(flows, target))(), lambda: torch.no_grad()(lambda: t_module(flows, target, CFG))(), None),
             "module forward + backward": (lambda: train_all(lambda: mod(flows, target)[0]), lambda: train_all(lambda: t_module(flows, target, CFG)), None)},
            args, lines)
    slow = [i for i, ok in verdicts.items() if not ok]
    lines.append("native forward + backward faster than the composition beyond the spread at every weighted level" if not slow else
                 f"native forward + backward NOT faster beyond the spread at level(s) {slow}")
    text = "\n".join(lines) + "\n"
    print(lines[-1])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
