#!/usr/bin/env python3
"""Time the native cost volume (rcf_amd.Correlation, csrc/correlation.hip) against the reference's 81-slice composition
(models/amd/correlation_native.py restated in plain torch, with torch autograd) on the same device, in one process.

The five PWC-Lite pyramid levels of a 480 x 854 frame, 8 pairs, max_displacement 4.  Per level: forward alone, and forward plus
both gradients (module call + .backward(dout), the gradients cleared before every call, for both sides).  Kernel and composition
are ALTERNATED, three repetitions each; every repetition is a window of device events around `--iters` (kernel) / `--torch-iters`
(composition) calls, after a warm-up of both.  A level "wins" when the slowest kernel repetition is faster than the fastest
composition repetition, i.e. the margin exceeds the spread of the repetitions.  For the largest level the forward's algorithmic
bytes (x1 and x2 read once, the 81 planes written once) per second are printed, to hold against tools/hbm_ceiling.py on the same
box.  Writes the table to --out (default profiles/correlation_time.txt)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import rcf_amd  # noqa: E402

LEVELS = [(192, 8, 14), (128, 15, 27), (96, 30, 54), (64, 60, 107), (32, 120, 214)]      # C, H, W at 480 x 854
B, D_MAX = 8, 4


def composition(x1, x2, d=D_MAX):
    H, W = x1.shape[2:]
    x2 = F.pad(x2, [d] * 4)
    cv = [torch.mean(x1 * x2[:, :, i:i + H, j:j + W], 1, keepdim=True) for i in range(2 * d + 1) for j in range(2 * d + 1)]
    return torch.cat(cv, 1)


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3           # microseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--torch-iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "correlation_time.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_correlation.py measures on the GPU; there is none here")
    dev = "cuda:0"
    mod = rcf_amd.Correlation(D_MAX)
    lines = [f"cost volume, {B} pairs, max_displacement {D_MAX}, float32; {torch.cuda.get_device_name(0)}; microseconds per call, "
             f"median [min .. max] of {args.reps} alternated repetitions ({args.iters} kernel / {args.torch_iters} composition calls each)"]
    for C, H, W in LEVELS:
        g = torch.Generator().manual_seed(C)
        x1 = torch.randn(B, C, H, W, generator=g).to(dev).requires_grad_(True)
        x2 = torch.randn(B, C, H, W, generator=g).to(dev).requires_grad_(True)
        dout = torch.randn(B, (2 * D_MAX + 1) ** 2, H, W, generator=g).to(dev)

        def train(f):
            x1.grad = x2.grad = None
            f(x1, x2).backward(dout)

        def fwd(f):
            with torch.no_grad():
                f(x1, x2)
        legs = {"forward": (lambda: fwd(mod), lambda: fwd(composition)), "forward + backward": (lambda: train(mod), lambda: train(composition))}
        train(mod)
        k_out, k1, k2 = mod(x1, x2).detach(), x1.grad.clone(), x2.grad.clone()
        train(composition)
        diff = [float((a - b).abs().max()) for a, b in ((k_out, composition(x1, x2).detach()), (k1, x1.grad), (k2, x2.grad))]
        lines.append(f"level {C} ch @ {H} x {W}: max abs difference kernel - composition: out {diff[0]:.1e} dx1 {diff[1]:.1e} dx2 {diff[2]:.1e}")
        for leg, (kern, comp) in legs.items():
            for _ in range(3):
                kern()
                comp()
            torch.cuda.synchronize()
            tk, tc = [], []
            for _ in range(args.reps):
                tk.append(window(kern, args.iters))
                tc.append(window(comp, args.torch_iters))
            tk.sort()
            tc.sort()
            mk, mc = tk[len(tk) // 2], tc[len(tc) // 2]
            verdict = "kernel faster beyond the spread" if tk[-1] < tc[0] else "NOT faster beyond the spread"
            line = (f"  {leg:18s}: kernel {mk:9.1f} [{tk[0]:9.1f} .. {tk[-1]:9.1f}]   composition {mc:9.1f} [{tc[0]:9.1f} .. {tc[-1]:9.1f}]   "
                    f"ratio {mc / mk:6.1f}x   {verdict}")
            if leg == "forward" and (C, H, W) == LEVELS[-1]:
                nbytes = 4 * B * H * W * (2 * C + (2 * D_MAX + 1) ** 2)
                line += f"\n  {'':18s}  forward algorithmic bytes {nbytes / 1e6:.1f} MB -> {nbytes / (mk * 1e-6) / 1e12:.2f} TB/s"
            lines.append(line)
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
