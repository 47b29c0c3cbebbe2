#!/usr/bin/env python3
"""Time one training step of rcf_amd.AMDModel by its parts, and the three kernels of csrc/amd.hip against the torch compositions they
replace, in one process.

The workload: 8 pairs of 384 x 640 frames, the model of configs/amd/amd.yaml (M = 5, SyncBN on one rank, dropout 0.1), float32.
Parts, each a window of device events around `--iters` calls after a warm-up, medians of `--reps` repetitions:
  segmentation network forward / forward + backward (backbone2 + decode_head2 on the tape, a fixed logit gradient),
  the flow network (PWCLite forward + backward of its loss from fixed masks), the loss alone (unFlowLoss forward + backward from fixed
  flows), the whole step (forward, `.backward()`), and the three kernels.
Each kernel is ALTERNATED with the composition it replaces: ops.nhwc_to_nchw + F.softmax (+ the reshapes of flow_head.softmax_masks)
and its autograd, and the de-normalisation in torch ops + ops.resize_nchw.  "faster beyond the spread": the slowest native repetition
is faster than the fastest composition repetition.  Writes the table to --out (default profiles/amd_time.txt)."""
import argparse
import os
import sys
import types

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import amd_cases as ac  # noqa: E402
import rcf_amd  # noqa: E402
from rcf_amd import config, ops  # noqa: E402
from rcf_amd.layers import Tape  # noqa: E402
from time_pwclite import measure, window  # noqa: E402

B, H, W, M = 8, 384, 640, 5


def median(fn, args):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t = sorted(window(fn, args.iters) for _ in range(args.reps))
    return t[len(t) // 2], t[0], t[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--size", type=int, nargs=3, default=[B, H, W], metavar=("B", "H", "W"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "amd_time.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_amd.py measures on the GPU; there is none here")
    dev = "cuda:0"
    b, h, w = args.size
    margs = types.SimpleNamespace(checkpoints_dir="/tmp/rcf_amd_time", object_channel=None, eval_save=False, eval_export=False)
    model = rcf_amd.AMDModel(margs, **config.amd_model_kwargs(mask_layer=M))
    model.load_state_dict(ac.state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}))
    model = model.to(dev).train()
    g = torch.Generator().manual_seed(11)
    imgs = [(torch.rand(b, 3, h, w, generator=g) * 4 - 2).to(dev) for _ in range(2)]
    batch = {"imgs": imgs}
    stacked = torch.stack(imgs, dim=1)
    lines = [f"AMDModel (configs/amd/amd.yaml), {b} pairs of {h} x {w}, M = {M}, float32; {torch.cuda.get_device_name(0)}; microseconds per call, "
             f"median [min .. max] of {args.reps} repetitions ({args.iters} calls each)"]

    def note(name, t):
        lines.append(f"  {name:44s}: {t[0]:11.1f} [{t[1]:11.1f} .. {t[2]:11.1f}]")
        print(lines[-1], flush=True)

    def zero():
        for p in model.parameters():
            p.grad = None

    # ---- the parts of the step
    def seg_fwd(tape=None):
        t = tape if tape is not None else Tape(enabled=False)
        return model.decode_head2.fwd(model.backbone2.fwd(model._images_nhwc(stacked), t, model._dist()), t, model._dist())
    with torch.no_grad():
        lg0 = seg_fwd()
    hm, wm = lg0.t.shape[1:3]
    dlog = torch.randn(lg0.t.shape, generator=g).to(dev) * 1e-3

    def seg_step():
        zero()
        with torch.no_grad():
            tape = Tape()
            lg = seg_fwd(tape)
            lg.grad = dlog.clone()
            rcf_amd.model.grads_through_flat_buffer([p for p in model.parameters() if p.requires_grad], tape.backward)
    masks = [m.detach().requires_grad_(True) for m in ops.mask_softmax(lg0.t, b, 2, M)]
    head = model.decode_head

    def flow_step():
        zero()
        for m in masks:
            m.grad = None
        _, fl, _, _, _ = head.flow_forward(stacked, masks, need_whole=False)
        fl["seg"].backward()
    two = ops.frame_pair(stacked, head.flow_size)
    with torch.no_grad():
        res = head.flownet(two, masks, with_bk=True)
    flows = [torch.cat([a, c], 1).detach().requires_grad_(True) for a, c in zip(res["flows_fw"], res["flows_bw"])]

    def loss_step():
        for f in flows:
            f.grad = None
        head.loss_func(flows, two)[0].backward()

    def whole_step():
        zero()
        model(batch).backward()
    with torch.no_grad():
        note("segmentation network forward", median(lambda: seg_fwd(), args))
    note("segmentation network forward + backward", median(seg_step, args))
    note("flow network + loss, forward + backward", median(flow_step, args))
    note("loss alone (unFlowLoss), forward + backward", median(loss_step, args))
    note("whole step (forward, .backward())", median(whole_step, args))

    # ---- the three kernels against the compositions they replace
    logits = lg0.t
    dm = [torch.randn(b, M, hm, wm, generator=g).to(dev) for _ in range(2)]

    def nat_soft():
        return ops.mask_softmax(logits, b, 2, M)

    def comp_soft():
        l = ops.nhwc_to_nchw(logits, M)
        return F.softmax(l.view(b, 2, M, hm, wm), dim=2)
    pm = nat_soft()
    lead = logits[..., :M].detach().clone().requires_grad_(True)

    def nat_soft_bwd():
        return ops.mask_softmax_bwd(pm, dm, logits.shape[3])

    def comp_soft_bwd():
        lead.grad = None
        p = F.softmax(lead.permute(0, 3, 1, 2).reshape(b, 2, M, hm, wm), dim=2)
        torch.autograd.backward([p[:, 0], p[:, 1]], dm)
        return lead.grad
    std = torch.tensor(ac.STD, device=dev).view(1, 1, 3, 1, 1)
    mean = torch.tensor(ac.MEAN, device=dev).view(1, 1, 3, 1, 1)

    def nat_pair():
        return ops.frame_pair(stacked, head.flow_size)

    def comp_pair():
        return ops.resize_nchw(((stacked * std + mean) / 255.0).reshape(b, 6, h, w), head.flow_size, align_corners=True)
    d_soft = float((nat_soft().permute(1, 0, 2, 3, 4) - comp_soft()).abs().max())
    d_bwd = float((nat_soft_bwd()[..., :M] - comp_soft_bwd()).abs().max())
    d_pair = float((nat_pair() - comp_pair()).abs().max())
    lines.append(f"kernels vs compositions, max abs difference: softmax {d_soft:.1e}, its backward {d_bwd:.1e}, frame pair {d_pair:.1e}")
    print(lines[-1], flush=True)
    with torch.no_grad():
        got = measure({f"mask softmax forward ({2 * b} x {hm} x {wm} x {M})": (nat_soft, comp_soft),
                       f"frame pair ({b} x 6 x {head.flow_size[0]} x {head.flow_size[1]})": (nat_pair, comp_pair)}, args, lines)
    got.update(measure({"mask softmax backward": (nat_soft_bwd, comp_soft_bwd)}, args, lines))
    lines.append("new kernels faster than their compositions beyond the spread: " + str([k for k, v in got.items() if v]) +
                 "; not: " + str([k for k, v in got.items() if not v]))
    print(lines[-1])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
