#!/usr/bin/env python3
"""Time the native flow network (rcf_amd.PWCLite) against the same network composed from torch ops on the device
(tests/pwc_cases.py::net_ref, the vector-segment restatement of models/amd/pwc_lite.py, moved to the device in float32, with torch
autograd), in one process.

The workload's own shape: 8 frame pairs of 384 x 640, mask_layer of configs/amd/amd.yaml (5), masks at 96 x 160, both directions.
Forward alone, and forward + backward of a fixed linear functional to every parameter and both masks (gradients cleared before every
call).  Then, per level, the segment-pool path (ops.segment_pool -> the two predict_flow parameters on B M rows -> ops.segment_flow)
against the reference's form of it: per mask, the pooled 96-vector broadcast to a full map, two 1 x 1 convs over the map, and the
masked sum.  Native and composition are ALTERNATED, `--reps` repetitions each; every repetition is a window of device events around
`--iters` calls, after a warm-up of both.  "faster beyond the spread": the slowest native repetition is faster than the fastest
composition repetition.  With --launches the native step is also run once under the library's per-family event brackets and the
conv families' shares are printed.  Writes the table to --out (default profiles/pwclite_time.txt)."""
import argparse
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import pwc_cases as pc  # noqa: E402
import rcf_amd  # noqa: E402
from rcf_amd import ops  # noqa: E402

B, H, W, M = 8, 384, 640, 5


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3           # microseconds per call


def measure(legs, args, lines):
    out = {}
    for leg, (kern, comp) in legs.items():
        for _ in range(2):
            kern()
            comp()
        torch.cuda.synchronize()
        tk, tc = [], []
        for _ in range(args.reps):
            tk.append(window(kern, args.iters))
            tc.append(window(comp, args.iters))
        tk.sort()
        tc.sort()
        mk, mc = tk[len(tk) // 2], tc[len(tc) // 2]
        out[leg] = tk[-1] < tc[0]
        verdict = "native faster beyond the spread" if out[leg] else "NOT faster beyond the spread"
        lines.append(f"  {leg:34s}: native {mk:10.1f} [{tk[0]:10.1f} .. {tk[-1]:10.1f}]   composition {mc:10.1f} [{tc[0]:10.1f} .. {tc[-1]:10.1f}]   "
                     f"ratio {mc / mk:5.2f}x   {verdict}")
        print(lines[-1], flush=True)
    return out


def broadcast_form(p, feat, mask, group_sum):
    """the reference's segment path on a planar feature map: per mask, pool, broadcast, two 1 x 1 convs on the full map, masked sum"""
    e = "flow_estimators."
    b, c, h, w = feat.shape
    flow = 0
    for i in range(mask.shape[1]):
        mk = mask[:, i:i + 1]
        cur = ((feat * mk).view(b, c, -1).sum(2) / mk.view(b, 1, -1).sum(2)).view(b, c, 1, 1).repeat(1, 1, h, w)
        hid = F.leaky_relu(F.conv2d(cur, p[e + "predict_flow1.0.weight"], p[e + "predict_flow1.0.bias"]), pc.SLOPE)
        flow = flow + mk * (F.conv2d(hid, p[e + "predict_flow2.0.weight"], p[e + "predict_flow2.0.bias"]) + group_sum[:, i].view(b, 2, 1, 1))
    return flow


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--size", type=int, nargs=4, default=[B, H, W, M], metavar=("B", "H", "W", "M"))
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pwclite_time.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_pwclite.py measures on the GPU; there is none here")
    dev = "cuda:0"
    b, h, w, m = args.size
    case = pc.Case("workload", b, h, w, m, 384640)
    frames, masks = pc.draw_inputs(case)
    params = pc.draw_params(case.seed)
    x = torch.from_numpy(frames).to(dev)
    mk = [torch.from_numpy(masks[i]).to(dev).requires_grad_(True) for i in range(2)]
    net = rcf_amd.PWCLite(m).to(dev)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    p = {k: torch.from_numpy(v).to(dev).requires_grad_(True) for k, v in params.items()}
    lines = [f"PWCLite, {b} pairs of {h} x {w}, mask_layer {m}, masks at {h // 4} x {w // 4}, both directions, float32; {torch.cuda.get_device_name(0)}; "
             f"microseconds per call, median [min .. max] of {args.reps} alternated repetitions ({args.iters} calls each)"]

    def nat_fwd():
        with torch.no_grad():
            return net(x, mk)

    def comp_fwd():
        with torch.no_grad():
            return pc.net_ref(p, x, mk)

    # the seeded functional draws its weights on the host: build them once per leg instead
    wts = {}

    def functional(res, tag):
        items = pc.output_items(res)
        if tag not in wts:
            g = torch.Generator().manual_seed(5)
            wts[tag] = [torch.randn(t.shape[:2] + (1, 1), generator=g).to(dev) for _, t in items]
        return sum((wt * t).mean() for wt, (_, t) in zip(wts[tag], items))

    def nat_step():
        for t in list(net.parameters()) + mk:
            t.grad = None
        functional(net(x, mk), "n").backward()

    def comp_step():
        for t in list(p.values()) + mk:
            t.grad = None
        functional(pc.net_ref(p, x, mk), "c").backward()
    a, c = nat_fwd(), comp_fwd()
    worst = max(float((u - v).abs().max()) for (_, u), (_, v) in zip(pc.output_items(a), pc.output_items(c)))
    top = max(float(v.abs().max()) for k, v in pc.output_items(c) if "group" not in k)
    lines.append(f"outputs: native vs composition, max abs difference {worst:.2e} px at flows of up to {top:.2f} px")
    print(lines[-1], flush=True)
    got = measure({"forward": (nat_fwd, comp_fwd), "forward + backward": (nat_step, comp_step)}, args, lines)

    # the segment path of every level, on the estimator's feature slice of the workload's sizes
    g = torch.Generator().manual_seed(7)
    seg_ok = {}
    for l in range(5):
        lh, lw = h >> (6 - l), w >> (6 - l)
        buf = torch.randn(b, lh, lw, 448, generator=g).to(dev)
        feat = buf[..., 352:448]
        planar = feat.permute(0, 3, 1, 2).contiguous()
        mask_l = F.interpolate(mk[0].detach(), (lh, lw), mode="bilinear", align_corners=True).contiguous()
        acc = torch.randn(b, m, 2, generator=g).to(dev)
        est = net.flow_estimators

        def nat():
            with torch.no_grad():
                pooled, _ = ops.segment_pool(feat, mask_l)
                return ops.segment_flow(mask_l, est.segment_vectors(pooled) + acc)

        def comp():
            with torch.no_grad():
                return broadcast_form(p, planar, mask_l, acc)
        d = float((nat() - comp()).abs().max())
        r = measure({f"segment path, level {l} ({lh} x {lw}), diff {d:.1e}": (nat, comp)}, args, lines)
        seg_ok[l] = list(r.values())[0]
    if args.launches:
        fams = list(ops.CONV_FAMILIES)
        ops.PROFILE.start(fams)
        nat_step()
        rec = ops.PROFILE.stop()
        tot = sum(v["ms"] for v in rec.values())
        lines.append(f"conv launches of one native forward + backward, by kernel family (event brackets, {tot:.2f} ms in all): " +
                     ", ".join(f"{k} {v['launches']} launches {v['ms']:.2f} ms" for k, v in sorted(rec.items(), key=lambda kv: -kv[1]["ms"]) if v["launches"]))
        print(lines[-1], flush=True)
    lines.append(("native forward + backward faster than the composition beyond the spread" if got["forward + backward"] else
                  "native forward + backward NOT faster than the composition beyond the spread") +
                 "; segment path faster beyond the spread at levels " + str([l for l, ok in seg_ok.items() if ok]))
    print(lines[-1])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
