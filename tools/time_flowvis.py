#!/usr/bin/env python3
"""Time the flow-colour pass of the training visualisation grids (ops.flow_color, csrc/flowvis.hip) against the reference's route,
and a logged training step against an unlogged one, in one process.

Shapes: 8 pairs at the RCF stage-1 mask size (120 x 214) with 4 and with 5 flow kinds (the affine head adds one), and 8 pairs of
96 x 160 with 2 kinds (AMDModel on 384 x 640 frames).  At each:
  the colour call     all 16 K flow images straight into the window of a grid canvas, one ops.flow_color call
  the reference route  restated (tests/flowvis_cases.reference_route): per image a clone, a blocking .cpu(), numpy's colour wheel
                       and the upload, then the concatenations and / 255 of rcf_model.py:562-575 -- 16 K round trips
  a whole step         model(batch) + backward with the grid written (a JPEG into a scratch `saved/`) against the same step
                       without (args.train_save = False); --no-steps skips this part
The two routes of a pair ALTERNATE in one process; microseconds per call, median [min .. max] of --reps repetitions of --iters
calls.  "faster beyond the spread": the slowest native repetition is faster than the fastest repetition of the other route.
Writes the table to --out (default profiles/flowvis_time.txt), and first the colour kernel's parity sweep against the float64
restatement -- differing elements per case, the worst share, the measured k -- to --parity-out (default profiles/flowvis_parity.txt)."""
import argparse
import copy
import os
import sys
import tempfile
import types

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import amd_cases as ac  # noqa: E402
import flowvis_cases as fc  # noqa: E402
import rcf_amd  # noqa: E402
from rcf_amd import config, flowvis, ops, synth  # noqa: E402
from time_pwclite import measure  # noqa: E402

PAIRS = 8


def colour_legs(h, w, K, dev, g):
    """(native, reference route) for 2 PAIRS grid rows of K flow images each"""
    N = 2 * PAIRS
    flows = (3.0 * torch.randn(N, K, 2, h, w, generator=g)).to(dev)
    panels = flowvis.grid_panels(5, [str(k) for k in range(K)])
    canvas = flowvis.new_canvas(2, PAIRS, panels, h, w, dev)
    window = canvas.view(N, 3, len(panels), h, w)[:, :, 6:6 + K].permute(0, 2, 1, 3, 4)

    def native():
        return ops.flow_color(flows, out=window)

    def reference():
        rows = []
        for n in range(N):
            cols = [fc.reference_route(flows[n, k][None], lambda a: torch.from_numpy(a).to(dev)) for k in range(K)]
            rows.append(torch.cat(cols, dim=2) / 255.0)
        return torch.cat(rows, 0)
    # the same picture, up to the rule of tests/flowvis_cases.py
    a = (native().reshape(N, K * 3, h, w) * 255).round().to(torch.uint8)
    b = (reference().view(N, 3, K, h, w).permute(0, 2, 1, 3, 4).reshape(N, K * 3, h, w) * 255).round().to(torch.uint8)
    differing = float((a != b).float().mean())
    assert differing <= fc.CAP and int((a.int() - b.int()).abs().max()) <= 1, differing
    return native, reference, differing


def step_legs(model, batch, backward):
    """(logged step, unlogged step): train_iter is put back to 0 before each, so that the step is due (log_interval is large: no
    .pth dump); args.train_save decides"""
    def run(save):
        model.args.train_save = save
        model.train_iter = 0
        for p in model.parameters():
            p.grad = None
        backward(model(batch))
    return (lambda: run(True)), (lambda: run(False))


def parity_lines(dev):
    """the sweep of tests/test_flowvis_gpu.py::test_color_parity as a table: per shape and value kind, elements whose byte differs
    from floor(level64), for the kernel and for the float32 numpy restatement; the measured k = the farthest differing element's
    distance from an integer level, in units of 2^-24 x 255"""
    one, tile = ops.flow_color_geometry()
    lines = [f"rcf_flow_color_f32 against the float64 restatement (tests/flowvis_cases.py); {torch.cuda.get_device_name(0)}; one-launch form up "
             f"to {one} pixels, {tile} pixels per workgroup above; rule: at most one level, only within EPS = {fc.K} x 2^-24 x 255 = {fc.EPS:.2e} "
             f"levels of an integer, at most {fc.CAP:.0e} of a case's elements",
             "differing elements per case, kernel | float32 numpy restatement (both: float32 up to radius and wheel position, fp64 tail):"]
    worst = dict(kernel=[0.0, 0.0, 0.0], numpy=[0.0, 0.0, 0.0])             # share, distance, step
    for shape in fc.BASE_SHAPES + fc.geometry_shapes(one):
        flows, levels = fc.batch(*shape)
        got = dict(kernel=ops.flow_color(torch.from_numpy(flows.copy()).to(dev)).cpu().numpy(),
                   numpy=np.stack([fc.to_bytes(fc.color_levels(f, head=np.float32)) for f in flows]))
        cells = []
        for i, kind in enumerate(fc.FINITE_KINDS):
            v = {k: fc.judge(g[i], levels[i]) for k, g in got.items()}
            assert all(x.ok for x in v.values()), (shape, kind, v)
            for k, x in v.items():
                worst[k] = [max(a, b) for a, b in zip(worst[k], (x.share, x.worst_distance, x.worst_step))]
            cells.append(f"{kind} {v['kernel'].differing}|{v['numpy'].differing}")
        lines.append(f"  {shape[0]:3d} x {shape[1]:4d} ({3 * shape[0] * shape[1]:6d} elements per image): " + "  ".join(cells))
    # a larger sample of the common case: 20 images of 96 x 160, 3 N(0, 1) flows scaled 1 .. 20 (one call)
    flows = np.concatenate([fc.batch(96, 160, kinds=("normal",), seed=i)[0] for i in range(20)]) * \
        np.arange(1, 21, dtype=np.float32).reshape(20, 1, 1, 1)
    levels = [fc.color_levels(f) for f in flows]
    got = dict(kernel=ops.flow_color(torch.from_numpy(flows).to(dev)).cpu().numpy(),
               numpy=np.stack([fc.to_bytes(fc.color_levels(f, head=np.float32)) for f in flows]))
    cells = []
    for k, g in got.items():
        vs = [fc.judge(a, lv) for a, lv in zip(g, levels)]
        assert all(v.ok for v in vs), (k, vs)
        worst[k] = [max(a, *b) for a, b in zip(worst[k], zip(*[(v.share, v.worst_distance, v.worst_step) for v in vs]))]
        cells.append(f"{k} {sum(v.differing for v in vs)} of {20 * 46080} (worst image {max(v.share for v in vs):.1e})")
    lines.append("  20 images of 96 x 160, 3 N(0, 1) scaled 1 .. 20, one call: " + "; ".join(cells))
    for k, (share, dist, step) in worst.items():
        lines.append(f"{k}: worst share of a case's elements differing {share:.2e} (cap {fc.CAP:.0e}); largest step {step:.0f} level; farthest differing "
                     f"element {dist:.2e} levels from an integer = measured k {dist / (2.0 ** -24 * 255.0):.3f} (derived bound k = {fc.K})")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-steps", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flowvis_time.txt"))
    ap.add_argument("--parity-out", default=os.path.join(ROOT, "profiles", "flowvis_parity.txt"),
                    help="also write the parity sweep of the colour kernel there ('' to skip)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_flowvis.py measures on the GPU; there is none here")
    dev = "cuda:0"
    if args.parity_out:
        with open(args.parity_out, "w") as f:
            f.write("\n".join(parity_lines(dev)) + "\n")
    g = torch.Generator().manual_seed(5)
    lines = [f"flow colours of the training grids, {PAIRS} pairs; {torch.cuda.get_device_name(0)}; microseconds per call, median [min .. max] of "
             f"{args.reps} repetitions ({args.iters} calls each), routes alternated; 'native' = the left column of each pair"]
    got = {}
    for h, w, K in ((120, 214, 4), (120, 214, 5), (96, 160, 2)):
        native, reference, differing = colour_legs(h, w, K, dev, g)
        lines.append(f"{2 * PAIRS} x {K} images of {h} x {w}: share of bytes differing between the routes {differing:.1e}")
        got.update(measure({f"colour call {h}x{w} K={K}": (native, reference)}, args, lines))
    if not args.no_steps:
        scratch = tempfile.mkdtemp(prefix="rcf_flowvis_time_")
        os.makedirs(os.path.join(scratch, "saved"))
        margs = lambda: types.SimpleNamespace(checkpoints_dir=scratch, object_channel=None, eval_save=False, eval_export=False)
        H, W = 480, 854
        nb = synth.make_batch(PAIRS, H, W, config_id=1)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        batch = {k: [t(a) for a in nb[k]] for k in ("imgs", "gt_fw_flows", "gt_bw_flows")}
        batch.update(seq_ids=nb["seq_ids"], seq_names=nb["seq_names"], paths=nb["paths"])
        for affine in (False, True):
            kw = config.stage1_model_kwargs(config.mask_size_for(H, W), affine=affine)
            kw.update(log_interval=10 ** 9)
            model = rcf_amd.RCFModel(margs(), **copy.deepcopy(kw)).to(dev).train()
            logged, plain = step_legs(model, batch, lambda losses: losses["loss"].backward())
            got.update(measure({f"RCF step {H}x{W} K={5 if affine else 4}": (plain, logged)}, args, lines))
            del model
        model = rcf_amd.AMDModel(margs(), **config.amd_model_kwargs(mask_layer=5, log_interval=10 ** 9))
        model.load_state_dict(ac.state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}))
        model = model.to(dev).train()
        imgs = [(torch.rand(PAIRS, 3, 384, 640, generator=g) * 4 - 2).to(dev) for _ in range(2)]
        abatch = dict(imgs=imgs, seq_ids=nb["seq_ids"], seq_names=nb["seq_names"], paths=nb["paths"])
        logged, plain = step_legs(model, abatch, lambda loss: loss.backward())
        got.update(measure({"AMD step 384x640 K=2": (plain, logged)}, args, lines))
        lines.append("step rows: 'native' column = the UNLOGGED step, 'composition' column = the logged one (grid + JPEG); the ratio is "
                     "what a logged step costs")
    lines.append("colour call faster than the reference's route beyond the spread: " +
                 str([k for k, v in got.items() if v and k.startswith("colour")]) + "; not: " +
                 str([k for k, v in got.items() if not v and k.startswith("colour")]))
    print(lines[-1])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
