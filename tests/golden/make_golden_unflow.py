#!/usr/bin/env python3
"""Fixture for the flow loss (rcf_amd.unFlowLoss, csrc/unflow.hip): the REFERENCE's own module decides the numbers.

Loads utils/warp_utils.py, models/amd/loss_blocks.py and models/amd/flow_loss.py by file path under stand-in `utils`, `models` and
`models.amd` package objects (the real packages pull mmseg), runs the reference's `unFlowLoss` and torch autograd on the CPU in
float64 and in float32 and stores in unflow.npz -- only data, no reference text:
  target               float32 [2, 6, 32, 48], two smooth frames plus a little noise, values k / 255
  flow_l               float32 [2, 4, 32 >> l, 48 >> l], l = 0..4: smooth forward / backward flows of a few pixels, values k / 32 + 1 / 64
  names                the cases, tests/unflow_cases.py::golden_cfgs() (the configuration of models/fcn_head.py:73-85 and variants)
per case k:
  vals64_k, vals32_k   total_loss, warp_loss, smooth_loss, pyramid_flows[0].abs().mean() of the float64 / float32 run
  mask1_k, mask2_k     pyramid_occu_mask1[0] / pyramid_occu_mask2[0] (uint8; the float64 and float32 runs agree, asserted)
  g64_k_l, g32_k_l     the gradient of total_loss with respect to flow_l in float64 / of the float32 run, at every GOLDEN_STRIDE-th
                       element of the flattened tensor (a level of weight 0 has none)
The file has to stay under 200 KB: inputs are quantised so that they compress (the flows to an odd multiple of 1 / 64, so that no
sample position is an integer: the float64 and the float32 run then take the same bilinear taps), and the incompressible
gradients are kept on a subsample -- 7 divides none of the widths, the sample walks through all columns.  Every element is
covered by the float64 sweep of tests/unflow_cases.py; the fixture pins that the restatement IS the reference.

Masks must be decisions, not ties: the seed is redrawn until no level-0 splat count lies within 1e-4 of 0.2, no bidirectional
margin within 1e-4 of its threshold (the tie sets of tests/warp_cases.py), and every level's mask mean is above 0.05 (an
all-occluded coarse level makes the reference return NaN; that case belongs to the sweep).

Regenerate, where a checkout of the reference exists:  python tests/golden/make_golden_unflow.py <reference checkout>
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import unflow_cases as uc  # noqa: E402
import warp_cases as wc  # noqa: E402

REF_FILES = [("utils.warp_utils", os.path.join("utils", "warp_utils.py")),
             ("models.amd.loss_blocks", os.path.join("models", "amd", "loss_blocks.py")),
             ("models.amd.flow_loss", os.path.join("models", "amd", "flow_loss.py"))]
SEED = 9200


def load_reference(root):
    for pkg in ("utils", "models", "models.amd"):
        m = types.ModuleType(pkg)
        m.__path__ = []
        sys.modules[pkg] = m
    mods = {}
    for name, rel in REF_FILES:
        spec = importlib.util.spec_from_file_location(name, os.path.join(root, rel))
        mods[name] = importlib.util.module_from_spec(spec)
        sys.modules[name] = mods[name]
        spec.loader.exec_module(mods[name])
    return mods["utils.warp_utils"], mods["models.amd.flow_loss"]


def draw(seed):
    B, H, W = uc.GOLDEN_SHAPE
    g = torch.Generator().manual_seed(seed)
    a, b = uc.smooth_images(B, H, W, g)
    target = (np.round(np.concatenate([a, b], 1) * 255) / 255).astype(np.float32)
    f0 = wc.smooth_flow(B, H, W, g, amp_y=2.5)
    back, _ = wc.warp_ref(f0, f0, "zeros")
    b0 = (-back + 0.15 * torch.randn(B, 2, H, W, generator=g).numpy()).astype(np.float32)
    full = torch.from_numpy(np.concatenate([f0, b0], 1))
    flows = []
    for l in range(uc.GOLDEN_LEVELS):
        fl = F.interpolate(full, (H >> l, W >> l), mode="bilinear", align_corners=False) / (2 ** l) if l else full
        flows.append((np.floor(fl.numpy() * 32) / 32 + 1 / 64).astype(np.float32))
    return target, flows


def decided(wu, flows):
    """no tie in either mask rule at level 0, every level's mask mean above 0.05"""
    f = torch.from_numpy(flows[0]).double()
    B, _, H, W = f.shape
    ok = True
    for a, b in ((f[:, :2], f[:, 2:]), (f[:, 2:], f[:, :2])):
        cnt = wu.get_corresponding_map(wu.mesh_grid(B, H, W).type_as(b) + b).clamp(0, 1)
        ok &= bool(((cnt - 0.2).abs() > wc.TIE).all())
        w = wu.flow_warp(b, a, pad="zeros")
        lhs = ((a + w) ** 2).sum(1, keepdim=True)
        rhs = 0.01 * ((a * a).sum(1, keepdim=True) + (w * w).sum(1, keepdim=True)) + 0.5
        ok &= bool(((lhs - rhs).abs() > wc.TIE * (lhs + rhs)).all())
        for m in (1 - wu.get_occu_mask_backward(b), 1 - wu.get_occu_mask_bidirection(a, b)):
            ok &= all(float(F.interpolate(m, fl.shape[2:], mode="nearest").mean()) > 0.05 for fl in flows)
    return ok


def run(flow_loss, cfg, flows, target, dt):
    leaves = [torch.from_numpy(f).to(dt).requires_grad_(True) for f in flows]
    mod = flow_loss.unFlowLoss(cfg)
    out = mod(leaves, torch.from_numpy(target).to(dt))
    out[0].backward()
    vals = np.asarray([float(v.detach()) if torch.is_tensor(v) else float(v) for v in out], dtype=np.float64)
    assert np.isfinite(vals).all()
    return vals, mod.pyramid_occu_mask1[0].numpy(), mod.pyramid_occu_mask2[0].numpy(), [t.grad for t in leaves]


def main():
    if len(sys.argv) != 2 or not all(os.path.isfile(os.path.join(sys.argv[1], rel)) for _, rel in REF_FILES):
        sys.exit("usage: make_golden_unflow.py <reference checkout>   (a directory that holds " + ", ".join(r for _, r in REF_FILES) + ")")
    wu, flow_loss = load_reference(sys.argv[1])
    for attempt in range(500):
        target, flows = draw(SEED + attempt)
        if decided(wu, flows):
            break
    else:
        sys.exit("no seed gives decided masks")
    print("seed", SEED + attempt)
    out = {"target": target, "names": np.asarray([n for n, _, _ in uc.golden_cfgs()])}
    for l, f in enumerate(flows):
        out[f"flow_{l}"] = f
    for k, (name, cfg, levels) in enumerate(uc.golden_cfgs()):
        v64, m1, m2, g64 = run(flow_loss, cfg, flows[:levels], target, torch.float64)
        v32, n1, n2, g32 = run(flow_loss, cfg, flows[:levels], target, torch.float32)
        assert np.array_equal(m1, n1) and np.array_equal(m2, n2), "the float32 run decides a mask pixel differently"
        assert set(np.unique(m1)) <= {0.0, 1.0}
        out[f"vals64_{k}"], out[f"vals32_{k}"] = v64, v32
        out[f"mask1_{k}"], out[f"mask2_{k}"] = m1.astype(np.uint8), m2.astype(np.uint8)
        for l in range(levels):
            if cfg.w_scales[l] == 0:
                assert g64[l] is None or not g64[l].abs().sum()
                continue
            out[f"g64_{k}_{l}"] = g64[l].numpy().reshape(-1)[::uc.GOLDEN_STRIDE]
            out[f"g32_{k}_{l}"] = g32[l].numpy().reshape(-1)[::uc.GOLDEN_STRIDE]
        print(name, v64, "float32 run:", v32, "mask means", m1.mean(), m2.mean(), "max |grad| level 0", float(g64[0].abs().max()))
    path = os.path.join(HERE, "unflow.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 200 * 1024


if __name__ == "__main__":
    main()
