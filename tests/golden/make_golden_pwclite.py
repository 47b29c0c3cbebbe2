#!/usr/bin/env python3
"""Fixture for the flow network (rcf_amd.PWCLite): the REFERENCE's own module decides the numbers.

Loads utils/warp_utils.py, models/amd/correlation_native.py and models/amd/pwc_lite.py by file path under stand-in `utils`, `models`,
`models.amd` and `mmseg.ops` packages (`resize` is F.interpolate), builds the reference's PWCLite with the seeded weights of
tests/pwc_cases.py::draw_params (load_state_dict, strict), runs it and torch autograd on the CPU in float64 and in float32 on the
inputs of pwc_cases.draw_inputs, and stores in pwclite.npz -- only data, no reference text:
  names, shapes          the reference's state-dict names and shapes (shapes flattened, -1 between them)
per case k (pwc_cases.GOLDEN) and tensor t:
  out_k_<key>            the float64 output on pwc_cases.sample(n, OUT_BUDGET) of the flattened tensor; <key> as pwc_cases.output_items
  dmask_k_<i>            the float64 gradient of pwc_cases.functional with respect to mask[i], on sample(n, MASK_BUDGET)
  dparam_k_<j>           ... with respect to parameter j (state-dict order), on sample(n, GRAD_BUDGET, 1)
  e32_k, amax_k          per tensor, outputs then masks then parameters: max |float32 run - float64 run| and max |float64 run| over the
                         WHOLE tensor -- the reference's own float32 error is the yardstick of the GPU test
The weights (1.7 M floats) are not stored: the tests regenerate them from the seed.  The file has to stay under 200 KB, and float64
samples do not compress: every seventh element is kept while a tensor then takes at most its budget of samples, else the stride grows
(the finest outputs have 10^5 elements each, and there are forty-odd output tensors and forty-eight parameters).  Every e32 must be at most 1e-5 of its
tensor's range, and no LeakyReLU pre-activation of the float64 run may lie within pwc_cases.MIN_KINK_DISTANCE of zero relative to its
layer's range (a float32 run that decides one slope differently moves a bias gradient by 1e-4 of its range: the fixture pins
arithmetic, not ties -- as make_golden_unflow.py does for its masks); the seed is redrawn otherwise.

Regenerate, where a checkout of the reference exists:  python tests/golden/make_golden_pwclite.py <reference checkout>
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
import pwc_cases as pc  # noqa: E402

REF_FILES = [("utils.warp_utils", os.path.join("utils", "warp_utils.py")),
             ("models.amd.correlation_native", os.path.join("models", "amd", "correlation_native.py")),
             ("models.amd.pwc_lite", os.path.join("models", "amd", "pwc_lite.py"))]


def load_reference(root):
    for pkg in ("utils", "models", "models.amd", "mmseg", "mmseg.ops"):
        m = types.ModuleType(pkg)
        m.__path__ = []
        sys.modules[pkg] = m
    sys.modules["mmseg.ops"].resize = lambda x, size=None, mode="bilinear", align_corners=None, warning=False: \
        F.interpolate(x, size=size, mode=mode, align_corners=align_corners)
    mods = {}
    for name, rel in REF_FILES:
        spec = importlib.util.spec_from_file_location(name, os.path.join(root, rel))
        mods[name] = importlib.util.module_from_spec(spec)
        sys.modules[name] = mods[name]
        spec.loader.exec_module(mods[name])
    return mods["models.amd.pwc_lite"]


def run(ref, c, seed, dt):
    frames, masks = pc.draw_inputs(c, seed)
    net = ref.PWCLite(c.M).to(dt)
    net.load_state_dict({k: pc.T(v).to(dt) for k, v in pc.draw_params(seed).items()}, strict=True)
    m = [pc.T(masks[i]).to(dt).requires_grad_(True) for i in range(2)]
    res = net(pc.T(frames).to(dt), m, with_bk=True)
    res = {k: [t if torch.is_tensor(t) else torch.full_like(v[1], float(t)) for t in v] for k, v in res.items()}
    pc.functional(res, seed).backward()
    outs = [(k, t.detach().double()) for k, t in pc.output_items(res)]
    return outs, [t.grad.double() for t in m], [p.grad.double() for p in net.parameters()], [k for k, _ in net.named_parameters()]


def main():
    if len(sys.argv) != 2 or not all(os.path.isfile(os.path.join(sys.argv[1], rel)) for _, rel in REF_FILES):
        sys.exit("usage: make_golden_pwclite.py <reference checkout>   (a directory that holds " + ", ".join(r for _, r in REF_FILES) + ")")
    ref = load_reference(sys.argv[1])
    out = {}
    for k, c in enumerate(pc.GOLDEN):
        for attempt in range(200):
            seed = c.seed + attempt
            kink = pc.kink_distance(c, seed)
            if kink < pc.MIN_KINK_DISTANCE:
                print(c.name, "seed", seed, f"a pre-activation at {kink:.1e} of its layer's range -- redrawn")
                continue
            o64, m64, p64, names = run(ref, c, seed, torch.float64)
            o32, m32, p32, _ = run(ref, c, seed, torch.float32)
            t64 = [t for _, t in o64] + m64 + p64
            t32 = [t for _, t in o32] + m32 + p32
            e32 = np.asarray([float((a - b).abs().max()) for a, b in zip(t32, t64)])
            amax = np.asarray([float(b.abs().max()) for b in t64])
            rel = e32 / np.maximum(amax, 1e-300)
            if all(np.isfinite(e32)) and rel.max() <= 1e-5:
                break
            print(c.name, "seed", seed, "worst float32 error", rel.max(), "-- redrawn")
        else:
            sys.exit("no seed keeps the float32 run within 1e-5")
        assert seed == c.seed, f"put seed {seed} into pwc_cases.GOLDEN for case {c.name}"
        assert names == [n for n, _ in pc.param_shapes()]
        out["names"] = np.asarray(names)
        out["shapes"] = np.asarray(sum(([*p.shape, -1] for p in p64), []), dtype=np.int64)
        for key, t in o64:
            out[f"out_{k}_{key}"] = t.reshape(-1)[pc.sample(t.numel(), pc.OUT_BUDGET)].numpy()
        for i, t in enumerate(m64):
            out[f"dmask_{k}_{i}"] = t.reshape(-1)[pc.sample(t.numel(), pc.MASK_BUDGET)].numpy()
        for j, t in enumerate(p64):
            out[f"dparam_{k}_{j}"] = t.reshape(-1)[pc.sample(t.numel(), pc.GRAD_BUDGET, 1)].numpy()
        out[f"e32_{k}"], out[f"amax_{k}"] = e32, amax
        no, nm = len(o64), len(m64)
        flows = max(float(t.abs().max()) for key, t in o64 if "group" not in key)
        print(f"{c.name}: largest flow {flows:.2f} px; float32 run vs float64, relative to each tensor's range: outputs {rel[:no].max():.1e}, "
              f"mask gradients {rel[no:no + nm].max():.1e}, parameter gradients {rel[no + nm:].max():.1e}")
    path = os.path.join(HERE, "pwclite.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 200 * 1024


if __name__ == "__main__":
    main()
