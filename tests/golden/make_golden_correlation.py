#!/usr/bin/env python3
"""Fixture for the cost volume (rcf_amd.Correlation, csrc/correlation.hip): the REFERENCE's own module decides the numbers.

Loads models/amd/correlation_native.py by file path (the `models` package itself needs mmseg and flow_vis), runs its
`Correlation` and torch autograd on the CPU and stores, per case k of SHAPES, in correlation.npz:
  x1_k, x2_k, dout_k   float32 inputs (drawn here from SEED + k)
  out64_k, dx1_64_k, dx2_64_k   the float64 run: forward, and the gradients of (out * dout).sum()
  out32_k              the float32 forward
Only data; no reference text.

The file has to stay under 200 KB with 83 000 float64 results in it, so the inputs are made to compress: x1 and x2 are integers
in [-2, 2] and dout is C times an integer in [-2, 2].  Every product and sum of the float64 run is then exact -- out is S / C for
an integer S, the mean's backward turns dout / C back into the integer, the gradients are integers -- and zlib stores the
repeating values in a fraction of their size.  What the fixture pins is therefore the reference's INDEXING: padding, which
displacement lands in which plane, the direction of both gradients.  Rounding is the business of the float64 sweep
(tests/correlation_cases.py).

Regenerate, where a checkout of the reference exists:  python tests/golden/make_golden_correlation.py <reference checkout>
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF_FILE = os.path.join("models", "amd", "correlation_native.py")          # inside the reference checkout
SEED = 8100
SHAPES = [(2, 3, 1, 7, 4), (1, 5, 3, 3, 1), (1, 7, 4, 6, 2), (2, 33, 9, 11, 4), (1, 192, 8, 14, 4)]        # B, C, H, W, d


def main():
    if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], REF_FILE)):
        sys.exit(f"usage: make_golden_correlation.py <reference checkout>   (a directory that holds {REF_FILE})")
    spec = importlib.util.spec_from_file_location("correlation_native", os.path.join(sys.argv[1], REF_FILE))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    out = {"shapes": np.asarray(SHAPES, dtype=np.int64)}
    for k, (B, C, H, W, d) in enumerate(SHAPES):
        g = torch.Generator().manual_seed(SEED + k)
        D = 2 * d + 1
        x1 = torch.randint(-2, 3, (B, C, H, W), generator=g).float()
        x2 = torch.randint(-2, 3, (B, C, H, W), generator=g).float()
        dout = (C * torch.randint(-2, 3, (B, D * D, H, W), generator=g)).float()
        mod = ref.Correlation(max_displacement=d, kernel_size=1, stride1=1, stride2=1, corr_multiply=1)
        assert (mod.output_dim, mod.pad_size) == (D, d)
        a, b = x1.double().requires_grad_(True), x2.double().requires_grad_(True)
        o64 = mod(a, b)
        o64.backward(dout.double())
        o32 = mod(x1, x2)
        assert o64.shape == (B, D * D, H, W) and o32.dtype == torch.float32
        for name, t in (("x1", x1), ("x2", x2), ("dout", dout), ("out64", o64.detach()), ("dx1_64", a.grad), ("dx2_64", b.grad),
                        ("out32", o32)):
            out[f"{name}_{k}"] = t.numpy()
        print((B, C, H, W, d), "out", float(o64.detach().abs().max()), "dx1", float(a.grad.abs().max()), "dx2", float(b.grad.abs().max()))
    path = os.path.join(HERE, "correlation.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 200 * 1024


if __name__ == "__main__":
    main()
