"""CPU: the launch plans of the conv entry points -- which kernel family a forward / data gradient takes, the split-K factor of
both weight gradients, the sizes of the workspaces -- are pure host functions of the shape, its operand pointers and its flags.
This test pins them against tests/golden/conv_plans.json (tests/golden/README.md: recorded from the commit BEFORE the launch
plumbing of the fp32 and 16-bit paths was folded), so that a refactor of that plumbing cannot move a plan unnoticed.  A change
that moves one on purpose (a new cost model, a new tile rule) records the table again and says so.

    python tests/test_conv_plan_cpu.py --record        # rewrites the table from the library built in this tree
"""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import rcf_amd  # noqa: E402,F401
from rcf_amd import _lib  # noqa: E402

TABLE = os.path.join(ROOT, "tests", "golden", "conv_plans.json")


def out_size(n, k, stride, pad, dil):
    return (n + 2 * pad - dil * (k - 1) - 1) // stride + 1


def model_convs(N, H, W):
    """(N, H, W, Cin, Cout, k, stride, pad, dil) of every conv of the stage-1 model (config.stage1_model_kwargs: ResNet-50 with
    strides 1,2,1,1 / dilations 1,1,2,4 / contract_dilation, and the two FCN heads) on N frames of H x W; the stem's 3 input
    channels padded to 4 (fp32 step) and to 8 (16-bit steps)"""
    convs = [(N, H, W, 4, 64, 7, 2, 3, 1), (N, H, W, 8, 64, 7, 2, 3, 1)]
    h, w = out_size(out_size(H, 7, 2, 3, 1), 3, 2, 1, 1), out_size(out_size(W, 7, 2, 3, 1), 3, 2, 1, 1)
    h0, w0 = h, w
    inplanes = 64
    for planes, blocks, stride, dil in ((64, 3, 1, 1), (128, 4, 2, 1), (256, 6, 1, 2), (512, 3, 1, 4)):
        for b in range(blocks):
            s = stride if b == 0 else 1
            d = dil // 2 if (b == 0 and dil > 1) else dil
            convs.append((N, h, w, inplanes, planes, 1, 1, 0, 1))
            convs.append((N, h, w, planes, planes, 3, s, d, d))
            if b == 0:
                convs.append((N, h, w, inplanes, planes * 4, 1, s, 0, 1))
            h, w = out_size(h, 3, s, d, d), out_size(w, 3, s, d, d)
            convs.append((N, h, w, planes, planes * 4, 1, 1, 0, 1))
            inplanes = planes * 4
    for (hh, ww, cin, ncls) in ((h0, w0, 256 + 2048, 4), (h, w, 4096, 16)):       # decode_head2 (resize_concat), decode_head3
        convs += [(N, hh, ww, cin, 256, 3, 1, 6, 6), (N, hh, ww, 256, 256, 3, 1, 6, 6), (N, hh, ww, 256, ncls, 1, 1, 0, 1)]
    return convs


def fuzz_convs(seed, ncases=60):
    """the shapes (and regions) tools/fuzz_conv.py draws: its generator lines, in its order"""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(ncases):
        Cin = int(rng.choice([32, 64, 96, 128, 192, 256, 320, 512]))
        Cout = int(rng.choice([32, 64, 72, 128, 136, 256, 512]))
        k = int(rng.choice([1, 3]))
        stride = int(rng.choice([1, 1, 2]))
        dil = int(rng.choice([1, 2, 3])) if k == 3 else 1
        pad = dil * (k // 2)
        N, H, W = int(rng.randint(1, 4)), int(rng.randint(6, 40)), int(rng.randint(6, 40))
        Ho, Wo = out_size(H, k, stride, pad, dil), out_size(W, k, stride, pad, dil)
        reg = None
        if stride == 1 and rng.rand() < 0.4 and Ho >= 6 and Wo >= 6:
            rh, rw = int(rng.randint(3, Ho + 1)), int(rng.randint(3, Wo + 1))
            y0, x0 = int(rng.randint(0, Ho - rh + 1)), int(rng.randint(0, Wo - rw + 1))
            t = int(rng.randint(1, min(rh, rw) // 2)) if min(rh, rw) >= 4 and rng.rand() < 0.5 else 0
            reg = (y0, x0, rh, rw, t)
        out.append(((N, H, W, Cin, Cout, k, stride, pad, dil), reg))
    return out


def cases():
    """[(label, ConvShape fields N..y_pitch, struct size or None = the right one, drawn region or None)]"""
    def fields(c):
        N, H, W, Cin, Cout, k, stride, pad, dil = c
        return (N, H, W, Cin, out_size(H, k, stride, pad, dil), out_size(W, k, stride, pad, dil), Cout, k, k, stride, pad, dil, Cin, Cout)
    out = []
    for N, H, W in ((8, 480, 854), (16, 480, 854), (2, 64, 96)):
        for c in dict.fromkeys(model_convs(N, H, W)):
            out.append(("model " + " ".join(map(str, c)), fields(c), None, None))
    for seed in (0, 1, 2):
        for i, (c, reg) in enumerate(fuzz_convs(seed)):
            out.append((f"fuzz seed {seed} case {i} " + " ".join(map(str, c)), fields(c), None, reg))
    # the shapes tests/test_abi_cpu.py expects to be refused (and the good one it is built from)
    sz = ctypes.sizeof(_lib.ConvShape)
    good = (16, 120, 214, 64, 120, 214, 64, 3, 3, 1, 1, 1, 64, 64)
    out.append(("abi Cin % 4", (1, 8, 8, 3, 8, 8, 8, 3, 3, 1, 1, 1, 3, 8), None, None))
    out.append(("abi wrong Ho", (1, 8, 8, 4, 7, 8, 8, 3, 3, 1, 1, 1, 4, 8), None, None))
    out.append(("abi good", good, None, None))
    out.append(("abi short struct", good, sz - 8, None))
    out.append(("abi struct size 0", good, 0, None))
    return out


_DUMMY = ctypes.create_string_buffer(256)                     # never read: the queries launch nothing


def plan_row(lib, f, size, drawn):
    """the integers the library answers for one shape (see the module docstring)"""
    ptr = (ctypes.addressof(_DUMMY) + 15) & ~15
    H, W, Ho, Wo = f[1], f[2], f[4], f[5]

    def shape(prepared, flags):
        p = [ptr] * 7 + [None] if prepared else [None] * 8
        return ctypes.byref(_lib.ConvShape(*f, *p, flags, ctypes.sizeof(_lib.ConvShape) if size is None else size))

    def region(h, w, band):
        if h < 4 or w < 4:
            return None
        return ctypes.byref(_lib.ConvRegion(0, 0, h, w, 1) if band else _lib.ConvRegion(1, 1, h - 2, w - 2, 0))
    rdrawn = ctypes.byref(_lib.ConvRegion(*drawn)) if drawn is not None else None
    regs_out = [None, rdrawn if drawn is not None else region(Ho, Wo, 0), region(Ho, Wo, 1)]
    regs_in = [None, region(H, W, 0), region(H, W, 1)]
    row = []
    for prepared in (False, True):
        s = shape(prepared, 0)
        row += [lib.rcf_conv_kernel_of(s, r, 0) for r in regs_out] + [lib.rcf_conv_kernel_of(s, r, 1) for r in regs_in]
        row += [lib.rcf_conv2d_wgrad_region_workspace_bytes(s, r) for r in regs_out]
        row += [lib.rcf_conv2d_wgrad_bf16_workspace_bytes(s, r) for r in regs_out]
        row += [lib.rcf_conv2d_dgrad_workspace_bytes(s), lib.rcf_conv2d_dgrad_bnsums_ok(s), lib.rcf_conv2d_dgrad_bnsums_workspace_bytes(s),
                lib.rcf_conv2d_fwd_stats_workspace_bytes(s), lib.rcf_conv2d_fwd_stats_bf16_workspace_bytes(s),
                lib.rcf_conv2d_dgrad_masked_bf16_workspace_bytes(s)]
    s = shape(True, _lib.CONV_X_PLANES | _lib.CONV_DY_PLANES)
    row += [lib.rcf_conv_kernel_of(s, None, 0), lib.rcf_conv_kernel_of(s, None, 1), lib.rcf_conv2d_dgrad_bnsums_ok(s)]
    row += [lib.rcf_conv2d_wgrad_region_workspace_bytes(s, r) for r in regs_out[:2]]
    for flags in (_lib.CONV_H2P_NEVER, _lib.CONV_H2P_ALWAYS):
        s = shape(True, flags)
        row += [lib.rcf_conv_kernel_of(s, None, 0), lib.rcf_conv_kernel_of(s, None, 1)]
    s = shape(True, _lib.CONV_WGRAD_TILE_128)
    row += [lib.rcf_conv2d_wgrad_region_workspace_bytes(s, r) for r in regs_out[:2]]
    row += [lib.rcf_conv2d_wgrad_bf16_workspace_bytes(s, r) for r in regs_out[:2]]
    return [int(v) for v in row]


def plans():
    lib = _lib.load()
    return {label: plan_row(lib, f, size, drawn) for label, f, size, drawn in cases()}


def test_conv_launch_plans_match_the_recorded_table():
    want = json.load(open(TABLE))
    got = plans()
    assert sorted(got) == sorted(want), "the set of shapes changed: record the table again (module docstring) and say why"
    moved = [f"{k}: {want[k]} -> {got[k]}" for k in want if want[k] != got[k]]
    assert not moved, f"{len(moved)} launch plans moved, e.g. " + "; ".join(moved[:3])
    # the table discriminates: every kernel family, and split factors from none to hundreds, occur in it
    kinds = {v for row in want.values() for v in row[18:24]}
    assert {1, 2}.issubset(kinds) and 3 in {row[36] for row in want.values()}
    splits = {row[24] // (4 *int(k.split()[4]) * int(k.split()[5]) * int(k.split()[6]) ** 2) for k, row in want.items() if k.startswith("model")}
    assert 0 in splits and max(splits) > 100 and len(splits) > 8


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], __doc__
    with open(TABLE, "w") as fh:
        fh.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in plans().items()) + "\n}\n")
    print("wrote", TABLE)
