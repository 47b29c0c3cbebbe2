"""The tap-column weight-gradient kernels (csrc/wgrad_cols.h: igemm_wgrad_h2t_kernel, igemm_wgrad_h2d_kernel, wgrad_bf16_kernel,
wgrad_bf16_dma_kernel) bit for bit against a recorded build.

tests/test_kernels_gpu.py, test_planes_gpu.py, test_bf16_gpu.py and test_fp16_gpu.py hold these kernels to float64 and to each
other; a change that only moves their code must move NOTHING.  For every case of tests/wgrad_cases.py and every variant it has
(fp32 operands with ranges; the same with RCF_CONV_WGRAD_TILE_128; the same with RCF_CONV_NO_WGRAD_XCD; both operands as fp16
pair planes; 16-bit operands in each of the two libraries) this module takes the SHA-256 of the raw bytes of dw after
    beta = 0 into a NaN-filled dw, and
    beta = 1 onto a seeded dw (split 1: the kernel's own add; split > 1: rcf_splitk_reduce),
through ops.conv2d_wgrad / ops.conv2d_wgrad_bf16.  The split-K reduction has a fixed order: no tolerance, no skipped case.

The fixture is recorded from a build of the commit the values are to be held to:
    python tests/test_wgrad_bits_gpu.py --record [path]        (default path: tests/golden/wgrad_bits.json)
which runs every group twice and refuses to write a fixture whose two runs differ."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import pytest
import torch

import rcf_amd  # noqa: F401  (package alias)
import wgrad_cases as wg
from rcf_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIXTURE = os.path.join(HERE, "golden", "wgrad_bits.json")


def sha(t):
    b = t.detach().contiguous().cpu().reshape(-1)
    return hashlib.sha256(b.view(torch.uint8).numpy().tobytes()).hexdigest()


def run_variant(c, v, x, dy, dw0):
    """{"<variant>-beta0": hash, "<variant>-beta1": hash} of one variant; x, dy, dw0 fp32 on the device"""
    args = (c.stride, c.pad, c.dil)
    if v in wg.H16_VARIANTS:
        dt = torch.bfloat16 if v == "bf16" else torch.float16
        xh, dyh = x.to(dt), dy.to(dt)
        go = lambda dw, beta: ops.conv2d_wgrad_bf16(xh, dyh, dw, dw, *args, beta=beta, region=c.region)
        storage = ops.half_storage(dt)
    else:
        ax, ag = ops.absmax(x), ops.absmax(dy)
        if v == "planes":
            xp, dyp = wg.to_planes(x, ax)[0], wg.to_planes(dy, ag)[0]
            go = lambda dw, beta: ops.conv2d_wgrad(xp, dyp, dw, dw, *args, beta=beta, region=c.region, amax=(ax, ag), planes=True)
        else:
            go = lambda dw, beta: ops.conv2d_wgrad(x, dy, dw, dw, *args, beta=beta, region=c.region, amax=(ax, ag),
                                                   small_tile=v == "tile128")
        storage = ops.half_storage(torch.float32)                  # leaves the library alone
    o = {}
    old = ops.set_conv_flags(_lib.CONV_NO_WGRAD_XCD) if v == "noxcd" else None
    try:
        with storage:
            for beta in (0, 1):
                buf = torch.full_like(dw0, float("nan")) if beta == 0 else dw0.clone()      # [Cout][k][k][Cin]: the weight's memory
                dw = buf.permute(0, 3, 1, 2)
                go(dw, beta)
                o[f"{v}-beta{beta}"] = sha(buf)
    finally:
        if old is not None:
            ops.set_conv_flags(old)
    return o


def compute(c):
    x, dy, dw0 = (t.to(DEV) for t in wg.inputs(c))
    o = {}
    for v in wg.variants(c):
        o.update(run_variant(c, v, x, dy, dw0))
    return o


_fixture = []


def fixture():
    if not _fixture:
        with open(FIXTURE) as f:
            _fixture.append(json.load(f))
    return _fixture[0]


@pytest.mark.parametrize("c", wg.CASES, ids=lambda c: c.name)
def test_wgrad_bits_match_recorded_build(c):
    want = fixture()["groups"][c.name]
    got = compute(c)
    assert sorted(got) == sorted(want), "the outputs of this case are not the recorded ones"
    differ = [k for k in want if got[k] != want[k]]
    assert not differ, f"case {c.name}: outputs that differ from the recorded build: {differ}"


def test_wgrad_bits_fixture_covers_every_run():
    groups = fixture()["groups"]
    assert sorted(groups) == sorted(c.name for c in wg.CASES)
    for c in wg.CASES:
        assert sorted(groups[c.name]) == sorted(f"{v}-beta{b}" for v in wg.variants(c) for b in (0, 1)), c.name
        # a recording that did not reach the kernel shows as constants: beta = 1 adds the seeded dw, so its bytes are other ones
        assert all(groups[c.name][f"{v}-beta0"] != groups[c.name][f"{v}-beta1"] for v in wg.variants(c)), c.name
    # the two 16-bit libraries round their operands differently
    assert all(groups[c.name]["bf16-beta0"] != groups[c.name]["fp16-beta0"] for c in wg.CASES)


def record(path):
    groups = {}
    for c in wg.CASES:
        a, b = compute(c), compute(c)
        differ = [k for k in a if a[k] != b.get(k)]
        assert sorted(a) == sorted(b) and not differ, f"case {c.name}: two runs of the same build differ: {differ}"
        groups[c.name] = a
        print(f"{c.name}: {len(a)} outputs", flush=True)
    torch.cuda.synchronize()
    with open(path, "w") as f:
        json.dump({"what": "by case of tests/wgrad_cases.py and run: SHA-256 of the raw bytes of dw (tests/test_wgrad_bits_gpu.py)",
                   "groups": groups}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"recorded {sum(len(v) for v in groups.values())} hashes of {len(groups)} cases to {path}")


if __name__ == "__main__":
    if "--record" not in sys.argv:
        sys.exit("usage: python tests/test_wgrad_bits_gpu.py --record [path]")
    rest = sys.argv[sys.argv.index("--record") + 1:]
    record(rest[0] if rest else FIXTURE)
