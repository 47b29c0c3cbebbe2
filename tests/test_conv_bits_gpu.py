"""The forward and data-gradient conv kernels (csrc/igemm_conv.hip: igemm_conv_x3_kernel, conv_h2d_kernel, conv_h2p_kernel,
igemm_conv_kernel; csrc/igemm_bf16.hip: conv_bf16_kernel) bit for bit against a recorded build.

tests/test_kernels_gpu.py, test_planes_gpu.py, test_tap_skip_gpu.py, test_bf16_gpu.py, test_fp16_gpu.py and test_fold_gpu.py hold
these kernels to float64 and to each other within bounds; a change that only moves their code must move NOTHING.  For every case of
tests/conv_cases.py and every variant it lists this module takes the SHA-256 of the raw bytes of everything a run writes -- the
output, the fused statistics or the finalised mean and invstd, amax_y, the ReLU bit words, the column sums and the lean data
gradient's sums2 -- at beta = 0 into a NaN-filled output and at beta = 1 onto a seeded one wherever the entry point takes beta.
These kernels have no float atomics and amax_y is an integer max: no tolerance, no skipped case.

The fixture is recorded from a build of the commit the values are to be held to:
    python tests/test_conv_bits_gpu.py --record [path]        (default path: tests/golden/conv_bits.json)
which runs every group twice and refuses to write a fixture whose two runs differ."""
import hashlib
import json
import os
import sys
from contextlib import contextmanager

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import pytest
import torch

import rcf_amd  # noqa: F401  (package alias)
import conv_cases as cc
from rcf_amd import ops
from wgrad_cases import to_planes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIXTURE = os.path.join(HERE, "golden", "conv_bits.json")
NAN = float("nan")


def sha(*ts):
    """one digest over the raw bytes of the tensors a run wrote (None: not written by this run)"""
    h = hashlib.sha256()
    for t in ts:
        if t is not None:
            h.update(t.detach().contiguous().cpu().reshape(-1).view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


@contextmanager
def conv_flags(flags):
    old = ops.set_conv_flags(ops.CONV_FLAGS | flags)
    try:
        yield
    finally:
        ops.set_conv_flags(old)


def target(seed_t, beta, dtype=None):
    """what a run writes into: NaN everywhere (beta = 0) or the seeded tensor (beta = 1)"""
    t = seed_t if dtype is None else seed_t.to(dtype)
    return torch.full_like(t, NAN) if beta == 0 else t.clone()


def batch_norm(C):
    return torch.nn.BatchNorm2d(C).to(DEV).train()


def run_f32(c, v, T):
    """{"<variant>/<run>": digest} of one fp32 variant of a case; T: the case's tensors on the device"""
    o = {}
    put = lambda run, *ts: o.__setitem__(f"{v}/{run}", sha(*ts))
    geo = (c.stride, c.pad, c.dil)
    x, dy, w = T["x"][..., :c.Cin], T["dy"][..., :c.Cout], T["w"]
    xshape = (c.N, c.H, c.W, c.Cin)
    mfma = v in cc.MFMAS
    ranged = v != "x3" and not mfma
    planes = v in ("planes", "leanp")
    with conv_flags(cc.FLAGS.get(v, 0)):
        fkw, dkw = {}, {}
        if ranged:
            ax, aw, ag = ops.absmax(x), ops.absmax(ops.weight_rsck(w)), ops.absmax(dy)
            fkw, dkw = dict(amax=(ax, aw)), dict(amax=(ag, aw))
            if v != "h2":                                            # the K order is baked into the planes: made under the flags
                fkw["w_pairs"], dkw["w_pairs_t"] = ops.weight_pairs(w, aw), ops.weight_pairs_t(w, aw)
            if planes:
                x, dy = to_planes(x, ax)[0], to_planes(dy, ag)[0]
                fkw["x_planes"], dkw["dy_planes"] = True, True
        rng = lambda: None if mfma else ops.new_amax(DEV)
        if v in ("lean", "leanp"):
            chan = T["chan"]
            bn = (T["x"][..., :c.Cin].contiguous(), T["masks"][0], chan[0, :c.Cin].clone(), chan[1, :c.Cin].clone())
            add = (T["dx0"], T["masks"][1])
            for beta in (0, 1):
                r = rng()
                dx, s2 = ops.conv2d_dgrad(dy, w, xshape, *geo, out=target(T["dx0"], beta), beta=beta, amax_y=r, bn_bwd=bn, **dkw)
                assert s2 is not None, "this case must take the lean epilogue"
                put(f"dgrad-bnsums-beta{beta}", dx, s2, r)
            r = rng()
            put("dgrad-add", ops.conv2d_dgrad(dy, w, xshape, *geo, out=target(T["dx0"], 0), amax_y=r, addend=add, **dkw), r)
            dx, s2 = ops.conv2d_dgrad(dy, w, xshape, *geo, out=target(T["dx0"], 0), addend=add, bn_bwd=bn, **dkw)
            assert s2 is not None
            put("dgrad-add-bnsums", dx, s2)
            return o
        if v == "band":
            for beta in (0, 1):
                r = rng()
                put(f"dgrad-band-beta{beta}", ops.conv2d_dgrad(dy, w, xshape, *geo, out=target(T["dx0"], beta), beta=beta, region=c.region,
                                                               amax_y=r, dy_band=2, **dkw), r)
            return o
        for beta in (0, 1):
            r = rng()
            put(f"fwd-beta{beta}", ops.conv2d_fwd(x, w, None, *geo, out=target(T["y0"], beta), beta=beta, region=c.region, amax_y=r, **fkw), r)
            if v != "h2p":                                           # bias and activation: the general epilogue (conv_h2p_kernel has none)
                r = rng()
                put(f"fwd-bias-beta{beta}", ops.conv2d_fwd(x, w, T["bias"], *geo, act=1, slope=0.1, out=target(T["y0"], beta), beta=beta,
                                                           region=c.region, amax_y=r, **fkw), r)
            r = rng()
            put(f"dgrad-beta{beta}", ops.conv2d_dgrad(dy, w, xshape, *geo, out=target(T["dx0"], beta), beta=beta, region=c.region, amax_y=r, **dkw), r)
        if c.region is None and not mfma:                            # the fused statistics: whole tensors, the default kernels
            r = rng()
            y, sums = ops.conv2d_fwd_stats(x, w, *geo, amax_y=r, **fkw)
            put("fwd-stats", y, sums, r)
            y, (mean, invstd, _) = ops.conv2d_fwd_stats(x, w, *geo, bn=batch_norm(c.Cout), **fkw)
            put("fwd-bnstats", y, mean, invstd)
    return o


def col_tile(C):
    return 64 if C <= 64 else (128 if C <= 128 else 256)


def run_h16(c, v, T):
    """the same for 16-bit operands in the library of `v`"""
    o = {}
    put = lambda run, *ts: o.__setitem__(f"{v}/{run}", sha(*ts))
    geo = (c.stride, c.pad, c.dil)
    dt = torch.bfloat16 if v == "bf16" else torch.float16
    xshape = (c.N, c.H, c.W, c.Cin)
    with ops.half_storage(dt):
        x, dy, w = T["x"].to(dt)[..., :c.Cin], T["dy"].to(dt)[..., :c.Cout], T["w"]
        wb, wtb = ops.weight_bf16(w), ops.weight_bf16(w, True)
        for beta in (0, 1):
            put(f"fwd16-bias-beta{beta}", ops.conv2d_fwd_bf16(x, w, wb, T["bias"], *geo, out=target(T["y0"], beta, dt), beta=beta, region=c.region))
            put(f"fwd32-beta{beta}", ops.conv2d_fwd_bf16(x, w, wb, None, *geo, out=target(T["y0"], beta), beta=beta, region=c.region))
            put(f"fwd32-bias-beta{beta}", ops.conv2d_fwd_bf16(x, w, wb, T["bias"], *geo, act=1, slope=0.1, out=target(T["y0"], beta), beta=beta,
                                                             region=c.region))
            put(f"dgrad-beta{beta}", ops.conv2d_dgrad_bf16(dy, w, xshape, *geo, out=target(T["dx0"], beta, dt), beta=beta, region=c.region, w_t_bf16=wtb))
        if c.region is None:
            put("fwd16-stats", *ops.conv2d_fwd_bf16(x, w, wb, None, *geo, stats=True))
            put("fwd32-stats", *ops.conv2d_fwd_bf16(x, w, wb, None, *geo, out_dtype=torch.float32, stats=True))
            y, (mean, invstd, _) = ops.conv2d_fwd_bf16(x, w, wb, None, *geo, stats=True, bn=batch_norm(c.Cout))
            put("fwd16-bnstats", y, mean, invstd)
        fused = c.region is None and c.stride == 1 and not c.pitch
        chan = T["chan"]
        if fused and c.Cout % col_tile(c.Cout) == 0:                 # EP 1: whole column tiles
            scale, shift = chan[2, :c.Cout].clone(), chan[3, :c.Cout].clone() - 1.0
            for res in (None, T["y0"].to(dt)):
                for relu in (False, True):
                    y = ops.conv2d_fwd_affine_bf16(x, w, wb, scale, shift, residual=res, relu=relu, stride=c.stride, pad=c.pad, dil=c.dil, want_bits=relu)
                    put(f"affine-res{int(res is not None)}-relu{int(relu)}", *(y if relu else (y,)))
        if fused and c.Cin % col_tile(c.Cin) == 0:                   # EP 2 / EP 3
            xm = x.contiguous()
            # the bits of an [N, H, W, Cin] output in its tile order: from an affine forward that writes that shape (a 1x1 conv of x)
            g = torch.Generator().manual_seed(c.seed + 500)
            w1 = (torch.randn(c.Cin, c.Cin, 1, 1, generator=g) / c.Cin ** 0.5).to(DEV).contiguous(memory_format=torch.channels_last)
            _, bits = ops.conv2d_fwd_affine_bf16(xm, w1, ops.weight_bf16(w1), chan[2, :c.Cin].clone(), chan[3, :c.Cin].clone() - 1.0, relu=True, want_bits=True)
            for beta in (0, 1):
                put(f"masked-beta{beta}", *ops.conv2d_dgrad_masked_bf16(dy, w, xshape, wtb, xm, target(T["dx0"], beta, dt), beta, *geo))
                put(f"maskbits-beta{beta}", *ops.conv2d_dgrad_masked_bf16(dy, w, xshape, wtb, None, target(T["dx0"], beta, dt), beta, *geo, mask_bits=bits))
    return o


def compute(c):
    T = {k: t.to(DEV) for k, t in cc.inputs(c).items()}
    T["w"] = T["w"].contiguous(memory_format=torch.channels_last)
    o = {}
    for v in c.variants:
        o.update(run_h16(c, v, T) if v in cc.H16_VARIANTS else run_f32(c, v, T))
    return o


def compute_gemm():
    """rcf_gemm_nt_f32 on bf16 triples, on fp16 pairs and with b split beforehand; bias + GELU with the output's range"""
    q = cc.GEMM
    g = torch.Generator().manual_seed(q["seed"])
    a, b = torch.randn(q["M"], q["K"], generator=g).to(DEV), (torch.randn(q["N"], q["K"], generator=g) / q["K"] ** 0.5).to(DEV)
    bias, c0 = torch.randn(q["N"], generator=g).to(DEV), torch.randn(q["M"], q["N"], generator=g).to(DEV)
    aa, ab = ops.absmax(a), ops.absmax(b)
    o = {}
    for v, kw in (("x3", {}), ("h2", dict(amax=(aa, ab))), ("pre", dict(amax=(aa, ab), b_pairs=ops.weight_pairs_2d(b, ab)))):
        for beta in (0, 1):
            o[f"{v}/gemm-beta{beta}"] = sha(ops.gemm_nt(a, b, out=target(c0, beta), beta=beta, **kw))
            r = ops.new_amax(DEV)
            o[f"{v}/gemm-gelu-beta{beta}"] = sha(ops.gemm_nt(a, b, bias, out=target(c0, beta), act=2, beta=beta, amax_out=r, **kw), r)
    return o


def compute_bgemm():
    q = cc.BGEMM
    (b0, b1), M, N, K = q["batch"], q["M"], q["N"], q["K"]
    g = torch.Generator().manual_seed(q["seed"])
    a, b = torch.randn(b0, b1, M, K, generator=g).to(DEV), torch.randn(b0, b1, N, K, generator=g).to(DEV)
    c0 = torch.randn(b0, b1, M, N, generator=g).to(DEV)
    o = {}
    for beta in (0, 1):
        out = target(c0, beta)
        ops.gemm_nt_batched(a, K, (b1 * M * K, M * K), b, K, (b1 * N * K, N * K), out, N, (b1 * M * N, M * N), (b0, b1), M, N, K, beta=beta)
        o[f"x3/bgemm-beta{beta}"] = sha(out)
    return o


GROUPS = {c.name: (lambda c=c: compute(c)) for c in cc.CASES}
GROUPS.update(GEMM=compute_gemm, BGEMM=compute_bgemm)

_fixture = []


def fixture():
    if not _fixture:
        with open(FIXTURE) as f:
            _fixture.append(json.load(f))
    return _fixture[0]


@pytest.mark.parametrize("name", list(GROUPS))
def test_conv_bits_match_recorded_build(name):
    want = fixture()["groups"][name]
    got = GROUPS[name]()
    assert sorted(got) == sorted(want), "the outputs of this case are not the recorded ones"
    differ = [k for k in want if got[k] != want[k]]
    assert not differ, f"case {name}: outputs that differ from the recorded build: {differ}"


def test_conv_bits_fixture_covers_every_run():
    groups = fixture()["groups"]
    assert sorted(groups) == sorted(GROUPS)
    for c in cc.CASES:
        runs = groups[c.name]
        assert {k.split("/")[0] for k in runs} == set(c.variants), c.name
        # a recording that did not reach the kernel shows as constants: beta = 1 adds the seeded tensor, so its bytes are other ones
        pairs = [k for k in runs if k.endswith("-beta0")]
        assert pairs and all(runs[k] != runs[k[:-1] + "1"] for k in pairs), c.name
        # the two 16-bit libraries round their operands differently
        if "bf16" in c.variants:
            h16 = [k.split("/")[1] for k in runs if k.startswith("bf16/")]
            assert h16 and all(runs[f"bf16/{k}"] != runs[f"fp16/{k}"] for k in h16), c.name
    for name in ("GEMM", "BGEMM"):
        assert all(groups[name][k] != groups[name][k[:-1] + "1"] for k in groups[name] if k.endswith("-beta0")), name


def record(path):
    groups = {}
    for name, go in GROUPS.items():
        a, b = go(), go()
        differ = [k for k in a if a[k] != b.get(k)]
        assert sorted(a) == sorted(b) and not differ, f"case {name}: two runs of the same build differ: {differ}"
        groups[name] = a
        print(f"{name}: {len(a)} outputs", flush=True)
    torch.cuda.synchronize()
    with open(path, "w") as f:
        json.dump({"what": "by case of tests/conv_cases.py and variant/run: SHA-256 of the raw bytes of everything the run writes "
                           "(tests/test_conv_bits_gpu.py)", "groups": groups}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"recorded {sum(len(v) for v in groups.values())} hashes of {len(groups)} groups to {path}")


if __name__ == "__main__":
    if "--record" not in sys.argv:
        sys.exit("usage: python tests/test_conv_bits_gpu.py --record [path]")
    rest = sys.argv[sys.argv.index("--record") + 1:]
    record(rest[0] if rest else FIXTURE)
