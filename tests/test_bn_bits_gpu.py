"""The batch-norm family (csrc/bn.hip, and the finalize of csrc/foldbn.hip) bit for bit against a recorded build.

tests/test_bn_sweep_gpu.py holds the kernels to float64 with a floor; a change that only moves code must move NOTHING.  For every
run of tests/bn_cases.py this module takes the SHA-256 of the raw bytes of every output and demands equality with
tests/golden/bn_bits.json -- no tolerance, no skipped case, and for runs with 16-bit storage once per library (bf16 and IEEE
fp16).  The inputs come from bn_cases' seeded CPU generators, the block maxima are maxima and every sum has a fixed order, so
the hashes depend on the kernels alone.

The fixture is recorded from a build of the commit the hashes are to be held to:
    python tests/test_bn_bits_gpu.py --record [path]        (default path: tests/golden/bn_bits.json)
which runs every group twice and refuses to write a fixture whose two runs differ."""
import ctypes
import hashlib
import json
import os
import sys
from ctypes import c_void_p

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import pytest
import torch

import bn_cases as bc
import rcf_amd  # noqa: F401  (package alias)
from rcf_amd import _lib, layers, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
SLICE0 = 8
FIXTURE = os.path.join(HERE, "golden", "bn_bits.json")
BF, FP = torch.bfloat16, torch.float16
HALF_TAG = {BF: "bf16lib", FP: "f16lib"}
TRIO = ("idle_threads", "ragged_cgroup", "cap_1024")
SIDE = ("idle_threads", "ragged_cgroup", "pitched")
CHUNKS = (1, 7, 8, 31, 32, 33, 127, 128, 129, 255, 256, 257, 1023, 1024, 2047, 2048, 2049, 3210)


def sha(t):
    """SHA-256 of a tensor's raw bytes (a view: of the elements it shows), None for no tensor"""
    if t is None:
        return None
    b = t.detach().contiguous().cpu().reshape(-1)
    return hashlib.sha256(b.view(torch.uint8).numpy().tobytes()).hexdigest()


def vec(t):
    return None if t is None else t.float().to(DEV)


def slot():
    return torch.zeros(1, dtype=torch.int32, device=DEV)


class Bufs:
    """device operands of one run in the storage types T = {"f32": .., "bf16": the library's 16-bit type}: contiguous NHWC
    tensors, or channel slices [..., 8:8 + C] of FILL-ed wider buffers"""

    def __init__(self, case, var, half):
        self.case, self.var, self.T = case, var, {"f32": torch.float32, "bf16": half}

    def empty(self, dt, fill):
        c = self.case
        if not self.var.pitch:
            return torch.full((c.N, c.H, c.W, c.C), fill, dtype=self.T[dt], device=DEV)
        v = torch.full((c.N, c.H, c.W, self.var.pitch), bc.FILL, dtype=self.T[dt], device=DEV)[..., SLICE0:SLICE0 + c.C]
        v.fill_(fill)
        return v

    def put(self, mat, dt):
        c = self.case
        v = self.empty(dt, 0.0)
        v.copy_(mat.reshape(c.N, c.H, c.W, c.C).to(self.T[dt]))
        return v


def ones_mask(rows, C):
    return torch.full((rows * C // 4,), 0xFF, dtype=torch.uint8, device=DEV)


# --------------------------------------------------------------------------------------------------------------- groups
def run_family(case, var, half):
    """stats -> finalize -> apply (ReLU on and off) -> backward reduce and apply (from the sign bits, from y, without ReLU)"""
    i = bc.inputs(case.name, var.tag)
    rows, C, n = case.rows, case.C, case.rows
    B, o = Bufs(case, var, half), {}
    xg, dyg = B.put(i.x, var.xdt), B.put(i.dy, var.ydt)
    rg = B.put(i.r, var.ydt) if case.res else None
    gam, bet, kg = vec(i.gamma), vec(i.beta), vec(i.keep)
    sums = ops.bn_stats(xg)
    rm, rv = vec(i.rm0), vec(i.rv0)
    mean, invstd = ops.bn_finalize(sums, n, bc.EPS, bc.MOMENTUM, rm, rv)
    o.update(sums=sha(sums), mean=sha(mean), invstd=sha(invstd), running_mean=sha(rm), running_var=sha(rv))
    kept = {}
    for relu in (True, False):
        y, am = B.empty(var.ydt, NAN), slot()
        mask = ones_mask(rows, C) if relu else None
        ops.bn_apply(xg, mean, invstd, gam, bet, relu, residual=rg, chan_scale=kg, out=y, relu_mask=mask, amax_out=am)
        k = "apply_relu" if relu else "apply_lin"
        o.update({k + ".y": sha(y), k + ".mask": sha(mask), k + ".amax": sha(am)})
        kept[relu] = (y, mask)
    y, mask = kept[True]
    for k, relu, y_in, m_in in (("mask", True, None, mask), ("y", True, y, None), ("lin", False, None, None)):
        s2 = ops.bn_bwd_reduce(dyg, xg, y_in, mean, invstd, relu, chan_scale=kg, relu_mask=m_in)
        dgam, dbet, am = vec(i.dgamma0), vec(i.dbeta0), slot()
        dx, dres = B.empty(var.xdt, NAN), None
        if case.res:
            dres = B.put(i.dres0, var.ydt) if case.res_beta else B.empty(var.ydt, NAN)
        ops.bn_bwd_apply(dyg, xg, y_in, mean, invstd, gam, relu, s2, n, dgam, dbet, dx=dx, dres=dres, res_beta=case.res_beta,
                         chan_scale=kg, relu_mask=m_in, amax_out=am)
        o.update({f"bwd_{k}.sums2": sha(s2), f"bwd_{k}.dx": sha(dx), f"bwd_{k}.dres": sha(dres), f"bwd_{k}.dgamma": sha(dgam),
                  f"bwd_{k}.dbeta": sha(dbet), f"bwd_{k}.amax": sha(am)})
    return o


def banded_family(case, var, half):
    try:
        ops.BN_FLAGS = _lib.BN_SWEEP_ALWAYS
        return run_family(case, var, half)
    finally:
        ops.BN_FLAGS = 0


def norms_of(B, i, var, n):
    xg, x2g = B.put(i.x, var.xdt), B.put(i.x2, var.xdt)
    m1 = ops.bn_finalize(ops.bn_stats(xg), n, bc.EPS, bc.MOMENTUM)
    m2 = ops.bn_finalize(ops.bn_stats(x2g), n, bc.EPS, bc.MOMENTUM)
    return xg, x2g, m1, m2


def shared_family(case, var, half):
    """rcf_bn_bwd_reduce2_mp / rcf_bn_bwd_apply2_mp under bn_cases' random 4-bit mask; fp32 with C % 8 == 0: also as pair planes"""
    i = bc.make_inputs(case, var) if var.xdt == "bf16" else bc.inputs(case.name, "f32")
    rows, C, n = case.rows, case.C, case.rows
    B, o = Bufs(case, var, half), {}
    xg, x2g, (mean, invstd), (mean2, invstd2) = norms_of(B, i, var, n)
    dyg, mask = B.put(i.dy, var.ydt), i.mask4.to(DEV)
    s4 = ops.bn_bwd_reduce2(dyg, xg, x2g, mean, invstd, mean2, invstd2, mask)
    o["sums4"] = sha(s4)
    forms = [False] + ([True] if var.xdt == "f32" and C % 8 == 0 else [])
    for planes in forms:
        pg = [vec(v) for v in (i.dgamma0, i.dbeta0, i.dgamma20, i.dbeta20)]
        dx, dx2, am, am2 = B.empty(var.xdt, NAN), B.empty(var.xdt, NAN), slot(), slot()
        kw = dict(dx_planes=True, amax_x=ops.absmax(xg), amax_x2=ops.absmax(x2g), amax_dy=ops.absmax(dyg)) if planes else {}
        ops.bn_bwd_apply2(dyg, xg, mean, invstd, vec(i.gamma), mask, s4[:2 * C], n, pg[0], pg[1], dx, x2g, mean2, invstd2,
                          vec(i.gamma2), s4[2 * C:], pg[2], pg[3], dx2, amax_out=am, amax_out2=am2, **kw)
        k = "apply2_planes" if planes else "apply2"
        o.update({f"{k}.{q}": sha(t) for q, t in zip(("dx", "dx2", "dgamma", "dbeta", "dgamma2", "dbeta2", "amax", "amax2"),
                                                     [dx, dx2] + pg + [am, am2])})
    return o


def resnorm_family(case, var, half):
    """rcf_bn_apply_res_mp: the residual normalised on the fly, as y and (C % 8 == 0, no Dropout2d scale) as pair planes"""
    i = bc.inputs(case.name, "f32")
    rows, C, n = case.rows, case.C, case.rows
    B, o = Bufs(case, var, half), {}
    xg, x2g, (mean, invstd), (mean2, invstd2) = norms_of(B, i, var, n)
    rn = (mean2, invstd2, vec(i.gamma2), vec(i.beta2))
    y, mask, am = B.empty("f32", NAN), ones_mask(rows, C), slot()
    ops.bn_apply(xg, mean, invstd, vec(i.gamma), vec(i.beta), True, residual=x2g, chan_scale=vec(i.keep), out=y, relu_mask=mask,
                 amax_out=am, res_norm=rn)
    o.update(y=sha(y), mask=sha(mask), amax=sha(am))
    if C % 8 == 0:
        for only in (False, True):
            mask, bound, pl = ones_mask(rows, C), slot(), B.empty("f32", NAN)
            y = ops.bn_apply(xg, mean, invstd, vec(i.gamma), vec(i.beta), True, residual=x2g, relu_mask=mask, amax_out=bound, planes=pl,
                             planes_only=only, amax_x=ops.absmax(xg), amax_res=ops.absmax(x2g), res_norm=rn,
                             out=None if only else B.empty("f32", NAN))
            k = "planes_only" if only else "planes"
            o.update({k + ".planes": sha(pl), k + ".bound": sha(bound), k + ".mask": sha(mask), k + ".y": sha(y)})
    return o


def planes_family(case, var, half):
    """RCF_BN_Y_PLANES_ONLY / y and planes / RCF_BN_DX_PLANES: the planes and the bound slot; a case with a Dropout2d scale
    takes the backward form only (the forward planes refuse the scale) -- its bound scans the scale's largest entry"""
    i = bc.inputs(case.name, "f32")
    rows, C, n = case.rows, case.C, case.rows
    B, o = Bufs(case, var, half), {}
    xg, dyg = B.put(i.x, "f32"), B.put(i.dy, "f32")
    rg = B.put(i.r, "f32") if case.res else None
    gam, bet, kg = vec(i.gamma), vec(i.beta), vec(i.keep)
    mean, invstd = ops.bn_finalize(ops.bn_stats(xg), n, bc.EPS, bc.MOMENTUM)
    ax, ag = ops.absmax(xg), ops.absmax(dyg)
    ar = ops.absmax(rg) if case.res else None
    mask0 = ones_mask(rows, C)
    ops.bn_apply(xg, mean, invstd, gam, bet, True, residual=rg, chan_scale=kg, relu_mask=mask0, out=B.empty("f32", NAN))
    if not case.drop:
        for only in (False, True):
            mask, bound, pl = ones_mask(rows, C), slot(), B.empty("f32", NAN)
            y = ops.bn_apply(xg, mean, invstd, gam, bet, True, residual=rg, relu_mask=mask, amax_out=bound, planes=pl, planes_only=only,
                             amax_x=ax, amax_res=ar, out=None if only else B.empty("f32", NAN))
            k = "planes_only" if only else "planes"
            o.update({k + ".planes": sha(pl), k + ".bound": sha(bound), k + ".mask": sha(mask), k + ".y": sha(y)})
    s2 = ops.bn_bwd_reduce(dyg, xg, None, mean, invstd, True, chan_scale=kg, relu_mask=mask0)
    dgam, dbet, gb = vec(i.dgamma0), vec(i.dbeta0), slot()
    dres = B.empty("f32", NAN) if case.res else None
    dx = ops.bn_bwd_apply(dyg, xg, None, mean, invstd, gam, True, s2, n, dgam, dbet, dx=B.empty("f32", NAN), dres=dres, chan_scale=kg,
                          relu_mask=mask0, amax_out=gb, dx_planes=True, amax_x=ax, amax_dy=ag)
    o.update({"bwd.planes": sha(dx), "bwd.bound": sha(gb), "bwd.dres": sha(dres), "bwd.dgamma": sha(dgam), "bwd.dbeta": sha(dbet)})
    return o


def side_family(case, var, half):
    """rcf_colsum_mp and rcf_relu_mask_copy_mp (pitched out), beta 0 and 1"""
    i = bc.inputs(case.name, var.tag)
    C = case.C
    B, o = Bufs(case, var, half), {}
    dt = B.T[var.ydt]
    dyg, mask = B.put(i.dy, var.ydt), i.mask4.to(DEV)
    for beta in (0, 1):
        o[f"colsum_beta{beta}"] = sha(ops.colsum(dyg, vec(i.dgamma0), beta=beta))
        big = torch.full((case.N, case.H, case.W, C + 12), bc.FILL, dtype=dt, device=DEV)
        out = big[..., 4:4 + C]
        out.copy_(i.dres0.to(dt).reshape(out.shape)) if beta else out.fill_(NAN)
        ops.relu_mask_copy(dyg, mask, out=out, beta=beta)
        o[f"relu_mask_copy_beta{beta}"] = sha(big)
    return o


def sum_partials_family(n):
    """rcf_sum_partials_f64 over the chunk counts around every threshold, with a scratch buffer and with none"""
    g = torch.Generator().manual_seed(n)
    full = torch.randn(max(CHUNKS), n, generator=g, dtype=torch.float64) * torch.exp2(6 * torch.rand(max(CHUNKS), 1, generator=g, dtype=torch.float64))
    full_g = full.to(DEV)
    scratch = torch.empty(64 * n, dtype=torch.float64, device=DEV)
    o = {}
    for chunks in CHUNKS:
        for sc in (scratch, None):
            out = torch.full((n + 32,), bc.FILL, dtype=torch.float64, device=DEV)
            ops.call("rcf_sum_partials_f64", c_void_p(full_g.data_ptr()), chunks, n, c_void_p(out.data_ptr()),
                     None if sc is None else c_void_p(sc.data_ptr()), ops._stream())
            o[f"chunks{chunks}_{'scratch' if sc is not None else 'none'}"] = sha(out)
    return o


def fused_finalize_family(H, W):
    """rcf_sum_partials_bn behind a 1x1 64 -> 64 conv with fused statistics: short lists of row tiles, 256 .. 1023 and >= 1024"""
    g = torch.Generator().manual_seed(H)
    C = 64
    x = torch.randn(1, H, W, C, generator=g).to(DEV)
    w = (torch.randn(C, C, 1, 1, generator=g) / 8).to(DEV).contiguous(memory_format=torch.channels_last)
    bn = torch.nn.BatchNorm2d(C).to(DEV)
    bn.running_mean.copy_(torch.randn(C, generator=g))
    bn.running_var.copy_(torch.rand(C, generator=g) + 0.5)
    _, (mean, invstd, _) = ops.conv2d_fwd_stats(x, w, bn=bn)
    _, sums = ops.conv2d_fwd_stats(x, w)
    return dict(sums=sha(sums), mean=sha(mean), invstd=sha(invstd), running_mean=sha(bn.running_mean), running_var=sha(bn.running_var),
                num_batches_tracked=sha(bn.num_batches_tracked))


def fold_family(n, K, C, half):
    """the finalize of a folded 1x1 conv + batch norm (csrc/foldbn.hip): local statistics (finalized in the statistics launch) and
    the SyncBN form (two "ranks" of rows, their sums added, rcf_fold_finalize_f32 on the global count); and the sums-only
    rcf_sum_partials_bn behind rcf_relu_mask_colsum_bf16"""
    g = torch.Generator().manual_seed(n + K)
    X = torch.relu(torch.randn(n, K, generator=g) + 0.3).to(half)
    Wm = torch.randn(C, K, generator=g) * (2.0 / K) ** 0.5
    gam, bet = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    rm0, rv0 = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    dy = torch.randn(n, K, generator=g).to(half)
    xa = X.to(DEV).view(1, 1, n, K)
    wd = Wm.view(C, K, 1, 1).to(DEV).contiguous(memory_format=torch.channels_last)

    def norm():
        bn = layers.BatchNorm2d(C).to(DEV)
        bn.weight.data.copy_(gam)
        bn.bias.data.copy_(bet)
        bn.running_mean.copy_(rm0)
        bn.running_var.copy_(rv0)
        return bn
    o = {}
    S, A1 = ops.gram_bf16(xa), ops.bn_stats(xa)
    bn = norm()
    _, outs = ops.fold_fwd(S, A1, wd, bn, n)
    names = ("mean", "invstd", "scale", "shift", "running_mean", "running_var", "num_batches_tracked")
    o.update({"local." + k: sha(t) for k, t in zip(names, outs + (bn.running_mean, bn.running_var, bn.num_batches_tracked))})
    cut, sums = (n // 3 + 7) // 8 * 8, None
    for lo, hi in ((0, cut), (cut, n)):
        xr = xa[:, :, lo:hi].contiguous()
        _, s_r = ops.fold_fwd(ops.gram_bf16(xr), ops.bn_stats(xr), wd, rows=hi - lo)
        sums = s_r if sums is None else sums + s_r
    bn = norm()
    outs = ops.fold_finalize(sums, n, bn)
    o.update({"sync." + k: sha(t) for k, t in zip(names, outs + (bn.running_mean, bn.running_var, bn.num_batches_tracked))})
    gm, cs = ops.relu_mask_colsum(dy.to(DEV).view(1, 1, n, K), xa)
    o.update({"mask_colsum.g": sha(gm), "mask_colsum.sums": sha(cs)})
    return o


def _groups():
    """id -> (function, args, 16-bit type or None): every group is one test case"""
    G = {}

    def add(gid, fn, args, sixteen):
        for half in ((BF, FP) if sixteen else (BF,)):
            G[gid + (f"/{HALF_TAG[half]}" if sixteen else "")] = (fn, args, half)
    for c, v in bc.RUNS:
        add(f"run/{c.name}-{v.tag}", run_family, (c, v), "bf16" in (v.xdt, v.ydt))
    add("banded/cap_1024-f32", banded_family, (bc.BY_NAME["cap_1024"], bc.F32), False)
    for name in TRIO:
        c = bc.BY_NAME[name]
        add(f"shared/{name}-f32", shared_family, (c, bc.F32), False)
        add(f"shared/{name}-bf16", shared_family, (c, bc.BF16), True)
        add(f"resnorm/{name}", resnorm_family, (c, bc.F32), False)
    for c in bc.PLANE_CASES + [bc.BY_NAME["idle_threads"]]:
        add(f"planes/{c.name}", planes_family, (c, bc.F32), False)
    for c, v in bc.RUNS:
        if c.name in SIDE:
            add(f"side/{c.name}-{v.tag}", side_family, (c, v), "bf16" in (v.xdt, v.ydt))
    for n in (8, 96, 512, 1024, 4096):
        G[f"sum_partials/n{n}"] = (lambda n, half: sum_partials_family(n), (n,), BF)
    for H, W in ((64, 96), (199, 211), (331, 431)):
        G[f"fused_finalize/{H}x{W}"] = (lambda H, W, half: fused_finalize_family(H, W), (H, W), BF)
    for shape in ((3000, 64, 256), (2500, 128, 512)):
        add("fold/" + "x".join(map(str, shape)), fold_family, shape, True)
    return G


GROUPS = _groups()


def compute(gid):
    fn, args, half = GROUPS[gid]
    with ops.half_storage(half):
        return fn(*args, half)


_fixture = []


def fixture():
    if not _fixture:
        with open(FIXTURE) as f:
            _fixture.append(json.load(f))
    return _fixture[0]


@pytest.mark.parametrize("gid", list(GROUPS))
def test_bn_bits_match_recorded_build(gid):
    want = fixture()["groups"][gid]
    got = compute(gid)
    assert sorted(got) == sorted(want), "the outputs of this group are not the recorded ones"
    differ = [k for k in want if got[k] != want[k]]
    assert not differ, f"{gid}: outputs whose bytes differ from the recorded build: {differ}"


def test_bn_bits_fixture_covers_every_group():
    assert sorted(fixture()["groups"]) == sorted(GROUPS)


def record(path):
    groups = {}
    for gid in GROUPS:
        a, b = compute(gid), compute(gid)
        assert a == b, f"{gid}: two runs of the same build differ: {[k for k in a if a[k] != b[k]]}"
        groups[gid] = a
        print(f"{gid}: {len(a)} outputs", flush=True)
    torch.cuda.synchronize()
    with open(path, "w") as f:
        json.dump({"what": "SHA-256 of the raw bytes of every output, by group (tests/test_bn_bits_gpu.py)", "groups": groups}, f,
                  indent=0, sort_keys=True)
        f.write("\n")
    print(f"recorded {sum(len(v) for v in groups.values())} hashes of {len(groups)} groups to {path}")


if __name__ == "__main__":
    if "--record" not in sys.argv:
        sys.exit("usage: python tests/test_bn_bits_gpu.py --record [path]")
    rest = sys.argv[sys.argv.index("--record") + 1:]
    record(rest[0] if rest else FIXTURE)
