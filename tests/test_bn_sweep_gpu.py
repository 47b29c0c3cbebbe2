"""The batch-norm kernels (csrc/bn.hip) against a float64 restatement at the edges of their launch geometry
(tests/bn_cases.py; conditioning of every case: tests/test_bn_sweep_cpu.py).  Errors are taken PER CHANNEL against float64
scales (the channels differ 8x in scale: a wrong small channel must not hide under a large one) and held to the floors the
project already uses: 2e-5 (fp32 tensors), 5e-7 (raw fp64 sums), 5e-3 (stored bf16), 1e-6 (sums of bf16-exact inputs)."""
import copy
import ctypes
from ctypes import c_void_p

import numpy as np
import pytest
import torch

import bn_cases as bc
import rcf_amd  # noqa: F401  (package alias)
from rcf_amd import _lib, ops
from test_planes_gpu import from_planes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TORCH = bc.TORCH
NAN = float("nan")
SLICE0 = 8                                            # first channel of a pitched operand inside its buffer


class Bufs:
    """device operands of one run: contiguous NHWC tensors, or channel slices [..., 8:8 + C] of FILL-ed wider buffers whose
    guard channels are checked at the end"""

    def __init__(self, case, var):
        self.case, self.var, self.wide = case, var, []

    def empty(self, dt, fill):
        c = self.case
        if not self.var.pitch:
            return torch.full((c.N, c.H, c.W, c.C), fill, dtype=TORCH[dt], device=DEV)
        big = torch.full((c.N, c.H, c.W, self.var.pitch), bc.FILL, dtype=TORCH[dt], device=DEV)
        self.wide.append(big)
        v = big[..., SLICE0:SLICE0 + c.C]
        v.fill_(fill)
        return v

    def put(self, mat, dt):
        c = self.case
        v = self.empty(dt, 0.0)
        v.copy_(mat.reshape(c.N, c.H, c.W, c.C).to(TORCH[dt]))
        return v

    def guards_intact(self):
        C = self.case.C
        return all(bool((b[..., :SLICE0] == bc.FILL).all()) and bool((b[..., SLICE0 + C:] == bc.FILL).all()) for b in self.wide)


def mat(t):
    """device NHWC (view) -> float64 [rows, C] on the CPU"""
    return t.double().cpu().reshape(-1, t.shape[-1])


def vec(t):
    return None if t is None else t.float().to(DEV)


def same(a, b):
    """bit-equal, NaN == NaN"""
    if a is None or b is None:
        return a is None and b is None
    return a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def veq(a, b):
    """equal in value (-0 == 0: a gradient zeroed through y > 0 is +0 where dy * 0 under a set sign bit may be -0); a NaN fails"""
    return (a is None and b is None) or torch.equal(a, b)


def twice(fn):
    """every call runs twice on fresh outputs: bit-equal"""
    a, b = fn(), fn()
    a = a if isinstance(a, tuple) else (a,)
    b = b if isinstance(b, tuple) else (b,)
    assert len(a) == len(b) and all(same(p, q) for p, q in zip(a, b)), "two runs of the same call differ"
    return a if len(a) > 1 else a[0]


def bits_of_max(t):
    return int(t.float().abs().max().view(torch.int32))


def lib_chunks(rows, C):
    """chunk rows of the reductions' workspace, from the library's own query"""
    return _lib.load().rcf_bn_stats_workspace_bytes(rows, C) // (2 * C * 8)


def check(errs, floors, what):
    bad = {k: v for k, v in errs.items() if not v < floors[k]}
    assert not bad, f"{what}: over the floor {bad} (all: {errs})"


def run_case(case, var, report, tag=""):
    """stats -> finalize -> apply (ReLU on and off) -> backward reduce (from the mask and from y) -> backward apply, every
    output per channel against float64"""
    i, f = bc.inputs(case.name, var.tag), bc.truth(case.name, var.tag)
    rows, C, n = case.rows, case.C, case.rows
    fl, B = bc.floors(var), Bufs(case, var)
    geo = bc.geometry(case, var)
    assert lib_chunks(rows, C) == bc.workspace_chunks(rows, C)
    xg, dyg = B.put(i.x, var.xdt), B.put(i.dy, var.ydt)
    rg = B.put(i.r, var.ydt) if case.res else None
    gam, bet = vec(i.gamma), vec(i.beta)
    kg = vec(i.keep)
    e = {}

    # ---- forward statistics, running statistics from random values
    sums = twice(lambda: ops.bn_stats(xg))

    def finalize():
        rm, rv = vec(i.rm0), vec(i.rv0)
        return ops.bn_finalize(sums, n, bc.EPS, bc.MOMENTUM, rm, rv) + (rm, rv)
    mean, invstd, rm, rv = twice(finalize)
    s = bc.scales(i, f)
    sc = sums.cpu()
    e["sum"], e["sumsq"] = bc.chan_err(sc[:C], f.sum, s.sum), bc.chan_err(sc[C:], f.sumsq, s.sumsq)
    for k, t in (("mean", mean), ("invstd", invstd), ("rm", rm), ("rv", rv)):
        e[k] = bc.chan_err(t.cpu(), getattr(f, k), getattr(s, k))

    # ---- forward apply
    want_amax = var.xdt == "f32" and var.ydt == "f32"

    def apply(relu):
        y = B.empty(var.ydt, NAN)
        mask = torch.full((rows * C // 4,), 0xFF, dtype=torch.uint8, device=DEV) if relu else None
        am = torch.zeros(1, dtype=torch.int32, device=DEV) if want_amax else None
        ops.bn_apply(xg, mean, invstd, gam, bet, relu, residual=rg, chan_scale=kg, out=y, relu_mask=mask, amax_out=am)
        return (y, mask, am) if relu else (y, am)
    y, mask, am = twice(lambda: apply(True))
    y_lin, am_lin = twice(lambda: apply(False))
    e["y"], e["y_lin"] = bc.chan_err(mat(y), f.y, s.y), bc.chan_err(mat(y_lin), f.y_lin, s.y_lin)
    if want_amax:
        assert int(am) == bits_of_max(y) and int(am_lin) == bits_of_max(y_lin), "amax_out is not the range of the kernel's own output"
    assert int(mask.max()) < 16, "a sign-bit byte was left unwritten or has its high nibble set"
    kpat = bc.mask_to_pattern(mask.cpu(), rows, C)
    near = bc.near_zero(f.pre)
    share = float(near.double().mean())
    assert share <= bc.TIE_SHARE
    assert bool(((kpat == (f.pre > 0)) | near).all()), "a sign bit outside the tie margin differs from float64"
    pat = bc.pattern_with_ties(f.pre, kpat)

    # ---- backward reduce: from the sign bits, and from y -- bit-equal
    s2 = twice(lambda: ops.bn_bwd_reduce(dyg, xg, None, mean, invstd, True, chan_scale=kg, relu_mask=mask))
    s2y = twice(lambda: ops.bn_bwd_reduce(dyg, xg, y, mean, invstd, True, chan_scale=kg))
    assert veq(s2, s2y), "the backward sums from y differ from those from the sign bits"
    b = bc.backward(i, f, pat, torch.float64)
    s = bc.scales(i, f, b, case.res_beta)
    s2c = s2.cpu()
    e["sg"], e["sgx"] = bc.chan_err(s2c[:C], b.sg, s.sg), bc.chan_err(s2c[C:], b.sgx, s.sgx)

    # ---- backward apply: dgamma / dbeta accumulate onto random values, dx (and an overwritten dres) start as NaN
    def bwd_apply(y_in, m_in, local=None):
        dgam, dbet = vec(i.dgamma0), vec(i.dbeta0)
        dx = B.empty(var.xdt, NAN)
        dres = None
        if case.res:
            dres = B.put(i.dres0, var.ydt) if case.res_beta else B.empty(var.ydt, NAN)
        ops.bn_bwd_apply(dyg, xg, y_in, mean, invstd, gam, True, s2, n, dgam, dbet, dx=dx, dres=dres, res_beta=case.res_beta,
                         chan_scale=kg, sums2_local=local, relu_mask=m_in)
        return dx, dres, dgam, dbet
    dx, dres, dgam, dbet = twice(lambda: bwd_apply(None, mask))
    dxy, dresy, dgy, dby = bwd_apply(y, None)
    assert veq(dx, dxy) and veq(dres, dresy) and veq(dgam, dgy) and veq(dbet, dby), "backward apply from y differs"
    e["dx"] = bc.chan_err(mat(dx), b.dx, s.dx)
    if case.res:
        e["dres"] = bc.chan_err(mat(dres), b.dres + (i.dres0 if case.res_beta else 0.0), s.dres)
    e["dgamma"] = bc.chan_err(dgam.cpu(), i.dgamma0 + b.sgx, s.sgx)
    e["dbeta"] = bc.chan_err(dbet.cpu(), i.dbeta0 + b.sg, s.sg)
    if case.rows == 1:
        assert not mat(dx).any(), "one value per channel: dx is identically 0"
    # this rank's sums differ from the all-reduced ones: the parameter gradients follow the local sums, dx the global ones
    local = s2 * 1.5 + 0.25
    dxl, dresl, dgl, dbl = bwd_apply(None, mask, local)
    assert same(dxl, dx) and same(dresl, dres)
    assert same(dgl, vec(i.dgamma0) + local[C:].float()) and same(dbl, vec(i.dbeta0) + local[:C].float())

    assert B.guards_intact(), "a guard channel of a pitched buffer was written"
    worst = max(v / fl[k] for k, v in e.items())
    report(f"bn sweep {case.name}-{var.tag}{tag}: V {geo.V} col {geo.col.chunks} chunks x {geo.col.cgroups} groups (RG {geo.col.RG}, "
           f"{geo.cols} columns), ew grid {geo.ew.bx} x {geo.ew.cchunks} (rpb {geo.ew.rpb}), workspace rows {lib_chunks(rows, C)}; "
           + " ".join(f"{k} {v:.2e}" for k, v in e.items()) + f"; near-zero share {share:.1e}; worst error / floor {worst:.3f}")
    check(e, fl, f"{case.name}-{var.tag}{tag}")


@pytest.mark.parametrize("case,var", bc.PARAMS_RUNS)
def test_bn_sweep_vs_float64(case, var, report):
    run_case(case, var, report)


def test_bn_sweep_banded_row_order_vs_float64(report):
    """cap_1024 under RCF_BN_SWEEP_ALWAYS: the banded row orders against float64, not against the plain order of the same kernels"""
    case = bc.BY_NAME["cap_1024"]
    assert case.rows >= 8192
    try:
        ops.BN_FLAGS = _lib.BN_SWEEP_ALWAYS
        run_case(case, bc.F32, report, tag=" (banded)")
    finally:
        ops.BN_FLAGS = 0


TRIO = ("idle_threads", "ragged_cgroup", "cap_1024")


@pytest.mark.parametrize("name", TRIO)
def test_bn_sweep_residual_normalised_on_the_fly(name, report):
    """rcf_bn_apply_res_mp: relu(bn(x) + bn_r(r)) against its float64, where it was only compared with the two passes it replaces"""
    case, var = bc.BY_NAME[name], bc.F32
    i, f = bc.inputs(name, "f32"), bc.truth(name, "f32", True)
    rows, C, n = case.rows, case.C, case.rows
    B = Bufs(case, var)
    xg, x2g = B.put(i.x, "f32"), B.put(i.x2, "f32")
    mean, invstd = ops.bn_finalize(ops.bn_stats(xg), n, bc.EPS, bc.MOMENTUM)
    mean2, invstd2 = ops.bn_finalize(ops.bn_stats(x2g), n, bc.EPS, bc.MOMENTUM)

    def apply():
        y, mask = B.empty("f32", NAN), torch.full((rows * C // 4,), 0xFF, dtype=torch.uint8, device=DEV)
        ops.bn_apply(xg, mean, invstd, vec(i.gamma), vec(i.beta), True, residual=x2g, chan_scale=vec(i.keep), out=y, relu_mask=mask,
                     res_norm=(mean2, invstd2, vec(i.gamma2), vec(i.beta2)))
        return y, mask
    y, mask = twice(apply)
    s = bc.scales(i, f)
    e = {"y": bc.chan_err(mat(y), f.y, s.y), "mean2": bc.chan_err(mean2.cpu(), f.mean2, i.x2.abs().mean(0)),
         "invstd2": bc.chan_err(invstd2.cpu(), f.invstd2, f.invstd2)}
    near = bc.near_zero(f.pre)
    share = float(near.double().mean())
    report(f"bn sweep {name}: residual normalised on the fly " + " ".join(f"{k} {v:.2e}" for k, v in e.items()) + f"; near-zero share {share:.1e}")
    assert share <= bc.TIE_SHARE and int(mask.max()) < 16
    assert bool(((bc.mask_to_pattern(mask.cpu(), rows, C) == (f.pre > 0)) | near).all())
    assert max(e.values()) < bc.FLOOR_F32


@pytest.mark.parametrize("tag", ["f32", "bf16"])
@pytest.mark.parametrize("name", TRIO)
def test_bn_sweep_shared_backward_passes(name, tag, report):
    """rcf_bn_bwd_reduce2_mp / rcf_bn_bwd_apply2_mp under a random 4-bit mask: all four sums, both input gradients and both
    pairs of parameter gradients against float64 with that mask as its pattern"""
    case = bc.BY_NAME[name]
    var = bc.variant(case, tag) if tag == "f32" else bc.BF16
    i = bc.make_inputs(case, var) if tag == "bf16" else copy.copy(bc.inputs(name, "f32"))
    rows, C, n = case.rows, case.C, case.rows
    i.keep, i.r = None, None                      # the two-norm passes take neither a dropout scale nor a residual
    f = bc.forward(i, torch.float64, True)
    pat = bc.mask_to_pattern(i.mask4, rows, C)
    xhat2 = (i.x2 - f.mean2) * f.invstd2
    b = bc.backward(i, f, pat, torch.float64)
    b2 = bc.backward(i, f, pat, torch.float64, xhat=xhat2, gamma=i.gamma2, invstd=f.invstd2)
    B = Bufs(case, var)
    xg, x2g, dyg = B.put(i.x, var.xdt), B.put(i.x2, var.xdt), B.put(i.dy, var.ydt)
    mask = i.mask4.to(DEV)
    mean, invstd = ops.bn_finalize(ops.bn_stats(xg), n, bc.EPS, bc.MOMENTUM)
    mean2, invstd2 = ops.bn_finalize(ops.bn_stats(x2g), n, bc.EPS, bc.MOMENTUM)
    s4 = twice(lambda: ops.bn_bwd_reduce2(dyg, xg, x2g, mean, invstd, mean2, invstd2, mask))

    def apply2():
        pg = [vec(v) for v in (i.dgamma0, i.dbeta0, i.dgamma20, i.dbeta20)]
        dx, dx2 = B.empty(var.xdt, NAN), B.empty(var.xdt, NAN)
        ops.bn_bwd_apply2(dyg, xg, mean, invstd, vec(i.gamma), mask, s4[:2 * C], n, pg[0], pg[1], dx, x2g, mean2, invstd2, vec(i.gamma2),
                          s4[2 * C:], pg[2], pg[3], dx2)
        return (dx, dx2) + tuple(pg)
    dx, dx2, dg, db, dg2, db2 = twice(apply2)
    dymax = i.dy.abs().amax(0)
    sdx, sdx2 = i.gamma.abs() * f.invstd * dymax, i.gamma2.abs() * f.invstd2 * dymax
    c = s4.cpu()
    e = {"sg": bc.chan_err(c[:C], b.sg, b.abs_sg), "sgx": bc.chan_err(c[C:2 * C], b.sgx, b.abs_sgx),
         "sg_2": bc.chan_err(c[2 * C:3 * C], b2.sg, b2.abs_sg), "sgx_2": bc.chan_err(c[3 * C:], b2.sgx, b2.abs_sgx),
         "dx": bc.chan_err(mat(dx), b.dx, sdx), "dx_2": bc.chan_err(mat(dx2), b2.dx, sdx2),
         "dgamma": bc.chan_err(dg.cpu(), i.dgamma0 + b.sgx, b.abs_sgx), "dbeta": bc.chan_err(db.cpu(), i.dbeta0 + b.sg, b.abs_sg),
         "dgamma_2": bc.chan_err(dg2.cpu(), i.dgamma20 + b2.sgx, b2.abs_sgx), "dbeta_2": bc.chan_err(db2.cpu(), i.dbeta20 + b2.sg, b2.abs_sg)}
    fl0 = bc.floors(var)
    fl = {k: fl0[k.replace("_2", "")] for k in e}
    report(f"bn sweep {name}-{tag}: shared backward passes " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    check(e, fl, f"{name}-{tag} reduce2 / apply2")


@pytest.mark.parametrize("name", [c.name for c in bc.PLANE_CASES])
def test_bn_sweep_pair_planes(name, report):
    """pair planes where the channel vectors do not fill the block (CV = 2: rpb = 128; CV = 66: rpb = 3, 198 threads): the
    bound bounds, the decoded planes match the kernel's own fp32 output to 2^-21 of each element (the limits of
    tests/test_planes_gpu.py), and that fp32 output is held to float64"""
    case, var = bc.BY_NAME[name], bc.F32
    i, f = bc.inputs(name, "f32"), bc.truth(name, "f32")
    rows, C, n = case.rows, case.C, case.rows
    B = Bufs(case, var)
    xg, dyg = B.put(i.x, "f32"), B.put(i.dy, "f32")
    rg = B.put(i.r, "f32") if case.res else None
    gam, bet = vec(i.gamma), vec(i.beta)
    mean, invstd = ops.bn_finalize(ops.bn_stats(xg), n, bc.EPS, bc.MOMENTUM)
    ax, ag = ops.absmax(xg), ops.absmax(dyg)
    ar = ops.absmax(rg) if case.res else None
    mask0 = torch.full((rows * C // 4,), 0xFF, dtype=torch.uint8, device=DEV)
    y0 = ops.bn_apply(xg, mean, invstd, gam, bet, True, residual=rg, relu_mask=mask0, out=B.empty("f32", NAN))

    def planes(only):
        mask, bound, pl = torch.full_like(mask0, 0xFF), torch.zeros(1, dtype=torch.int32, device=DEV), B.empty("f32", NAN)
        y = ops.bn_apply(xg, mean, invstd, gam, bet, True, residual=rg, relu_mask=mask, amax_out=bound, planes=pl, planes_only=only,
                         amax_x=ax, amax_res=ar, out=None if only else B.empty("f32", NAN))
        return (pl, bound, mask) if only else (pl, bound, mask, y)
    pl, bound, mask, y = twice(lambda: planes(False))
    pl1, bound1, mask1 = twice(lambda: planes(True))
    assert same(y, y0) and same(mask, mask0) and same(pl1, pl) and same(bound1, bound) and same(mask1, mask0)

    def decoded_error(buf, bound_bits, own):
        bf = float(bound_bits.view(torch.float32))
        dec = from_planes(buf, 14 - int(np.floor(np.log2(bf))))
        big = own.abs().double() > bf * 2.0 ** -16
        return bf, float(own.abs().max()), float(((dec - own.double()).abs() / own.abs().double().clamp_min(1e-30))[big].max())
    bf, ymax, e_el = decoded_error(pl, bound, y0)
    assert bf >= ymax and bf < 64 * ymax and e_el < 2.0 ** -21, (bf, ymax, e_el)

    s2 = ops.bn_bwd_reduce(dyg, xg, None, mean, invstd, True, relu_mask=mask0)

    def bwd(as_planes):
        dgam, dbet, gb = vec(i.dgamma0), vec(i.dbeta0), torch.zeros(1, dtype=torch.int32, device=DEV)
        dres = B.empty("f32", NAN) if case.res else None
        dx = ops.bn_bwd_apply(dyg, xg, None, mean, invstd, gam, True, s2, n, dgam, dbet, dx=B.empty("f32", NAN), dres=dres,
                              relu_mask=mask0, amax_out=gb, dx_planes=as_planes, amax_x=ax if as_planes else None,
                              amax_dy=ag if as_planes else None)
        return dx, dres, dgam, dbet, gb
    dx0, dres0, dg0, db0, _ = twice(lambda: bwd(False))
    dxp, dres1, dg1, db1, gb = twice(lambda: bwd(True))
    assert same(dres1, dres0) and same(dg1, dg0) and same(db1, db0)
    bb, dmax, e_del = decoded_error(dxp, gb, dx0)
    assert bb >= dmax and bb < 64 * dmax and e_del < 2.0 ** -21, (bb, dmax, e_del)

    kpat, near = bc.mask_to_pattern(mask0.cpu(), rows, C), bc.near_zero(f.pre)
    assert float(near.double().mean()) <= bc.TIE_SHARE and bool(((kpat == (f.pre > 0)) | near).all())
    b = bc.backward(i, f, bc.pattern_with_ties(f.pre, kpat), torch.float64)
    s = bc.scales(i, f, b)
    e = {"y": bc.chan_err(mat(y0), f.y, s.y), "dx": bc.chan_err(mat(dx0), b.dx, s.dx)}
    report(f"bn sweep {name}: pair planes forward bound / max |y| {bf / ymax:.2f}, element error {e_el:.1e}; backward bound / max |dx| "
           f"{bb / dmax:.2f}, element error {e_del:.1e} (2^-21 = 4.8e-7); fp32 y {e['y']:.2e} dx {e['dx']:.2e} against float64")
    assert max(e.values()) < bc.FLOOR_F32


SIDE_RUNS = [pytest.param(c, v, id=f"{c.name}-{v.tag}") for c, v in bc.RUNS if c.name in ("idle_threads", "ragged_cgroup", "pitched")]


@pytest.mark.parametrize("case,var", SIDE_RUNS)
def test_bn_sweep_colsum_and_relu_mask_copy(case, var, report):
    """rcf_colsum_mp (beta 0 and 1) against float64 at the existing 1e-6; rcf_relu_mask_copy_mp (beta 0 and 1, pitched out) exactly:
    it is a select and at most one add"""
    i = bc.inputs(case.name, var.tag)
    rows, C = case.rows, case.C
    B = Bufs(case, var)
    dyg, mask = B.put(i.dy, var.ydt), i.mask4.to(DEV)
    truth, scale = bc.colsum(i.dy), bc.colsum(i.dy.abs())
    e = {}
    for beta in (0, 1):
        out = twice(lambda: ops.colsum(dyg, vec(i.dgamma0), beta=beta))
        e[f"colsum beta {beta}"] = bc.chan_err(out.cpu(), truth + beta * i.dgamma0, scale + beta * i.dgamma0.abs())
    pat = bc.mask_to_pattern(i.mask4, rows, C)
    dt = TORCH[var.ydt]
    sel = torch.where(pat, i.dy, torch.zeros(())).to(dt)
    old = i.dres0.to(dt)
    wide = []
    for beta in (0, 1):
        def copy():
            big = torch.full((case.N, case.H, case.W, C + 12), bc.FILL, dtype=dt, device=DEV)
            out = big[..., 4:4 + C]
            out.copy_(old.reshape(out.shape)) if beta else out.fill_(NAN)
            ops.relu_mask_copy(dyg, mask, out=out, beta=beta)
            return big
        big = twice(copy)
        want = (sel.float() + old.float()).to(dt) if beta else sel
        assert torch.equal(big[..., 4:4 + C].cpu().reshape(rows, C), want), f"relu_mask_copy beta {beta}"
        wide.append(big)
    assert all(bool((b[..., :4] == bc.FILL).all()) and bool((b[..., 4 + C:] == bc.FILL).all()) for b in wide) and B.guards_intact()
    report(f"bn sweep {case.name}-{var.tag}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()) + "; relu_mask_copy exact (beta 0 and 1)")
    assert max(e.values()) < 1e-6


# ------------------------------------------------------------------------------------------ the reductions' second stage
CHUNKS = (1, 7, 8, 31, 32, 33, 127, 128, 129, 255, 256, 257, 1023, 1024, 2047, 2048, 2049, 3210)


@pytest.mark.parametrize("n", [8, 96, 512, 1024, 4096])
def test_sum_partials_f64(n, report):
    """rcf_sum_partials_f64 on random partials of mixed sign, with a scratch buffer (groups launch from 256 rows) and with none:
    |err_i| <= chunks 2^-52 sum_k |p_ki| (each of the < chunks float64 additions rounds by at most 2^-53 of a partial sum no larger
    than sum_k |p_ki| (1 + chunks 2^-53))"""
    g = torch.Generator().manual_seed(n)
    full = torch.randn(max(CHUNKS), n, generator=g, dtype=torch.float64) * torch.exp2(6 * torch.rand(max(CHUNKS), 1, generator=g, dtype=torch.float64))
    full_g = full.to(DEV)
    scratch = torch.empty(64 * n, dtype=torch.float64, device=DEV)
    worst = 0.0
    for chunks in CHUNKS:
        p = full_g[:chunks]
        truth, mag = full[:chunks].sum(0), full[:chunks].abs().sum(0)
        for sc in (scratch, None):
            def run():
                out = torch.full((n + 32,), bc.FILL, dtype=torch.float64, device=DEV)
                ops.call("rcf_sum_partials_f64", c_void_p(p.data_ptr()), chunks, n, c_void_p(out.data_ptr()),
                         None if sc is None else c_void_p(sc.data_ptr()), ops._stream())
                return out
            out = twice(run).cpu()
            assert bool((out[n:] == bc.FILL).all()), "elements beyond n were written"
            ratio = float(((out[:n] - truth).abs() / (chunks * 2.0 ** -52 * mag)).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, (chunks, n, sc is not None, ratio)
    report(f"sum_partials_f64 n={n}: {len(CHUNKS)} chunk counts x (scratch, none), worst error / bound {worst:.3f}")


@pytest.mark.parametrize("H,W,lo,hi", [(199, 211, 256, 1023), (331, 431, 1024, 1 << 30)])
def test_conv_fused_finalize_long_tile_lists(H, W, lo, hi, report):
    """rcf_sum_partials_bn behind ops.conv2d_fwd_stats(..., bn=layer): a 1x1 64 -> 64 conv whose list of row tiles is 256 .. 1023
    long (sum_finalize_kernel<8>) and >= 1024 long (groups launch + finalize).  The tile count is OBSERVED: the statistics
    workspace is filled with NaN before the call and the conv writes one row of 2 Cout partial sums per row tile from its start
    (the groups launch, when taken, adds its 64 group rows right behind them)."""
    g = torch.Generator().manual_seed(H)
    Cin = Cout = 64
    x = torch.randn(1, H, W, Cin, generator=g).to(DEV)
    w = (torch.randn(Cout, Cin, 1, 1, generator=g) / 8).to(DEV).contiguous(memory_format=torch.channels_last)
    count = H * W
    s = ops._conv_shape(x.shape, Cin, w, 1, 0, 1, nt_cols=Cout)
    need = _lib.load().rcf_conv2d_fwd_stats_workspace_bytes(ctypes.byref(s))
    ws = ops.workspace(need, x.device)

    def written_rows():
        rowsw = ~torch.isnan(ws[:need].view(torch.float64).reshape(-1, 2 * Cout)).any(1)
        k = int(rowsw.sum())
        assert bool(rowsw[:k].all()), "the written partial rows are not a prefix of the workspace"
        return k
    bn = torch.nn.BatchNorm2d(Cout).to(DEV)
    rm0, rv0 = torch.randn(Cout, generator=g), torch.rand(Cout, generator=g) + 0.5
    bn.running_mean.copy_(rm0)
    bn.running_var.copy_(rv0)
    nbt0 = int(bn.num_batches_tracked)
    ws.fill_(0xFF)
    y, (mean, invstd, cnt) = ops.conv2d_fwd_stats(x, w, bn=bn)
    tiles = written_rows() - (64 if hi > 1023 else 0)
    assert lo <= tiles <= hi and cnt == count, tiles
    ws.fill_(0xFF)
    y1, sums = ops.conv2d_fwd_stats(x, w)
    assert written_rows() == tiles + (64 if hi > 1023 else 0) and torch.equal(y, y1)
    yd = y.double().cpu().reshape(-1, Cout)
    t_sum, t_sq, t_abs = yd.sum(0), (yd * yd).sum(0), yd.abs().sum(0)
    e_sums = max(bc.chan_err(sums[:Cout].cpu(), t_sum, t_abs), bc.chan_err(sums[Cout:].cpu(), t_sq, t_sq))
    m = t_sum / count
    var = ((yd - m) ** 2).sum(0) / count
    assert bool((m.abs() <= var.sqrt()).all()), "inputs: |mean| <= std, so the error of the sums at most doubles through the subtraction"
    istd = 1.0 / torch.sqrt(var + bn.eps)
    ulp = torch.tensor(np.spacing(m.abs().float().numpy()), dtype=torch.float64)
    d_mean = (mean.double().cpu() - m).abs()
    e_mean = float((d_mean / (5e-7 * t_abs / count + ulp)).max())
    rm = 0.9 * rm0.double() + 0.1 * m
    rv = 0.9 * rv0.double() + 0.1 * var * count / (count - 1)
    e_is, e_rv = bc.chan_err(invstd.cpu(), istd, istd), bc.chan_err(bn.running_var.cpu(), rv, rv)
    e_rm = bc.chan_err(bn.running_mean.cpu(), rm, rm.abs())
    report(f"conv-fused finalize {H}x{W}: {tiles} row tiles; sums {e_sums:.2e}, mean error / (5e-7 mean|y| + ulp) {e_mean:.3f}, invstd {e_is:.2e} "
           f"running_var {e_rv:.2e} running_mean {e_rm:.2e}")
    assert e_sums < 5e-7 and e_mean <= 1.0 and e_is < 2e-6 and e_rv < 2e-6 and e_rm < 2e-6
    assert int(bn.num_batches_tracked) == nbt0 + 1


# ------------------------------------------------------------------------------------------------------------ refusals
def test_bn_family_refuses_what_it_cannot_do():
    """every one of these is answered with a status before anything is launched, and the output buffers keep their fill"""
    g = torch.Generator().manual_seed(1)
    N, H, W, C = 2, 5, 7, 16
    rows = N * H * W
    t = lambda *s, dt=torch.float32: torch.randn(*s, generator=g).to(DEV).to(dt)
    x, dy = t(N, H, W, C), t(N, H, W, C)
    mean, invstd, gam, bet = t(C), t(C).abs() + 0.5, t(C), t(C)
    outs = []

    def out(*shape, dtype=torch.float32):
        o = torch.full(shape, bc.FILL, dtype=dtype, device=DEV)
        outs.append(o)
        return o
    einval, ews = dict(match="status -1"), dict(match="status -2")
    P = lambda v: c_void_p(v.data_ptr())
    lib = _lib.load()
    need = lib.rcf_bn_stats_workspace_bytes(rows, C)
    ws, sums = torch.empty(2 * need, dtype=torch.uint8, device=DEV), out(4 * C, dtype=torch.float64)
    st = ops._stream()
    mask = torch.zeros(rows * C // 4, dtype=torch.uint8, device=DEV)
    s2 = torch.zeros(2 * C, dtype=torch.float64, device=DEV)

    # C % 4 != 0
    x6 = t(N, H, W, 6)
    with pytest.raises(_lib.RcfHipError, **einval):
        ops.call("rcf_bn_stats_mp", P(x6), _lib.F32, rows, 6, 8, P(sums), P(ws), need, st)
    with pytest.raises(_lib.RcfHipError, **einval):
        ops.bn_apply(x6, mean, invstd, gam, bet, True, out=out(N, H, W, 6))
    with pytest.raises(_lib.RcfHipError, **einval):
        ops.call("rcf_colsum_mp", P(x6), _lib.F32, rows, 6, 8, P(out(C)), 0, P(ws), need, st)
    # a pitch not divisible by 4
    x50 = t(N, H, W, 50)[..., :C]
    with pytest.raises(_lib.RcfHipError, **einval):
        ops.bn_stats(x50)
    with pytest.raises(_lib.RcfHipError, **einval):
        ops.bn_apply(x50, mean, invstd, gam, bet, True, out=out(N, H, W, C))
    with pytest.raises(_lib.RcfHipError, **einval):
        ops.bn_apply(x, mean, invstd, gam, bet, True, out=out(N, H, W, 50)[..., :C])
    with pytest.raises(_lib.RcfHipError, **einval):
        ops.bn_bwd_apply(dy, x50, None, mean, invstd, gam, False, s2, rows, None, None, dx=out(N, H, W, C))
    # pitch < C
    with pytest.raises(_lib.RcfHipError, **einval):
        ops.call("rcf_bn_stats_mp", P(x), _lib.F32, rows, C, C - 4, P(sums), P(ws), need, st)
    with pytest.raises(_lib.RcfHipError, **einval):
        ops.call("rcf_colsum_mp", P(x), _lib.F32, rows, C, C - 4, P(out(C)), 0, P(ws), need, st)
    # count = 0
    with pytest.raises(_lib.RcfHipError, **einval):
        ops.call("rcf_bn_finalize_f32", P(s2), 0.0, C, 1e-5, 0.1, P(out(C)), P(out(C)), None, None, st)
    with pytest.raises(_lib.RcfHipError, **einval):
        ops.bn_bwd_apply(dy, x, None, mean, invstd, gam, False, s2, 0, out(C), out(C), dx=out(N, H, W, C))
    # a workspace one byte short
    with pytest.raises(_lib.RcfHipError, **ews):
        ops.call("rcf_bn_stats_mp", P(x), _lib.F32, rows, C, C, P(sums), P(ws), need - 1, st)
    with pytest.raises(_lib.RcfHipError, **ews):
        ops.call("rcf_colsum_mp", P(x), _lib.F32, rows, C, C, P(out(C)), 0, P(ws), need - 1, st)
    with pytest.raises(_lib.RcfHipError, **ews):
        ops.call("rcf_bn_bwd_reduce_mp", P(dy), _lib.F32, C, P(x), _lib.F32, C, None, 0, rows, C, P(mean), P(invstd), 0, None, None, H * W,
                 P(sums), P(ws), need - 1, 0, st)
    with pytest.raises(_lib.RcfHipError, **ews):
        ops.call("rcf_bn_bwd_reduce2_mp", P(dy), _lib.F32, C, P(x), _lib.F32, C, P(x), C, rows, C, P(mean), P(invstd), P(mean), P(invstd),
                 P(mask), P(sums), P(ws), 2 * need - 1, 0, st)
    # ReLU with neither y nor the sign bits
    with pytest.raises(_lib.RcfHipError, **einval):
        ops.bn_bwd_reduce(dy, x, None, mean, invstd, True)
    with pytest.raises(_lib.RcfHipError, **einval):
        ops.bn_bwd_apply(dy, x, None, mean, invstd, gam, True, s2, rows, out(C), out(C), dx=out(N, H, W, C))
    # pair planes: with a per-channel dropout scale; with C % 8 == 4
    ax, bound = ops.absmax(x), out(1, dtype=torch.int32)
    with pytest.raises(_lib.RcfHipError, **einval):
        ops.bn_apply(x, mean, invstd, gam, bet, True, chan_scale=t(N, C), out=out(N, H, W, C), relu_mask=mask, amax_out=bound,
                     planes=out(N, H, W, C), amax_x=ax)
    x20 = t(N, H, W, 20)
    with pytest.raises(_lib.RcfHipError, **einval):
        ops.bn_apply(x20, t(20), t(20), t(20), t(20), True, out=out(N, H, W, 20), amax_out=bound, planes=out(N, H, W, 20), amax_x=ops.absmax(x20))
    # a residual norm without a residual
    with pytest.raises(_lib.RcfHipError, **einval):
        ops.bn_apply(x, mean, invstd, gam, bet, True, out=out(N, H, W, C), res_norm=(mean, invstd, gam, bet))
    # the shared backward reduction with mixed storage types
    with pytest.raises(_lib.RcfHipError, **einval):
        ops.bn_bwd_reduce2(dy.to(torch.bfloat16), x, x, mean, invstd, mean, invstd, mask)
    torch.cuda.synchronize()
    assert all(bool((o == bc.FILL).all()) for o in outs), "a refused call wrote to an output"
