"""The pooling, resize and layout kernels (csrc/spatial.hip) against a float64 restatement at the edges of their dispatch and
launch geometry (tests/spatial_cases.py; conditioning of every case: tests/test_spatial_sweep_cpu.py).  Resize errors are taken
PER ELEMENT against the rounding bound of that element on the cases whose float32 source positions are exact, and per image
against the project's floors (2e-5 fp32, 5e-3 stored 16-bit) on the others; the maximum of a pooling window, the layout kernels,
the copies and the rectangle split are compared for equal bits.  Output buffers start as NaN where the kernel must write them,
gradients hold NaN where it must not read them, guard channels of pitched buffers hold 7.0 and must keep it."""
import contextlib
from ctypes import c_void_p

import pytest
import torch

import rcf_amd  # noqa: F401  (package alias)
import spatial_cases as sc
from rcf_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
TORCH = sc.TORCH


def storage(dt):
    """the library that stores dt as its 16-bit type"""
    return ops.half_storage(torch.float16) if dt == "f16" else contextlib.nullcontext()


def P(t):
    return None if t is None else c_void_p(t.data_ptr())


def same(a, b):
    """bit-equal, NaN == NaN"""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def veq(a, b):
    """equal in value with NaN == NaN (and -0 == 0)"""
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0))


class Bufs:
    """device NHWC operands: contiguous, or channel slices [..., 8:8 + C] of FILL-ed buffers `pitch` wide whose guard channels
    are checked at the end"""

    def __init__(self, pitch):
        self.pitch, self.wide = pitch, []

    def full(self, shape, dt, fill):
        if not self.pitch:
            return torch.full(shape, fill, dtype=TORCH[dt], device=DEV)
        big = torch.full(tuple(shape[:3]) + (self.pitch,), sc.FILL, dtype=TORCH[dt], device=DEV)
        self.wide.append((big, shape[3]))
        v = big[..., sc.SLICE0:sc.SLICE0 + shape[3]]
        v.fill_(fill)
        return v

    def put(self, t64, dt):
        v = self.full(tuple(t64.shape), dt, 0.0)
        v.copy_(t64.to(TORCH[dt]))
        return v

    def guards_intact(self):
        return all(bool((b[..., :sc.SLICE0] == sc.FILL).all()) and bool((b[..., sc.SLICE0 + C:] == sc.FILL).all()) for b, C in self.wide)


# ============================================================================================================ resize, NHWC
@pytest.mark.parametrize("c,dt,pitch,frame", sc.PARAMS_FWD)
def test_resize_forward_vs_float64(c, dt, pitch, frame, report):
    x64 = sc.resize_inputs(c.name, dt)[0]
    ref, mass = sc.resize_fwd_truth(c.name, dt)
    B = Bufs(pitch)
    xg = B.put(x64, dt)

    def run(fr, x=xg):
        out = B.full((x.shape[0], c.Ho, c.Wo, c.C), dt, NAN)
        with storage(dt):
            ops.resize_nhwc_fwd(x, (c.Ho, c.Wo), c.align, out=out, frame=fr)
        return out
    out = run(frame)
    got = out.double().cpu()
    M = sc.frame_mask(c.Ho, c.Wo, max(frame, 0))
    assert bool(torch.isnan(got[:, ~M]).all()), "an output pixel off the frame was written"
    m = sc.resize_margins(c, dt, got, ref, mass, mask=M)
    branch = sc.fwd_branch(c, dt, pitch, frame)
    note = ""
    if frame == -1 and c.name == "fb_general_2x":
        # the fallback against the exact-2x kernel on the same data in two halves of the batch
        assert sc.fwd_branch(c, dt, pitch, 0)[0] == "2x"
        h = c.N // 2
        assert same(out[:h], run(0, xg[:h])) and same(out[h:], run(0, xg[h:])), "the fallback differs from the exact-2x kernel"
        note = "; bit-equal to the 2x kernel on two halves"
    elif frame == -1:
        assert sc.fwd_branch(c, dt, pitch, 0)[0] == "2x" and same(out, run(0)), "the general kernel differs from the exact-2x kernel"
        note = "; bit-equal to the 2x kernel"
    assert B.guards_intact(), "a guard channel of a pitched buffer was written"
    report(f"spatial sweep resize fwd {sc.run_id(c, dt, pitch, frame)}: {branch[0]} kernel ({branch[1]}, V {branch[2]}), "
           f"{'exact' if c.exact else 'inexact'}, worst error / bound {m:.3f}{note}")
    assert m <= 1.0


@pytest.mark.parametrize("c,dt,pitch,frame,beta", sc.PARAMS_BWD)
def test_resize_backward_vs_float64(c, dt, pitch, frame, beta, report):
    _, dy64, old64 = sc.resize_inputs(c.name, dt)
    dx64, mass0, terms0 = sc.resize_bwd_truth(c.name, dt, frame)
    ref, mass, terms = sc.with_beta(dx64, mass0, terms0, old64, beta)
    fr = max(frame, 0)
    B = Bufs(pitch)
    dyg = B.put(dy64, dt)
    if fr > 0:
        dyg[:, ~sc.frame_mask(c.Ho, c.Wo, fr).to(DEV)] = NAN                     # off the frame the gradient must not be read

    def run(f):
        dx = B.put(old64, dt) if beta else B.full(tuple(old64.shape), dt, NAN)
        with storage(dt):
            ops.resize_nhwc_bwd(dyg, (c.Hi, c.Wi), c.align, out=dx, beta=beta, frame=f)
        return dx
    dx = run(frame)
    got = dx.double().cpu()
    m = sc.resize_margins(c, dt, got, ref, mass, terms)
    none = terms0 == 0                                                           # input pixels no term reaches
    if c.exact and beta:
        assert torch.equal(got[:, none], old64[:, none]), "an input pixel that receives nothing lost its prior value"
    if c.exact and not beta:
        assert not got[:, none].any(), "an input pixel that receives nothing is not zero"
    branch = sc.bwd_branch(c, dt, pitch, frame, beta)
    note = ""
    if frame == -1:
        assert sc.bwd_branch(c, dt, pitch, 0, beta)[0] == "2x" and same(dx, run(0)), "the general kernel differs from the exact-2x kernel"
        note = "; bit-equal to the 2x kernel"
    assert B.guards_intact(), "a guard channel of a pitched buffer was written"
    report(f"spatial sweep resize bwd {sc.run_id(c, dt, pitch, frame, beta)}: {branch[0]} kernel ({branch[1]}, V {branch[2]}, tc {branch[3]}), "
           f"{'exact' if c.exact else 'inexact'}, terms up to {int(terms.max())}, untouched pixels {int(none.sum())}, "
           f"worst error / bound {m:.3f}{note}")
    assert m <= 1.0


@pytest.mark.parametrize("name,planes,Hi,Wi,Ho,Wo,align", sc.NCHW, ids=[n[0] for n in sc.NCHW])
def test_resize_nchw_vs_float64(name, planes, Hi, Wi, Ho, Wo, align, report):
    x = sc.nchw_input(name, planes, Hi, Wi)
    ref, mass = sc.resize_fwd_ref(x.double().reshape(-1, Hi, Wi, 1), Ho, Wo, align)
    xg = x.to(DEV)
    out = torch.full(planes + (Ho, Wo), NAN, device=DEV)
    ops.call("rcf_resize_bilinear_nchw_f32", P(xg), P(out), xg.numel() // (Hi * Wi), Hi, Wi, Ho, Wo, int(align), ops._stream())
    got = out.double().cpu().reshape(-1, Ho, Wo, 1)
    if name == "davis":
        assert got.numel() > sc.TRIP
        m = sc.image_margin(got, ref, sc.FLOOR_F32)
    else:
        m = sc.elem_margin(got, ref, sc.fwd_bound(mass, ref, "f32"))
    report(f"spatial sweep resize nchw {name}: {got.numel()} outputs, worst error / bound {m:.3f}")
    assert m <= 1.0


# ================================================================================================================ max-pool
def pool_fwd(xg):
    N, H, W, C = xg.shape
    Ho, Wo = sc.pool_out(H), sc.pool_out(W)
    y = torch.full((N, Ho, Wo, C), NAN, dtype=xg.dtype, device=DEV)
    am = torch.full((N, Ho, Wo, C), 0xFF, dtype=torch.uint8, device=DEV)
    ops.call("rcf_maxpool3x3s2_fwd_mp", P(xg), P(y), ops._dt(xg), P(am), N, H, W, C, Ho, Wo, ops._stream())
    return y, am


def pool_bwd(dyg, am, H, W):
    N, Ho, Wo, C = dyg.shape
    dx = torch.full((N, H, W, C), NAN, dtype=dyg.dtype, device=DEV)
    ops.call("rcf_maxpool3x3s2_bwd_mp", P(dyg), P(am), P(dx), ops._dt(dyg), N, H, W, C, Ho, Wo, ops._stream())
    return dx


def pool_check(x64, dt, seed, backward=True, forward=True):
    """one pooling round trip against the reference: (worst backward error / bound, share of tied windows)"""
    N, H, W, C = x64.shape
    y_ref, code = sc.maxpool_ref(x64)
    with storage(dt):
        if forward:
            y, am = pool_fwd(x64.to(TORCH[dt]).to(DEV))
            assert veq(y.double().cpu(), y_ref), "the window maximum differs"
            assert torch.equal(am.cpu(), code), "the argmax code differs from the first-valid-tap / strict > / NaN rule"
        else:
            am = code.to(DEV)
        if not backward:
            return 0.0
        g = torch.Generator().manual_seed(seed)
        dy64 = sc.stored(torch.randn(y_ref.shape, generator=g), dt)
        dx = pool_bwd(dy64.to(TORCH[dt]).to(DEV), am, H, W)
    dx_ref, mass, terms = sc.maxpool_bwd_ref(dy64, code, H, W)
    return sc.elem_margin(dx.double().cpu(), dx_ref, sc.pool_bwd_bound(mass, terms, dx_ref, dt))


@pytest.mark.parametrize("kind", sc.POOL_KINDS)
@pytest.mark.parametrize("H,W", sc.POOL_HW)
def test_maxpool_vs_float64(H, W, kind, report):
    worst = {}
    for dt in ("f32", "bf16", "f16"):
        worst[dt] = pool_check(sc.pool_input(H, W, kind, dt), dt, seed=H * W)
    report(f"spatial sweep maxpool {H}x{W} {kind}: maxima and argmax codes bit-equal in fp32 / bf16 / fp16; backward error / bound "
           + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0


def test_maxpool_second_trip(report):
    """more than 8192 x 256 work items: the backward in fp32 on codes from the reference, the forward in bf16"""
    N, H, W, C, dt = sc.POOL_BIG_BWD
    g = torch.Generator().manual_seed(7)
    m = pool_check(torch.randn(N, H, W, C, generator=g), dt, seed=8, forward=False)
    N, H, W, C, dt = sc.POOL_BIG_FWD
    x = torch.randn(N, H, W, C, generator=g).to(TORCH[dt])
    pool_check(x, dt, seed=9, backward=False)
    report(f"spatial sweep maxpool second trip: backward {sc.POOL_BIG_BWD[:4]} error / bound {m:.3f}; forward bf16 {sc.POOL_BIG_FWD[:4]} bit-equal")
    assert m <= 1.0


# ================================================================================================================== layout
def to_nhwc(xg, cpad):
    N, C, H, W = xg.shape
    out = torch.full((N, H, W, cpad), NAN, device=DEV)
    ops.call("rcf_nchw_to_nhwc_f32", P(xg), P(out), N, C, H, W, cpad, ops._stream())
    return out


def to_nchw(xg, C):
    N, H, W, _ = xg.shape
    out = torch.full((N, C, H, W), NAN, device=DEV)
    ops.call("rcf_nhwc_to_nchw_f32", P(xg), ops.pitch_of(xg), P(out), N, C, H, W, ops._stream())
    return out


def test_layout_kernels_bit_equal(report):
    g = torch.Generator().manual_seed(11)
    for N, C, H, W, cpad in sc.LAYOUT + [sc.LAYOUT_BIG_TO]:
        x = torch.randn(N, C, H, W, generator=g)
        y = to_nhwc(x.to(DEV), cpad)
        assert same(y.cpu(), sc.nchw_to_nhwc_ref(x, cpad)), (N, C, H, W, cpad)           # pad channels exactly +0
        back = to_nchw(y, C)                                                             # x_pitch = Cpad > C
        assert same(back.cpu(), x), (N, C, H, W, cpad)
    N, C, H, W, pitch = sc.LAYOUT_BIG_BACK
    big = torch.randn(N, H, W, pitch, generator=g)
    assert same(to_nchw(big.to(DEV)[..., :C], C).cpu(), sc.nhwc_to_nchw_ref(big, C))
    report(f"spatial sweep layout: {len(sc.LAYOUT)} (C, Cpad) pairs both ways bit-equal; {sc.LAYOUT_BIG_TO[2] * sc.LAYOUT_BIG_TO[3]} pixels to "
           f"NHWC and {N * C * H * W} elements back take the second trip")


# ================================================================================================================== copies
@pytest.mark.parametrize("sk,dk,h16", [(s, d, h) for h in ("bf16", "f16") for s, d in sc.COPY_PAIRS if h == "bf16" or "h16" in (s, d)])
def test_copy2d_bit_equal(sk, dk, h16, report):
    sdt, ddt = (h16 if sk == "h16" else "f32"), (h16 if dk == "h16" else "f32")
    g = torch.Generator().manual_seed(13)
    n = 0
    with storage(h16):
        for rows, C, sp, dp in sc.COPY_SHAPES:
            for beta in (0, 1):
                src = torch.randn(rows, sp, generator=g).to(TORCH[sdt])
                dst = torch.randn(rows, dp, generator=g).to(TORCH[ddt])
                want = dst.clone()
                want[:, :C] = sc.copy2d_ref(src[:, :C].float(), dst[:, :C].float(), beta, TORCH[ddt])
                sg, dg = src.to(DEV), dst.to(DEV)
                ops.copy2d(sg, sp, dg, dp, rows, C, beta=beta)
                assert same(dg.cpu(), want), (sk, dk, rows, C, sp, dp, beta)             # columns C .. pitch keep what they held
                n += 1
    report(f"spatial sweep copy2d {sdt} -> {ddt}: {n} (shape, beta) runs bit-equal to one rounding of the fp32 sum")


def test_copy2d_second_trip(report):
    rows, C = sc.COPY_BIG
    g = torch.Generator().manual_seed(14)
    src, dst = torch.randn(rows, C, generator=g).bfloat16(), torch.randn(rows, C, generator=g).bfloat16()
    dg = dst.to(DEV)
    ops.copy2d(src.to(DEV), C, dg, C, rows, C, beta=1)
    assert same(dg.cpu(), sc.copy2d_ref(src.float(), dst.float(), 1, torch.bfloat16))
    report(f"spatial sweep copy2d second trip: {rows * C // 4} items, bf16 accumulate, bit-equal")


@pytest.mark.parametrize("b", [pytest.param(b, id=b.name) for b in sc.BATCHED])
def test_copy2d_batched_bit_equal(b, report):
    g = torch.Generator().manual_seed(15)
    n = 0
    for dt in ("f32", "bf16"):
        for beta in (0, 1):
            src = torch.randn(b.src_len, generator=g).to(TORCH[dt])
            dst = torch.randn(b.dst_len, generator=g).to(TORCH[dt])
            want = sc.batched_ref(src.float(), dst.float(), b, beta, TORCH[dt])
            sg, dg = src.to(DEV), dst.to(DEV)
            ops.copy2d_batched(sg[b.src[0]:], b.src[1], b.src[2:], dg[b.dst[0]:], b.dst[1], b.dst[2:], b.rows, b.C, (b.n0, b.n1), beta=beta)
            assert same(dg.cpu(), want), (b.name, dt, beta)                               # elements outside the copies keep what they held
            n += 1
    report(f"spatial sweep copy2d_batched {b.name}: {b.n0} x {b.n1} copies of {b.rows} x {b.C}, strides src {b.src[2:]} dst {b.dst[2:]}: "
           f"{n} (type, beta) runs bit-equal")


# ============================================================================================================= split_rect
def split(xg, rect, inside, outside):
    N, H, W, C = xg.shape
    ins = torch.full_like(xg, NAN) if inside else None
    outs = torch.full_like(xg, NAN) if outside else None
    ops.call("rcf_split_rect_mp", P(xg), P(ins), P(outs), ops._dt(xg), N, H, W, C, *rect, ops._stream())
    return ins, outs


def test_split_rect_bit_equal(report):
    g = torch.Generator().manual_seed(16)
    n = 0
    for dt in ("f32", "bf16"):
        x = torch.randn(*sc.SPLIT_SHAPE, generator=g).to(TORCH[dt])
        xg = x.to(DEV)
        for rect in sc.SPLIT_RECTS:
            wi, wo = sc.split_rect_ref(x, rect)
            for inside, outside in ((True, True), (True, False), (False, True)):
                ins, outs = split(xg, rect, inside, outside)
                assert (ins is None) == (not inside) and (outs is None) == (not outside)
                assert (ins is None or same(ins.cpu(), wi)) and (outs is None or same(outs.cpu(), wo)), (dt, rect, inside, outside)
                n += 1
    N, H, W, C, rect = sc.SPLIT_BIG
    x = torch.randn(N, H, W, C, generator=g).bfloat16()
    ins, _ = split(x.to(DEV), rect, True, False)
    assert same(ins.cpu(), sc.split_rect_ref(x, rect)[0])
    report(f"spatial sweep split_rect: {n} (type, rectangle, outputs) runs on {sc.SPLIT_SHAPE} and {N * H * W * C // 4} items (second trip) bit-equal")


# ================================================================================================================ refusals
def test_spatial_kernels_refuse_what_they_cannot_do():
    """every one of these is answered with RCF_EINVAL before anything is launched, and the output buffers keep their fill"""
    g = torch.Generator().manual_seed(17)
    t = lambda *s: torch.randn(*s, generator=g).to(DEV)
    outs = []

    def out(*shape, dtype=torch.float32):
        o = torch.full(shape, sc.FILL, dtype=dtype, device=DEV)
        outs.append(o)
        return o
    st = ops._stream()
    F32 = _lib.F32

    def refused(name, *args):
        with pytest.raises(_lib.RcfHipError, match="status -1"):
            ops.call(name, *args)
    N, Hi, Wi, Ho, Wo, C = 2, 4, 6, 8, 12, 8
    x, dy = t(N, Hi, Wi, C), t(N, Ho, Wo, C)
    fwd = lambda xp, xpitch, yp, ypitch, C_, frame, Ho_=Ho: refused("rcf_resize_bilinear_nhwc_fwd_mp", xp, xpitch, yp, ypitch, F32, N, Hi, Wi, Ho_, Wo,
                                                                     C_, 0, frame, st)
    bwd = lambda gp, gpitch, dp, dpitch, C_, frame, Ho_=Ho: refused("rcf_resize_bilinear_nhwc_bwd_mp", gp, gpitch, dp, dpitch, F32, 1, N, Hi, Wi, Ho_,
                                                                     Wo, C_, 0, frame, st)
    y, dx = out(N, Ho, Wo, C), out(N, Hi, Wi, C)
    # C % 4, a pitch % 4
    fwd(P(x), 8, P(y), 8, 6, 0)
    bwd(P(dy), 8, P(dx), 8, 6, 0)
    fwd(P(x), 10, P(y), 8, C, 0)
    fwd(P(x), 8, P(y), 10, C, 0)
    bwd(P(dy), 10, P(dx), 8, C, 0)
    bwd(P(dy), 8, P(dx), 10, C, 0)
    # 2 * frame >= Ho (and Wo), frame < -1, sizes that are not positive
    fwd(P(x), 8, P(y), 8, C, 4)
    bwd(P(dy), 8, P(dx), 8, C, 4)
    fwd(P(x), 8, P(y), 8, C, 6)
    fwd(P(x), 8, P(y), 8, C, -2)
    bwd(P(dy), 8, P(dx), 8, C, -2)
    fwd(P(x), 8, P(y), 8, C, 0, 0)
    bwd(P(dy), 8, P(dx), 8, C, 0, 0)
    # null pointers
    fwd(None, 8, P(y), 8, C, 0)
    fwd(P(x), 8, None, 8, C, 0)
    bwd(None, 8, P(dx), 8, C, 0)
    bwd(P(dy), 8, None, 8, C, 0)
    refused("rcf_resize_bilinear_nchw_f32", None, P(y), 2, 4, 4, 8, 8, 0, st)
    refused("rcf_resize_bilinear_nchw_f32", P(x), None, 2, 4, 4, 8, 8, 0, st)
    refused("rcf_resize_bilinear_nhwc_fwd_frame_f32", P(x), 8, P(y), 8, N, Hi, Wi, Ho, Wo, C, 0, 0, st)      # the frame entry without a frame
    refused("rcf_resize_bilinear_nhwc_bwd_frame_f32", P(dy), 8, P(dx), 8, 1, N, Hi, Wi, Ho, Wo, C, 0, 0, st)

    # max-pool: sizes that do not match H, W (forward and backward), sizes that are not positive, C % 4, null pointers
    H, W = 7, 10
    ph, pw = sc.pool_out(H), sc.pool_out(W)
    px, pdy = t(N, H, W, C), t(N, ph, pw, C)
    py, pam, pdx = out(N, ph, pw, C), out(N, ph, pw, C, dtype=torch.uint8), out(N, H, W, C)
    pf = lambda xp, yp, ap, *dims: refused("rcf_maxpool3x3s2_fwd_mp", xp, yp, F32, ap, *dims, st)
    pb = lambda gp, ap, dp, *dims: refused("rcf_maxpool3x3s2_bwd_mp", gp, ap, dp, F32, *dims, st)
    for dims in ((N, H, W, C, ph + 1, pw), (N, H, W, C, ph, pw - 1), (N, H, W, C, ph - 1, pw), (N, H, W, C, H, W), (0, H, W, C, ph, pw),
                 (N, 0, W, C, 0, pw), (N, H, -1, C, ph, 0), (N, H, W, 0, ph, pw), (N, H, W, 6, ph, pw)):
        pf(P(px), P(py), P(pam), *dims)
        pb(P(pdy), P(pam), P(pdx), *dims)
    pf(None, P(py), P(pam), N, H, W, C, ph, pw)
    pf(P(px), None, P(pam), N, H, W, C, ph, pw)
    pf(P(px), P(py), None, N, H, W, C, ph, pw)
    pb(None, P(pam), P(pdx), N, H, W, C, ph, pw)
    pb(P(pdy), None, P(pdx), N, H, W, C, ph, pw)
    pb(P(pdy), P(pam), None, N, H, W, C, ph, pw)

    # split_rect: a rectangle outside the image, an empty one, C % 4, null pointers
    sx, si, so = t(N, H, W, C), out(N, H, W, C), out(N, H, W, C)
    for rect in ((0, 0, H + 1, W), (0, 0, H, W + 1), (1, 0, H, W), (0, 1, H, W), (-1, 0, 2, 2), (0, -1, 2, 2), (2, 2, 0, 3), (2, 2, 3, 0)):
        refused("rcf_split_rect_mp", P(sx), P(si), P(so), F32, N, H, W, C, *rect, st)
    refused("rcf_split_rect_mp", P(sx), P(si), P(so), F32, N, H, W, 6, 0, 0, 2, 2, st)
    refused("rcf_split_rect_mp", None, P(si), P(so), F32, N, H, W, C, 0, 0, 2, 2, st)
    refused("rcf_split_rect_mp", P(sx), None, None, F32, N, H, W, C, 0, 0, 2, 2, st)

    # copies: C % 4, a pitch or a batch stride % 4, no rows, n0 * n1 > 65535, null pointers
    cs, cd = t(16, 16), out(16, 16)
    cp = lambda sp_, spitch, dp_, dpitch, rows, C_: refused("rcf_copy2d_mp", sp_, F32, spitch, dp_, F32, dpitch, rows, C_, 0, st)
    cp(P(cs), 16, P(cd), 16, 16, 6)
    cp(P(cs), 14, P(cd), 16, 16, 8)
    cp(P(cs), 16, P(cd), 14, 16, 8)
    cp(P(cs), 16, P(cd), 16, 0, 8)
    cp(None, 16, P(cd), 16, 16, 8)
    cp(P(cs), 16, None, 16, 16, 8)
    refused("rcf_copy2d_mp", P(cs), 7, 16, P(cd), F32, 16, 16, 8, 0, st)                  # a storage type that does not exist
    cb = lambda sp_, dp_, spitch, sb0, sb1, db0, db1, C_, n0, n1, rows=2: refused("rcf_copy2d_batched_mp", sp_, spitch, sb0, sb1, dp_, 16, db0, db1, F32,
                                                                                  rows, C_, 0, n0, n1, st)
    cb(P(cs), P(cd), 16, 32, 8, 32, 8, 8, 256, 256)                                       # 65536 copies
    cb(P(cs), P(cd), 16, 32, 8, 32, 8, 8, 0, 2)
    cb(P(cs), P(cd), 16, 32, 8, 32, 8, 6, 2, 2)
    cb(P(cs), P(cd), 14, 32, 8, 32, 8, 8, 2, 2)
    cb(P(cs), P(cd), 16, 30, 8, 32, 8, 8, 2, 2)
    cb(P(cs), P(cd), 16, 32, 6, 32, 8, 8, 2, 2)
    cb(P(cs), P(cd), 16, 32, 8, 30, 8, 8, 2, 2)
    cb(P(cs), P(cd), 16, 32, 8, 32, 6, 8, 2, 2)
    cb(P(cs), P(cd), 16, 32, 8, 32, 8, 8, 2, 2, 0)
    cb(None, P(cd), 16, 32, 8, 32, 8, 8, 2, 2)
    cb(P(cs), None, 16, 32, 8, 32, 8, 8, 2, 2)

    # layout: Cpad % 4, Cpad < C, x_pitch < C, null pointers
    lx, ly = t(2, 3, 4, 4), out(2, 4, 4, 8)
    refused("rcf_nchw_to_nhwc_f32", P(lx), P(ly), 2, 3, 4, 4, 6, st)
    refused("rcf_nchw_to_nhwc_f32", P(lx), P(ly), 2, 5, 4, 4, 4, st)
    refused("rcf_nchw_to_nhwc_f32", None, P(ly), 2, 3, 4, 4, 4, st)
    refused("rcf_nchw_to_nhwc_f32", P(lx), None, 2, 3, 4, 4, 4, st)
    refused("rcf_nhwc_to_nchw_f32", P(lx), 2, P(ly), 2, 3, 4, 4, st)
    refused("rcf_nhwc_to_nchw_f32", None, 4, P(ly), 2, 3, 4, 4, st)
    refused("rcf_nhwc_to_nchw_f32", P(lx), 4, None, 2, 3, 4, 4, st)
    torch.cuda.synchronize()
    assert all(bool((o == sc.FILL).all()) for o in outs), "a refused call wrote to an output"
