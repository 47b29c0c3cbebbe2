"""The tap list of the forward / data-gradient tile kernel (csrc/igemm_conv.hip igemm_conv_x3_kernel, csrc/region_order.h): a tile
drops the K-steps of taps none of its rows can read, a frame region is walked by depth, and the data gradient can take its
source as zero off a border frame (rcf_conv2d_dgrad_region_band_f32).

Every case is compared twice: bit for bit (torch.equal) against the same call under RCF_CONV_NO_TAP_SKIP -- the terms that are
dropped are exact zeros -- and against a float64 CPU conv at the tolerance of tests/test_kernels_gpu.py::test_conv_fp16_pairs
(rms error < max(4 x torch's fp32 error, 5e-7), largest element error in units of the result's rms < max(4 x torch's, 1e-5)),
both taken over the pixels the launch writes.  Pixels off the region must keep what they held."""
import functools

import pytest
import torch
import torch.nn.functional as F

import rcf_amd  # noqa: F401  (package alias)
from rcf_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def to_nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous().to(DEV)


def from_nhwc(y):
    return y.permute(0, 3, 1, 2).cpu()


def cl_weight(w):
    return w.to(DEV).contiguous(memory_format=torch.channels_last)


def frame_mask(H, W, t):
    """[H, W] bool: the border frame of thickness t (t = 0: everything)"""
    m = torch.ones(H, W, dtype=torch.bool)
    if t > 0:
        m[t:H - t, t:W - t] = False
    return m


@functools.lru_cache(maxsize=None)
def problem(N, Cin, Cout, k, stride, pad, dil, H, W, dy_frame):
    """seeded operands and the float64 / torch-fp32 results of one conv, computed once and shared; dy_frame > 0: the output
    gradient the references see is zero off that frame (`dy_full` keeps the interior)"""
    g = torch.Generator().manual_seed(1000 * Cin + 10 * Cout + H + dy_frame)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    xd, wd = x.double().requires_grad_(True), w.double().requires_grad_(True)
    yref = F.conv2d(xd, wd, None, stride=stride, padding=pad, dilation=dil)
    dy_full = torch.randn(yref.shape, generator=g)
    dy = dy_full * frame_mask(yref.shape[2], yref.shape[3], dy_frame) if dy_frame else dy_full
    yref.backward(dy.double())
    x32, w32 = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y32 = F.conv2d(x32, w32, None, stride=stride, padding=pad, dilation=dil)
    y32.backward(dy)
    return dict(x=x, w=w, dy=dy, dy_full=dy_full, y=yref.detach(), dx=xd.grad, dw=wd.grad, y32=y32.detach(), dx32=x32.grad,
                dw32=w32.grad)


def check64(name, got, ref, ref32, mask, report):
    """`got` against float64 over the pixels of `mask` ([H, W]), torch's fp32 result as the yardstick"""
    sel = lambda t: t.detach().double().cpu()[:, :, mask]
    a, b, c = sel(got), sel(ref), sel(ref32)
    scale = float((b ** 2).mean().sqrt()) + 1e-300
    e, r = float(((a - b) ** 2).mean().sqrt()) / scale, float(((c - b) ** 2).mean().sqrt()) / scale
    em, rm = float((a - b).abs().max()) / scale, float((c - b).abs().max()) / scale
    report(f"tap skip {name}: rms error vs float64 {e:.2e} (torch fp32 {r:.2e}), max element / rms {em:.2e} ({rm:.2e})")
    assert e < max(4 * r, 5e-7)
    assert em < max(4 * rm, 1e-5)


def both(fn, extra=0):
    """fn() with the tap list and under RCF_CONV_NO_TAP_SKIP (`extra`: flags both runs carry)"""
    try:
        ops.set_conv_flags(extra)
        new = fn()
        ops.set_conv_flags(extra | _lib.CONV_NO_TAP_SKIP)
        old = fn()
    finally:
        ops.set_conv_flags(0)
    torch.cuda.synchronize()
    return new, old


GRID = (2, 30, 37)            # 1066 (frame 13) / 742 (frame 7) rows per image: tiles straddle strips, corners and images; an M tail


@pytest.mark.parametrize("beta", [0, 1])
@pytest.mark.parametrize("Cin,Cout", [(256, 256), (256, 64), (64, 64)])
def test_dgrad_frame(Cin, Cout, beta, report):
    """data gradient on the 13-frame of a dilation-6 conv whose dy lives on the 7-frame (decode_head2's band): the 128 x 256 tile in
    the chunked (Cout 256) and the natural (Cout 64) K order, and the 64-row tile (Cin 64); plain call on a dy with a zeroed
    interior, and the dy_band = 7 entry on the whole dy -- all four launches must write the same bits"""
    N, H, W = GRID
    P = problem(N, Cin, Cout, 3, 1, 6, 6, H, W, 7)
    wg, gz, gf = cl_weight(P["w"]), to_nhwc(P["dy"]), to_nhwc(P["dy_full"])
    assert float(gf[:, 7:-7, 7:-7].abs().max()) > 0 and float(gz[:, 7:-7, 7:-7].abs().max()) == 0
    aw, ag = ops.absmax(ops.weight_rsck(wg)), ops.absmax(gf)          # the layer's range is the whole gradient's
    region = (0, 0, H, W, 13)
    g = torch.Generator().manual_seed(3)
    init = to_nhwc(torch.randn(N, Cin, H, W, generator=g))

    def run(dy, band):
        def f():
            pt = ops.weight_pairs_t(wg, aw)
            return ops.conv2d_dgrad(dy, wg, (N, H, W, Cin), 1, 6, 6, out=init.clone(), beta=beta, region=region, amax=(ag, aw),
                                    w_pairs_t=pt, dy_band=band)
        return both(f)
    new, old = run(gz, 0)
    bnew, bold = run(gf, 7)
    assert torch.equal(new, old)
    assert torch.equal(bnew, old) and torch.equal(bold, old)
    m = frame_mask(H, W, 13)
    off = (~m).to(DEV)
    assert torch.equal(new[:, off], init[:, off])                      # off the region: untouched
    base = from_nhwc(init).double() if beta else 0.0
    base32 = from_nhwc(init) if beta else 0.0
    check64(f"dgrad frame 13 {Cout}->{Cin} beta {beta}", from_nhwc(new), P["dx"] + base, P["dx32"] + base32, m, report)


@pytest.mark.parametrize("h2p", [False, True])
def test_fwd_frame(h2p, report):
    """forward on the 7-frame of the same grid, once on the tile kernel (tap list, frame by depth) and once on conv_h2p_kernel (no
    tap list, the row-major frame: the switch must not reach it)"""
    N, H, W = GRID
    P = problem(N, 256, 256, 3, 1, 6, 6, H, W, 7)
    xg, wg = to_nhwc(P["x"]), cl_weight(P["w"])
    ax, aw = ops.absmax(xg), ops.absmax(ops.weight_rsck(wg))
    init = torch.full((N, H, W, 256), 3.0, device=DEV)
    region = (0, 0, H, W, 7)

    def f():
        return ops.conv2d_fwd(xg, wg, None, 1, 6, 6, out=init.clone(), region=region, amax=(ax, aw), w_pairs=ops.weight_pairs(wg, aw))
    new, old = both(f, _lib.CONV_H2P_ALWAYS if h2p else _lib.CONV_H2P_NEVER)
    assert torch.equal(new, old)
    m = frame_mask(H, W, 7)
    off = (~m).to(DEV)
    assert torch.equal(new[:, off], init[:, off])
    check64(f"fwd frame 7 h2p={h2p}", from_nhwc(new), P["y"], P["y32"], m, report)


def test_wgrad_frame(report):
    """weight gradient over the 7-frame: its pixel order is its summation order and stays; the switch must not move a bit"""
    N, H, W = GRID
    P = problem(N, 256, 256, 3, 1, 6, 6, H, W, 7)
    xg, wg, gg = to_nhwc(P["x"]), cl_weight(P["w"]), to_nhwc(P["dy_full"])
    ax, ag = ops.absmax(xg), ops.absmax(gg)

    def f():
        return ops.conv2d_wgrad(xg, gg, wg, torch.zeros_like(wg), 1, 6, 6, beta=0, region=(0, 0, H, W, 7), amax=(ax, ag))
    new, old = both(f)
    assert torch.equal(new, old)
    e = float(((new.double().cpu() - P["dw"]) ** 2).mean().sqrt() / (P["dw"] ** 2).mean().sqrt())
    r = float(((P["dw32"].double() - P["dw"]) ** 2).mean().sqrt() / (P["dw"] ** 2).mean().sqrt())
    report(f"tap skip wgrad frame 7: rms error vs float64 {e:.2e} (torch fp32 {r:.2e})")
    assert e < max(4 * r, 5e-7)


def test_whole_tensor_short_image(report):
    """whole tensor, 10 x 40 at dilation 6: on lines 4 and 5 both outer tap rows leave the image; forward and data gradient.
    (Whole-tensor launches keep the plain K loop by the launch rule -- the list measured slower there -- so this holds trivially
    today; it stays as the case the rule would have to pass if it is widened.)"""
    N, H, W, C = 2, 10, 40, 256
    P = problem(N, C, C, 3, 1, 6, 6, H, W, 0)
    xg, wg, gg = to_nhwc(P["x"]), cl_weight(P["w"]), to_nhwc(P["dy"])
    ax, aw, ag = ops.absmax(xg), ops.absmax(ops.weight_rsck(wg)), ops.absmax(gg)
    m = frame_mask(H, W, 0)
    y, y0 = both(lambda: ops.conv2d_fwd(xg, wg, None, 1, 6, 6, amax=(ax, aw), w_pairs=ops.weight_pairs(wg, aw)), _lib.CONV_H2P_NEVER)
    assert torch.equal(y, y0)
    check64("fwd 10x40 d6", from_nhwc(y), P["y"], P["y32"], m, report)
    dx, dx0 = both(lambda: ops.conv2d_dgrad(gg, wg, (N, H, W, C), 1, 6, 6, amax=(ag, aw), w_pairs_t=ops.weight_pairs_t(wg, aw)),
                   _lib.CONV_H2P_NEVER)
    assert torch.equal(dx, dx0)
    check64("dgrad 10x40 d6", from_nhwc(dx), P["dx"], P["dx32"], m, report)


@pytest.mark.parametrize("case", [(2, 64, 128, 3, 2, 1, 1, 13, 18), (2, 64, 256, 1, 1, 0, 1, 13, 17)])
def test_plain_loop_paths(case, report):
    """a 3x3 stride-2 data gradient and a 1x1 conv keep the plain K loop: unchanged"""
    N, Cin, Cout, k, stride, pad, dil, H, W = case
    P = problem(N, Cin, Cout, k, stride, pad, dil, H, W, 0)
    xg, wg, gg = to_nhwc(P["x"]), cl_weight(P["w"]), to_nhwc(P["dy"])
    ax, aw, ag = ops.absmax(xg), ops.absmax(ops.weight_rsck(wg)), ops.absmax(gg)
    m = frame_mask(H, W, 0)
    dx, dx0 = both(lambda: ops.conv2d_dgrad(gg, wg, (N, H, W, Cin), stride, pad, dil, amax=(ag, aw)))
    assert torch.equal(dx, dx0)
    check64(f"dgrad {case}", from_nhwc(dx), P["dx"], P["dx32"], m, report)
    y, y0 = both(lambda: ops.conv2d_fwd(xg, wg, None, stride, pad, dil, amax=(ax, aw)))
    assert torch.equal(y, y0)
    check64(f"fwd {case}", from_nhwc(y), P["y"], P["y32"], frame_mask(y.shape[1], y.shape[2], 0), report)


def test_refused_dgrad_band_writes_nothing():
    """a source frame on a 7x7 filter is refused -- 49 taps do not fit the tap list's 32-bit mask -- by the launch plan, before the
    pre-pass that would transpose the weights into the caller's workspace: the status is RCF_EINVAL, and neither dx nor the workspace
    (exactly rcf_conv2d_dgrad_workspace_bytes, so the refusal is not a workspace one) is written.  The entry point is called
    directly: ops.call would raise on the status"""
    from ctypes import byref, c_void_p, sizeof
    lib = _lib.load()
    N, H, W, C, k = 1, 12, 12, 16, 7
    s = _lib.ConvShape(N, H, W, C, H, W, C, k, k, 1, 3, 1, C, C, *([None] * 8), 0, sizeof(_lib.ConvShape))
    need = lib.rcf_conv2d_dgrad_workspace_bytes(byref(s))
    assert need == k * k * C * C * 4
    g = torch.Generator().manual_seed(5)
    dy, w = torch.randn(N, H, W, C, generator=g).to(DEV), torch.randn(C, k, k, C, generator=g).to(DEV)
    dx, ws = torch.full((N, H, W, C), -7.25, device=DEV), torch.full((need,), 0xA5, dtype=torch.uint8, device=DEV)
    dx0, ws0 = dx.clone(), ws.clone()
    ptr = lambda t: c_void_p(t.data_ptr())
    st = lib.rcf_conv2d_dgrad_region_band_f32(ptr(dy), ptr(w), ptr(dx), byref(s), None, 1, 0, ptr(ws), need, None)
    torch.cuda.synchronize()
    assert st == -1                                                       # RCF_EINVAL
    assert torch.equal(dx.view(torch.int32), dx0.view(torch.int32)) and torch.equal(ws, ws0)
    # ... and the same call without the source frame runs (the refusal is the frame's, not the shape's)
    assert lib.rcf_conv2d_dgrad_region_band_f32(ptr(dy), ptr(w), ptr(dx), byref(s), None, 0, 0, ptr(ws), need, None) == 0
    torch.cuda.synchronize()
    assert not torch.equal(dx, dx0) and not torch.equal(ws, ws0)
