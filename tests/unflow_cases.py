"""Cases and the reference of the flow-loss kernels (csrc/unflow.hip, rcf_amd.unFlowLoss): models/amd/flow_loss.py and
models/amd/loss_blocks.py restated term by term.

Shared by tests/test_unflow_cpu.py (the restatement equals the reference-made fixture and its analytic gradients equal autograd of
its own forward) and tests/test_unflow_gpu.py (the kernels and the module against it).  torch on the CPU; nothing of the HIP
package enters except the pure geometry query that places the case table on the kernel's seams.

Sample positions come from tests/warp_cases.py (`make_taps`: float32, in the order of utils/warp_utils.py and grid_sample), so
floors, clips and tap choices are the kernels' own and the bilinear kinks need no tie set; `pdt=np.float64` runs the position in
float64 as the reference's float64 run does and exists to be compared with the fixture.  Everything after the position runs in
`dt`: float64 is the reference; float32 is "what the same arithmetic does in float32 on the CPU", whose error against float64
(`e32`) scales the gradient bound of the GPU test.

The forward is written so that torch autograd can differentiate it with respect to `delta`, a shift of the un-normalised sample
coordinate (d position / d flow = 1 where the clip leaves the coordinate alone, 0 where it clips); the ANALYTIC gradient next to
it is the form the kernels implement: the L1 sign, the three SSIM coefficient planes per window
    dL/dx_q = sum_{p contains q} A_p + x_q sum B_p + y_q sum C_p,
the ternary gather (a pixel is the neighbour of up to 8 interior centres and a centre itself), then the tap differences.

The non-smooth points form the TIE set excluded from gradient comparisons (never from a forward value): a pixel with
|im - rec| < 1e-6 in a channel where occ > 0 (under a zero mask the term is identically zero, not a kink), a pixel covered by a
window whose SSIM distance lies within 1e-4 of 0 or 1 (a window wholly under a zero mask is constant, not a kink), a flow element in a difference under 1e-6 that is not exactly 0 (smoothness; sign(0) = 0 is checked).  MAX_TIE_SHARE
caps its share of a case; cases whose construction puts whole regions on a kink (`grad=False`) are compared on the forward only.
"""
import dataclasses
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

import warp_cases as wc

U = 2.0 ** -24
TIE_L1, TIE_SSIM, TIE_SMOOTH = 1e-6, 1e-4, 1e-6
MAX_TIE_SHARE = 0.02
SCALAR_RTOL = wc.PHOTO_RTOL                # 1e-4: the suite's limit on the photometric loss
GRAD_FACTOR, GRAD_ULPS = 6.0, 16.0         # max|err| <= max(6 e32, 16 u max|g64|)
C1, C2 = 0.01 ** 2, 0.03 ** 2
GRAY = (0.2989, 0.5870, 0.1140)
T = torch.from_numpy


class Cfg(dict):
    """attribute access and keys(), like the reference's Objectview / EasyDict"""
    __getattr__ = dict.__getitem__


def fcn_cfg(**over):
    """models/fcn_head.py:73-85"""
    c = dict(alpha=10, ssim_sz=1, occ_from_back=True, type="unflow", w_l1=0.15, w_scales=[1.0, 1.0, 1.0, 1.0, 0.0],
             w_sm_scales=[1.0, 0.0, 0.0, 0.0, 0.0], w_real_smooth=0., w_ssim=0.85, w_ternary=0.0, warp_pad="border", with_bk=True)
    c.update(over)
    return Cfg(c)


GOLDEN_SHAPE, GOLDEN_LEVELS, GOLDEN_STRIDE = (2, 32, 48), 5, 7       # tests/golden/unflow.npz (make_golden_unflow.py)


def golden_cfgs():
    """name, cfg, pyramid depth.  The last: 3 levels, the deepest at which a 5 x 5 window still fits (8 x 12)"""
    return [("fcn", fcn_cfg(), 5),
            ("bidirectional", fcn_cfg(occ_from_back=False), 5),
            ("ternary_smooth1", fcn_cfg(w_ternary=1.0, w_real_smooth=50.0, w_sm_scales=[1.0, 1.0, 0.0, 0.0, 0.0]), 5),
            ("ssim2_smooth2", fcn_cfg(ssim_sz=2, smooth_2nd=True, w_real_smooth=50.0, w_scales=[1.0, 1.0, 1.0],
                                      w_sm_scales=[1.0, 1.0, 1.0]), 3)]


def geometry():
    from rcf_amd import _lib
    lib = _lib.load()
    return tuple(int(lib.rcf_unflow_geometry(k)) for k in range(3))          # tile rows, tile columns, largest md


# ============================================================================================================ small pieces
def nearest_index(out, inp):
    """torch's `nearest`: min(floor(dst * float32(in) / out), in - 1), float32"""
    scale = np.float32(inp) / np.float32(out)
    return np.minimum(np.floor(np.arange(out, dtype=np.float32) * scale).astype(np.int64), inp - 1)


def nearest_mask(occ0, h, w):
    """occ0 numpy [B, 1, H0, W0] -> [B, 1, h, w]"""
    return occ0[:, :, nearest_index(h, occ0.shape[2])][:, :, :, nearest_index(w, occ0.shape[3])]


def area_ref(x, h, w):
    """adaptive average of numpy [B, C, H, W] in float64 -> (out, mass, n): rows floor(i H / h) .. ceil((i + 1) H / h)"""
    B, C, H, W = x.shape
    x = x.astype(np.float64)
    out, mass, n = np.zeros((B, C, h, w)), np.zeros((B, C, h, w)), np.zeros((h, w))
    for i in range(h):
        ys, ye = (i * H) // h, -((-(i + 1) * H) // h)
        for j in range(w):
            xs, xe = (j * W) // w, -((-(j + 1) * W) // w)
            win = x[:, :, ys:ye, xs:xe]
            n[i, j] = (ye - ys) * (xe - xs)
            out[:, :, i, j] = win.sum((2, 3)) / n[i, j]
            mass[:, :, i, j] = np.abs(win).sum((2, 3)) / n[i, j]
    return out, mass, n


def area_bound(mass, n):
    """n - 1 additions, one division, one store"""
    return (n + 2) * U * mass


def _gather4(other, taps):
    B, C, h, w = other.shape
    flat = other.reshape(B, C, h * w)
    out = []
    for k in range(4):
        idx = T(taps.idx[k].reshape(B, 1, h * w)).expand(B, C, h * w)
        v = torch.gather(flat, 2, idx).reshape(B, C, h, w)
        out.append(torch.where(T(taps.ok[k][:, None]), v, torch.zeros((), dtype=other.dtype)))
    return out


def warp_t(other, taps, delta=None):
    """-> rec, the four tap values, wx, wy ([B, 1, h, w]); delta [B, 2, h, w] shifts the coordinate where the clip lets it move"""
    dt = other.dtype
    v = _gather4(other, taps)
    wx, wy = T(taps.wx)[:, None].to(dt), T(taps.wy)[:, None].to(dt)
    if delta is not None:
        wx = wx + delta[:, 0:1] * T(taps.live_x[:, None]).to(dt)
        wy = wy + delta[:, 1:2] * T(taps.live_y[:, None]).to(dt)
    rec = v[0] * ((1 - wy) * (1 - wx)) + v[1] * ((1 - wy) * wx) + v[2] * (wy * (1 - wx)) + v[3] * (wy * wx)
    return rec, v, wx, wy


def box(a, md):
    """mean over the (2 md + 1)^2 window of every pixel that has one: [B, C, h - 2 md, w - 2 md]"""
    K = 2 * md + 1
    h, w = a.shape[2:]
    s = 0
    for dy in range(K):
        for dx in range(K):
            s = s + a[:, :, dy:dy + h - 2 * md, dx:dx + w - 2 * md]
    return s / (K * K)


def ssim_parts(x, y, md):
    mx, my = box(x, md), box(y, md)
    vx, vy, cxy = box(x * x, md) - mx * mx, box(y * y, md) - my * my, box(x * y, md) - mx * my
    a1, a2 = 2 * mx * my + C1, 2 * cxy + C2
    b1, b2 = mx * mx + my * my + C1, vx + vy + C2
    S = a1 * a2 / (b1 * b2)
    return dict(mx=mx, my=my, a1=a1, a2=a2, b1=b1, b2=b2, S=S, raw=(1 - S) / 2)


def gray(a):
    return (a[:, 0] * GRAY[0] + a[:, 1] * GRAY[1] + a[:, 2] * GRAY[2]) * 255


def _tern_pairs(h, w):
    c = (slice(None), slice(1, h - 1), slice(1, w - 1))
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            yield c, (slice(None), slice(1 + dy, h - 1 + dy), slice(1 + dx, w - 1 + dx))


def ternary_t(x, y):
    """the ternary distance of the interior pixels [B, h - 2, w - 2]; the 1-pixel border is masked to zero by the reference"""
    ix, iy = gray(x), gray(y)
    h, w = ix.shape[1:]
    acc = 0
    for c, nb in _tern_pairs(h, w):
        d1, d2 = ix[nb] - ix[c], iy[nb] - iy[c]
        u = d1 / torch.sqrt(0.81 + d1 * d1) - d2 / torch.sqrt(0.81 + d2 * d2)
        acc = acc + u * u / (0.1 + u * u)
    return acc / 9


# ====================================================================================================== photometric term
@dataclasses.dataclass
class Photo:
    loss: float
    l1: float
    ssim: float
    tern: float
    occ_mean: float
    dflow: np.ndarray = None         # analytic, [B, 2, h, w]
    tie: np.ndarray = None           # [B, h, w] bool


def photo_forward(im, other, taps, occ, md, w_l1, w_ssim, w_tern, delta=None):
    """torch, in im.dtype.  -> (loss, dict of the pieces)"""
    rec, v, wx, wy = warp_t(other, taps, delta)
    B, _, h, w = im.shape
    x, y = rec * occ, im * occ
    zero = torch.zeros((), dtype=im.dtype)
    l1 = ((im - rec).abs() * occ).mean() if w_l1 > 0 else zero
    sp = ssim_parts(x, y, md) if w_ssim > 0 else None
    ss = torch.clamp(sp["raw"], 0, 1).mean() if w_ssim > 0 else zero
    te = ternary_t(x, y).sum() / (B * h * w) if w_tern > 0 else zero
    om = occ.float().mean().to(im.dtype)      # the reference's masks are .float() whatever the run's type: the mean is float32's
    loss = (w_l1 * l1 * (w_l1 > 0) + w_ssim * ss * (w_ssim > 0) + w_tern * te * (w_tern > 0)) / om
    return loss, dict(rec=rec, v=v, wx=wx, wy=wy, x=x, y=y, sp=sp, l1=l1, ssim=ss, tern=te, om=om)


def photo_analytic(im, other, taps, occ, md, w_l1, w_ssim, w_tern):
    """float64: the forward's pieces, the gradient in the form the kernels implement, and the tie set"""
    with torch.no_grad():
        loss, p = photo_forward(im, other, taps, occ, md, w_l1, w_ssim, w_tern)
        B, _, h, w = im.shape
        rec, x, y = p["rec"], p["x"], p["y"]
        drec = torch.zeros_like(rec)
        tie = torch.zeros(B, h, w, dtype=torch.bool)
        if w_l1 > 0:
            drec += -torch.sign(im - rec) * occ * (w_l1 / (3 * B * h * w))
            tie |= (((im - rec).abs() < TIE_L1) & (occ > 0)).any(1)
        if w_ssim > 0:
            sp = p["sp"]
            n = (2 * md + 1) ** 2
            hh, ww = h - 2 * md, w - 2 * md
            count = 3 * B * hh * ww
            live = ((sp["raw"] > 0) & (sp["raw"] < 1)).double()
            wgt = -0.5 * live * w_ssim / count
            a1, a2, b1, b2, S, mx, my = (sp[k] for k in ("a1", "a2", "b1", "b2", "S", "mx", "my"))
            A = wgt * (2 * my * (a2 - a1) / (b1 * b2) - 2 * mx * S * (1 / b1 - 1 / b2)) / n
            Bc = -2 * wgt * S / (b2 * n)
            Cc = 2 * wgt * a1 / (b1 * b2 * n)
            near = ((sp["raw"].abs() < TIE_SSIM) | ((sp["raw"] - 1).abs() < TIE_SSIM)).any(1)
            near &= box(occ, md)[:, 0] > 0     # a window wholly under a zero mask has x = y = 0 whatever the flow: constant, no kink
            sa, sb, sc = torch.zeros_like(rec), torch.zeros_like(rec), torch.zeros_like(rec)
            for dy in range(2 * md + 1):
                for dx in range(2 * md + 1):
                    sl = (slice(None), slice(None), slice(dy, dy + hh), slice(dx, dx + ww))
                    sa[sl] += A
                    sb[sl] += Bc
                    sc[sl] += Cc
                    tie[:, dy:dy + hh, dx:dx + ww] |= near
            drec += occ * (sa + x * sb + y * sc)
        if w_tern > 0:
            ix, iy = gray(x), gray(y)
            dI = torch.zeros(B, h, w, dtype=torch.float64)
            for c, nb in _tern_pairs(h, w):
                d1, d2 = ix[nb] - ix[c], iy[nb] - iy[c]
                r1 = 0.81 + d1 * d1
                u = d1 / torch.sqrt(r1) - d2 / torch.sqrt(0.81 + d2 * d2)
                phi = (0.2 * u / (0.1 + u * u) ** 2) * (0.81 / r1 ** 1.5) / 9
                dI[nb] += phi                  # as the neighbour p + k of centre p
                dI[c] -= phi                   # as the centre itself
            k = 255 * w_tern / (B * h * w)
            drec += occ * k * dI[:, None] * torch.tensor(GRAY, dtype=torch.float64).view(1, 3, 1, 1)
        v, wx, wy = p["v"], p["wx"], p["wy"]
        gx = (drec * ((1 - wy) * (v[1] - v[0]) + wy * (v[3] - v[2]))).sum(1)
        gy = (drec * ((1 - wx) * (v[2] - v[0]) + wx * (v[3] - v[1]))).sum(1)
        zero = torch.zeros((), dtype=torch.float64)
        dflow = torch.stack([torch.where(T(taps.live_x), gx / p["om"], zero), torch.where(T(taps.live_y), gy / p["om"], zero)], 1)
    return Photo(float(loss), float(p["l1"]), float(p["ssim"]), float(p["tern"]), float(p["om"]), dflow.numpy(), tie.numpy())


def photo_autograd(im, other, taps, occ, md, w_l1, w_ssim, w_tern):
    """the forward in im.dtype and torch autograd's gradient with respect to the coordinate shift -> (loss, dflow numpy float64)"""
    B, _, h, w = im.shape
    delta = torch.zeros(B, 2, h, w, dtype=im.dtype, requires_grad=True)
    loss, _ = photo_forward(im, other, taps, occ, md, w_l1, w_ssim, w_tern, delta)
    loss.backward()
    return float(loss.detach()), delta.grad.double().numpy()


# ============================================================================================================ smoothness
def smooth_forward(flow, im, alpha, s, second):
    """loss_blocks.py smooth_grad_1st / smooth_grad_2nd of flow / s, torch in flow.dtype"""
    f = flow / s
    wx = torch.exp(-(im[:, :, :, 1:] - im[:, :, :, :-1]).abs().mean(1, keepdim=True) * alpha)
    wy = torch.exp(-(im[:, :, 1:] - im[:, :, :-1]).abs().mean(1, keepdim=True) * alpha)
    dx, dy = f[:, :, :, 1:] - f[:, :, :, :-1], f[:, :, 1:] - f[:, :, :-1]
    if not second:
        return (wx * dx.abs() / 2.).mean() / 2. + (wy * dy.abs() / 2).mean() / 2.
    dx2, dy2 = dx[:, :, :, 1:] - dx[:, :, :, :-1], dy[:, :, 1:] - dy[:, :, :-1]
    return (wx[:, :, :, 1:] * dx2.abs()).mean() / 2. + (wy[:, :, 1:, :] * dy2.abs()).mean() / 2.


def _near0(d):
    """under the tie threshold but not exactly 0: sign(0) = 0 is a decision everyone makes alike"""
    return (d.abs() < TIE_SMOOTH) & (d != 0)


def smooth_analytic(flow, im, alpha, s, second):
    """float64 -> (loss, dflow, tie [B, 2, h, w]): every difference pays its sign times its weight to the 2 (3) elements in it"""
    with torch.no_grad():
        loss = smooth_forward(flow, im, alpha, s, second)
        f = flow / s
        wx = torch.exp(-(im[:, :, :, 1:] - im[:, :, :, :-1]).abs().mean(1, keepdim=True) * alpha)
        wy = torch.exp(-(im[:, :, 1:] - im[:, :, :-1]).abs().mean(1, keepdim=True) * alpha)
        dx, dy = f[:, :, :, 1:] - f[:, :, :, :-1], f[:, :, 1:] - f[:, :, :-1]
        g = torch.zeros_like(flow)
        tie = torch.zeros(flow.shape, dtype=torch.bool)
        rx, ry = flow[:, :, :, 1:] - flow[:, :, :, :-1], flow[:, :, 1:] - flow[:, :, :-1]
        if not second:
            if dx.numel():
                tx = wx * torch.sign(dx) / (4 * dx.numel() * s)
                g[:, :, :, 1:] += tx
                g[:, :, :, :-1] -= tx
                k = (rx.abs() < TIE_SMOOTH) & (rx != 0)
                tie[:, :, :, 1:] |= k
                tie[:, :, :, :-1] |= k
            if dy.numel():
                ty = wy * torch.sign(dy) / (4 * dy.numel() * s)
                g[:, :, 1:] += ty
                g[:, :, :-1] -= ty
                k = (ry.abs() < TIE_SMOOTH) & (ry != 0)
                tie[:, :, 1:] |= k
                tie[:, :, :-1] |= k
        else:
            dx2, dy2 = dx[:, :, :, 1:] - dx[:, :, :, :-1], dy[:, :, 1:] - dy[:, :, :-1]
            if dx2.numel():
                tx = wx[:, :, :, 1:] * torch.sign(dx2) / (2 * dx2.numel() * s)
                g[:, :, :, 2:] += tx
                g[:, :, :, 1:-1] -= 2 * tx
                g[:, :, :, :-2] += tx
                k = _near0(rx[:, :, :, 1:] - rx[:, :, :, :-1])
                tie[:, :, :, 2:] |= k
                tie[:, :, :, 1:-1] |= k
                tie[:, :, :, :-2] |= k
            if dy2.numel():
                ty = wy[:, :, 1:, :] * torch.sign(dy2) / (2 * dy2.numel() * s)
                g[:, :, 2:] += ty
                g[:, :, 1:-1] -= 2 * ty
                g[:, :, :-2] += ty
                k = _near0(ry[:, :, 1:] - ry[:, :, :-1])
                tie[:, :, 2:] |= k
                tie[:, :, 1:-1] |= k
                tie[:, :, :-2] |= k
    return float(loss), g.numpy(), tie.numpy()


def smooth_autograd(flow, im, alpha, s, second):
    f = flow.clone().requires_grad_(True)
    loss = smooth_forward(f, im, alpha, s, second)
    loss.backward()
    return float(loss.detach()), f.grad.double().numpy()


# ====================================================================================================== the whole module
def masks_level0(flow, from_back, pdt=np.float32):
    """flow numpy float32 [B, 4, h, w] -> (occu_mask1, occu_mask2, tie1, tie2) numpy float64 / bool [B, 1, h, w]"""
    f12, f21 = np.ascontiguousarray(flow[:, :2]), np.ascontiguousarray(flow[:, 2:])
    if from_back:
        (m1, t1), (m2, t2) = wc.occ_backward_ref(f21, 0.2, pdt), wc.occ_backward_ref(f12, 0.2, pdt)
    else:
        (m1, t1), (m2, t2) = wc.occ_bidir_ref(f12, f21, pdt=pdt), wc.occ_bidir_ref(f21, f12, pdt=pdt)
    return 1 - m1, 1 - m2, t1, t2


def loss_ref(cfg, flows, target, dt=torch.float64, pdt=np.float32, analytic=True, masks=None):
    """flow_loss.py forward restated.  flows: list of numpy float32 [B, 4, h, w]; target numpy float32 [B, 6, H, W].
    -> dict(total, warp, smooth, absmean, mask1, mask2 (level 0), grads: list of [B, 4, h, w] float64 (None for a level of weight 0),
    ties: the same shape, bool).  analytic=True: float64 with the analytic gradients; False: the forward in dt with torch autograd.
    masks: (mask1, mask2) of level 0 to use instead of computing them (the GPU test hands over the kernels' own when a tie
    decides a pixel)"""
    md = int(cfg.ssim_sz)
    second = "smooth_2nd" in cfg.keys() and bool(cfg.smooth_2nd)
    wts = (md, float(cfg.w_l1), float(cfg.w_ssim), float(cfg.w_ternary))
    tgt = T(np.ascontiguousarray(target)).to(dt)
    m1 = m2 = None
    s = 1.0
    warp, smooth = 0.0, 0.0
    grads, ties = [], []
    leaves = []
    for i, fl in enumerate(flows):
        if cfg.w_scales[i] == 0:
            grads.append(None)
            ties.append(None)
            continue
        B, _, h, w = fl.shape
        if dt == torch.float64:
            im1, im2 = (T(area_ref(target[:, k:k + 3], h, w)[0]) for k in (0, 3))
        else:
            im1, im2 = F.interpolate(tgt[:, :3], (h, w), mode="area"), F.interpolate(tgt[:, 3:], (h, w), mode="area")
        if m1 is None:
            assert i == 0
            m1, m2 = masks if masks is not None else masks_level0(fl, cfg.occ_from_back, pdt)[:2]
            s = float(min(h, w))
        o1, o2 = T(nearest_mask(m1, h, w)).to(dt), T(nearest_mask(m2, h, w)).to(dt)
        g = np.zeros(fl.shape)
        tie = np.zeros(fl.shape, dtype=bool)
        lw, ls = [], []
        dirs = [(slice(0, 2), im1, im2, o1)] + ([(slice(2, 4), im2, im1, o2)] if cfg.with_bk else [])
        half = 0.5 if cfg.with_bk else 1.0
        for sl, im, other, occ in dirs:
            f = np.ascontiguousarray(fl[:, sl])
            taps = wc.make_taps(f, "border", pdt)
            ft = T(f).to(dt)
            if analytic:
                p = photo_analytic(im, other, taps, occ, *wts)
                lw.append(p.loss)
                g[:, sl] += p.dflow * (half * cfg.w_scales[i])
                tie[:, sl] |= p.tie[:, None]
                if cfg.w_real_smooth > 0:
                    l, gs, ts = smooth_analytic(ft, im, float(cfg.alpha), s, second)
                    ls.append(l)
                    g[:, sl] += gs * (half * cfg.w_sm_scales[i] * cfg.w_real_smooth)
                    if cfg.w_sm_scales[i] != 0:
                        tie[:, sl] |= ts
            else:
                delta = torch.zeros(B, 2, h, w, dtype=dt, requires_grad=True)
                fleaf = ft.clone().requires_grad_(True)
                leaves.append((i, sl, delta, fleaf))
                lw.append(photo_forward(im, other, taps, occ, *wts, delta)[0])
                if cfg.w_real_smooth > 0:
                    ls.append(smooth_forward(fleaf, im, float(cfg.alpha), s, second))
        warp = warp + sum(lw) * half * cfg.w_scales[i]
        if ls:
            smooth = smooth + sum(ls) * half * cfg.w_sm_scales[i]
        grads.append(g)
        ties.append(tie)
    smooth = cfg.w_real_smooth * smooth if cfg.w_real_smooth > 0 else 0.0
    total = warp + smooth
    if not analytic:
        total.backward()
        for i, sl, delta, fleaf in leaves:
            grads[i][:, sl] = delta.grad.double().numpy() + (fleaf.grad.double().numpy() if fleaf.grad is not None else 0.0)
    absmean = float(T(flows[0]).to(dt).abs().mean())
    _f = lambda v: float(v.detach()) if torch.is_tensor(v) else float(v)
    return dict(total=_f(total), warp=_f(warp), smooth=_f(smooth), absmean=absmean, mask1=m1, mask2=m2, grads=grads, ties=ties)


def grad_bound(e32, g64):
    return max(GRAD_FACTOR * e32, GRAD_ULPS * U * float(np.abs(g64).max()) if g64.size else 0.0)


def max_err(got, ref, tie=None):
    d = np.abs(np.asarray(got, dtype=np.float64) - ref)
    if tie is not None:
        d = np.where(tie, 0.0, d)
    if np.isnan(d).any():
        return float("inf")
    return float(d.max()) if d.size else 0.0


def rel_err(got, ref):
    """scalars: NaN equals NaN"""
    if math.isnan(ref) or math.isnan(got):
        return 0.0 if math.isnan(ref) and math.isnan(got) else float("inf")
    return abs(got - ref) / abs(ref) if ref != 0 else abs(got)


# =================================================================================================================== cases
def smooth_images(B, h, w, g, noise=0.04):
    """two frames [B, 3, h, w] float32 in [0, 1]: low-frequency waves plus a little noise, the second a shifted, dimmed first"""
    y, x = torch.arange(h).double()[:, None], torch.arange(w).double()[None, :]
    ph = 6.283 * torch.rand(B, 3, 1, 1, generator=g).double()
    fr = 0.15 + 0.25 * torch.rand(B, 3, 1, 1, generator=g).double()
    base = lambda sh: 0.5 + 0.3 * torch.sin(fr * (x + sh) + 0.7 * fr * y + ph) * torch.cos(0.11 * (y - sh))
    a = base(0.0) + noise * torch.randn(B, 3, h, w, generator=g).double()
    b = 0.95 * base(1.3) + noise * torch.randn(B, 3, h, w, generator=g).double()
    return a.clamp(0, 1).float().numpy(), b.clamp(0, 1).float().numpy()


@dataclasses.dataclass(frozen=True)
class Case:
    h: int
    w: int
    md: int = 1
    B: int = 2
    mask: str = "random"          # ones, random (~20 % zeros), zeros, tile (zero on the whole first tile)
    flow: str = "gauss"           # the kinds of tests/warp_cases.py::make_flow
    image: str = "smooth"         # smooth, const (a constant region in both frames)
    weights: tuple = (0.15, 0.85, 0.0)     # w_l1, w_ssim, w_ternary
    mask_size: tuple = None       # (H0, W0) of the level-0 mask when the level is a deeper one
    grad: bool = True             # False: the forward only (the construction puts whole regions on a kink)

    @property
    def name(self):
        wt = "-".join(f"{v:g}" for v in self.weights)
        ms = f"-from{self.mask_size[0]}x{self.mask_size[1]}" if self.mask_size else ""
        return f"{self.h}x{self.w}-md{self.md}-b{self.B}-{self.mask}-{self.flow}-{self.image}-w{wt}{ms}"

    @property
    def seed(self):
        return 7000 + 131 * self.h + 17 * self.w + self.md + 3 * len(self.name)


ALL_W = (0.15, 0.85, 1.0)


def _cases():
    TH, TW, _ = geometry()
    out = [Case(3, 3, weights=ALL_W), Case(3, 40, weights=ALL_W), Case(40, 3, weights=ALL_W),
           Case(5, 5, md=2), Case(7, 7, md=3, weights=ALL_W)]
    # the seams of the tile, under the narrowest and the widest halo
    seam = [(TH - 1, TW - 1), (TH, TW), (TH + 1, TW + 1), (2 * TH + 1, 2 * TW + 1)]
    out += [Case(h, w, md=1, weights=ALL_W) for h, w in seam]
    out += [Case(h, w, md=3, weights=ALL_W) for h, w in seam[1:]]
    out += [Case(TH + 1, TW + 1, md=2, weights=ALL_W)]
    out += [Case(TH + 1, TW + 1), Case(2 * TH + 1, 2 * TW + 1)]          # the FCNHead weights: L1 + SSIM 3 x 3, no ternary term
    # a deeper level: non-integer nearest indices into the level-0 mask
    out += [Case(4, 5, mask_size=(9, 11), weights=ALL_W)]
    # masks
    out += [Case(2 * TH + 1, 2 * TW + 1, mask=m, weights=ALL_W) for m in ("ones", "tile")]
    out += [Case(TH + 1, TW + 1, mask="zeros", weights=ALL_W, grad=False)]          # 0 / 0: NaN must equal NaN
    # flows: integer / half-pixel positions, out of the image on every side, far away, NaN
    out += [Case(TH + 1, TW + 1, flow=f, weights=ALL_W) for f in ("integer", "half", "edges", "far", "nan")]
    # sigma = 0: SSIM sits on its clamp over the whole region -- forward only
    out += [Case(2 * TH + 1, TW + 1, md=m, image="const", weights=ALL_W, grad=False) for m in (1, 3)]
    # each weight alone
    out += [Case(TH + 1, TW + 1, md=2, weights=wt) for wt in ((0.15, 0.0, 0.0), (0.0, 0.85, 0.0), (0.0, 0.0, 1.0))]
    return out


CASES = _cases()
SMOOTH_CASES = [(h, w, second) for second in (False, True) for h, w in ((3, 3), (3, 40), (40, 3), (9, 33), (17, 65))] + \
               [(2, 2, False), (2, 9, True), (1, 5, False)]         # the last three: an axis without a difference -> NaN
AREA_CASES = [(9, 11, 4, 5), (32, 48, 16, 24), (32, 48, 32, 48), (13, 17, 5, 3), (7, 5, 7, 2), (8, 8, 3, 3)]       # H, W, h, w


@functools.lru_cache(maxsize=None)
def inputs(c):
    g = torch.Generator().manual_seed(c.seed)
    B, h, w = c.B, c.h, c.w
    im, other = smooth_images(B, h, w, g)
    if c.image == "const":
        im[:, :, 2:h - 2, 3:w - 3] = np.float32(0.4)
        other[:, :, 1:h - 1, 1:w - 1] = np.float32(0.4)
    flow = wc.make_flow(wc.Case(h, w, 3, B, c.flow), g)
    if c.flow == "gauss":
        flow = (flow * np.float32(0.6)).astype(np.float32)
    H0, W0 = c.mask_size or (h, w)
    occ = (torch.rand(B, 1, H0, W0, generator=g) > (0.2 if c.mask in ("random", "tile") else -1.0)).float().numpy()
    if c.mask == "tile":
        TH, TW, _ = geometry()
        occ[:, :, :TH, :TW] = 0
    if c.mask == "zeros":
        occ[:] = 0
    return dict(im=im, other=other, flow=np.ascontiguousarray(flow, dtype=np.float32), occ=occ)


@functools.lru_cache(maxsize=None)
def photo_truth(c):
    """-> (Photo in float64 with the analytic gradient and the tie set, e32: the float32 CPU run's worst gradient error outside it,
    loss32)"""
    d = inputs(c)
    taps = wc.make_taps(d["flow"], "border")
    occ = nearest_mask(d["occ"], c.h, c.w)
    a = [T(d[k]).double() for k in ("im", "other")] + [taps, T(occ).double(), c.md] + list(c.weights)
    p = photo_analytic(*a)
    b = [T(d[k]) for k in ("im", "other")] + [taps, T(occ), c.md] + list(c.weights)
    with np.errstate(all="ignore"):
        loss32, g32 = photo_autograd(*b)
    e32 = max_err(g32, p.dflow, p.tie[:, None]) if c.grad else float("nan")
    return p, e32, loss32


def smooth_inputs(h, w, second):
    g = torch.Generator().manual_seed(500 + 31 * h + w + int(second))
    im, _ = smooth_images(2, h, w, g)
    flow = (torch.randn(2, 2, h, w, generator=g) * 1.5).numpy()
    if h * w > 20:
        flow[0, 0, 1, 1:3] = flow[0, 0, 1, 0]              # planted zero differences: sign(0) = 0
    return im, flow.astype(np.float32)


# module-level cases: name, cfg, pyramid sizes from (B, H, W)
def module_cases():
    TH, TW, _ = geometry()
    H, W = 4 * TH + 2, 2 * TW + 6
    return [
        ("fcn", fcn_cfg(), (2, H, W), 5),
        ("bidir_no_bk", fcn_cfg(occ_from_back=False, with_bk=False), (2, H, W), 5),
        ("ternary_smooth1", fcn_cfg(w_ternary=1.0, w_real_smooth=50.0, w_sm_scales=[1, 1, 0, 0, 0]), (2, H, W), 5),
        ("zero_in_the_middle", fcn_cfg(w_scales=[1.0, 0.0, 1.0, 0.0, 0.0], w_real_smooth=50.0, smooth_2nd=True, ssim_sz=2,
                                       w_sm_scales=[1.0, 1.0, 1.0, 0.0, 0.0]), (2, H, W), 4),
    ]


def pyramid_inputs(B, H, W, levels, seed, need_mask_mean=0.05):
    """smooth frames and smooth low-frequency forward / backward flows of a few pixels on a halving pyramid; the seed is redrawn
    until no level-0 mask decision is a tie and every level's mask mean is above need_mask_mean (for both mask rules)"""
    for attempt in range(200):
        g = torch.Generator().manual_seed(seed + 1000 * attempt)
        a, b = smooth_images(B, H, W, g)
        target = np.concatenate([a, b], 1)
        f0 = wc.smooth_flow(B, H, W, g, amp_y=2.5)
        back, _ = wc.warp_ref(f0, f0, "zeros")
        b0 = (-back + 0.15 * torch.randn(B, 2, H, W, generator=g).numpy()).astype(np.float32)
        full = torch.from_numpy(np.concatenate([f0, b0], 1))
        flows = []
        for l in range(levels):
            h, w = max(H >> l, 1), max(W >> l, 1)
            fl = F.interpolate(full, (h, w), mode="bilinear", align_corners=False) / (2 ** l) if l else full
            flows.append(np.ascontiguousarray(fl.numpy(), dtype=np.float32))
        ok = True
        for from_back in (True, False):
            for pdt in (np.float32, np.float64):
                m1, m2, t1, t2 = masks_level0(flows[0], from_back, pdt)
                ok &= not t1.any() and not t2.any()
                for fl in flows:
                    ok &= nearest_mask(m1, *fl.shape[2:]).mean() > need_mask_mean and nearest_mask(m2, *fl.shape[2:]).mean() > need_mask_mean
        if ok:
            return flows, target, attempt
    raise AssertionError("no seed gives tie-free masks")
