"""What the PWC-Lite tests share (tests/test_pwclite_cpu.py, tests/test_pwclite_gpu.py, tests/golden/make_golden_pwclite.py,
tools/time_pwclite.py): a restatement of models/amd/pwc_lite.py from torch ops in the vector-segment form rcf_amd.PWCLite uses (the
pooled features and the segment flows are [B, M, .] vectors, never broadcast maps), the seeded inputs and weights of the fixture,
float64 restatements of every kernel of csrc/pwc.hip with their analytic backward and the sums of absolute terms the error bounds
are stated in, and the edge-case tables of the sweep.  None of it is the reference's text."""
import collections

import numpy as np
import torch
import torch.nn.functional as F

import spatial_cases as sc

SLOPE = 0.1
U32 = 2.0 ** -24
NUM_CHS = [3, 16, 32, 64, 96, 128, 192]
LEVEL_CHS = (192, 128, 96, 64, 32)
OUT_LEVELS = 5
T = torch.from_numpy


# ====================================================================================================== parameters and inputs
def param_shapes():
    """(name, shape) in the reference's state-dict order"""
    out = []
    for l, (ci, co) in enumerate(zip(NUM_CHS[:-1], NUM_CHS[1:])):
        for j, c in enumerate((ci, co)):
            out += [(f"feature_pyramid_extractor.convs.{l}.{j}.0.weight", (co, c, 3, 3)), (f"feature_pyramid_extractor.convs.{l}.{j}.0.bias", (co,))]
    est = [("conv1", 115, 128, 3), ("conv2", 128, 128, 3), ("conv3", 256, 96, 3), ("conv4", 224, 64, 3), ("conv5", 160, 32, 3),
           ("predict_flow1", 96, 64, 1), ("predict_flow2", 64, 2, 1)]
    for name, ci, co, k in est:
        out += [(f"flow_estimators.{name}.0.weight", (co, ci, k, k)), (f"flow_estimators.{name}.0.bias", (co,))]
    for l, c in enumerate(LEVEL_CHS):
        out += [(f"conv_1x1.{l}.0.weight", (32, c, 1, 1)), (f"conv_1x1.{l}.0.bias", (32,))]
    return out


FLOW2_SCALE = 0.1          # a Kaiming-size predict_flow2 gives flows of a hundred pixels; this one a few


def draw_params(seed):
    """float32 numpy weights, drawn in param_shapes() order: Kaiming-normal weights (predict_flow2 scaled down), small biases"""
    rng = np.random.default_rng(seed)
    out = collections.OrderedDict()
    for name, shape in param_shapes():
        if len(shape) == 4:
            v = rng.standard_normal(shape) * np.sqrt(2.0 / (shape[1] * shape[2] * shape[3]))
            if "predict_flow2" in name:
                v *= FLOW2_SCALE
        else:
            v = rng.standard_normal(shape) * (0.002 if "predict_flow2" in name else 0.02)
        out[name] = v.astype(np.float32)
    return out


Case = collections.namedtuple("Case", "name B H W M seed")
GOLDEN = [Case("smallest", 2, 64, 128, 5, 4110), Case("tiles", 2, 128, 192, 2, 4439)]


def draw_inputs(c, seed=None):
    """(frames float32 [B, 6, H, W] with values k / 255, masks float32 [2, B, M, H / 4, W / 4]: a softmax of seeded normals)"""
    rng = np.random.default_rng(c.seed if seed is None else seed)
    y, x = np.mgrid[0:c.H, 0:c.W].astype(np.float64)
    frames = np.zeros((c.B, 6, c.H, c.W))
    for b in range(c.B):
        fy, fx, ph = rng.uniform(0.02, 0.12, (3, 4)), rng.uniform(0.02, 0.12, (3, 4)), rng.uniform(0, 6.28, (3, 4))
        dx, dy = rng.uniform(-2.5, 2.5, 2)
        for ch in range(3):
            for k, (xs, ys) in enumerate(((x, y), (x + dx, y + dy))):
                v = sum(np.sin(fy[ch, i] * ys + fx[ch, i] * xs + ph[ch, i]) for i in range(4))
                frames[b, 3 * k + ch] = 0.5 + v / 8.0
    frames = np.round(np.clip(frames, 0, 1) * 255) / 255
    logits = rng.standard_normal((2, c.B, c.M, c.H // 4, c.W // 4)) * 1.5
    e = np.exp(logits - logits.max(2, keepdims=True))
    return frames.astype(np.float32), (e / e.sum(2, keepdims=True)).astype(np.float32)


def output_items(res):
    """(key, tensor) of every output, in one fixed order"""
    out = []
    for d in ("fw", "bw"):
        for kind in ("", "_all", "_group"):
            key = f"flows_{d}{kind}"
            if key in res:
                out += [(f"{key}_{i}", t) for i, t in enumerate(res[key])]
    return out


def functional(res, seed):
    """a fixed linear functional of all flow outputs: sum over the tensors of mean(w t), w seeded normals"""
    rng = np.random.default_rng(seed + 17)
    total = 0
    for _, t in output_items(res):
        w = torch.from_numpy(rng.standard_normal(tuple(t.shape))).to(device=t.device, dtype=t.dtype)
        total = total + (w * t).mean()
    return total


def sample(n, budget, least=7):
    """the stored elements of a flattened tensor of n elements: every `least`-th while that fits `budget`, else a larger odd stride"""
    return slice(0, n, max(least, -(-n // budget)) | 1)


OUT_BUDGET, GRAD_BUDGET, MASK_BUDGET = 200, 48, 1000


# ================================================================================================= the network, from torch ops
KINKS = None          # a list: _conv appends min |pre-activation| / max |pre-activation| of every LeakyReLU conv (kink_distance)


def _conv(p, name, x, stride=1, relu=True):
    w = p[name + ".weight"]
    y = F.conv2d(x, w, p[name + ".bias"], stride=stride, padding=(w.shape[2] - 1) // 2)
    if relu and KINKS is not None:
        a = y.detach().abs()
        KINKS.append(float(a.min() / a.max()))
    return F.leaky_relu(y, SLOPE) if relu else y


def _features(p, img):
    out = []
    for l in range(6):
        img = _conv(p, f"feature_pyramid_extractor.convs.{l}.1.0", _conv(p, f"feature_pyramid_extractor.convs.{l}.0.0", img, stride=2))
        out.append(img)
    return out[::-1]


def _warp(x, flow):
    B, _, H, W = x.shape
    gy, gx = torch.meshgrid(torch.arange(H, dtype=x.dtype, device=x.device), torch.arange(W, dtype=x.dtype, device=x.device), indexing="ij")
    px, py = gx[None] + flow[:, 0], gy[None] + flow[:, 1]
    grid = torch.stack([2.0 * px / (W - 1) - 1.0, 2.0 * py / (H - 1) - 1.0], -1)
    return F.grid_sample(x, grid, mode="bilinear", padding_mode="border", align_corners=True)


def _corr(x1, x2, d=4):
    B, C, H, W = x1.shape
    x2 = F.pad(x2, [d] * 4)
    return torch.stack([(x1 * x2[:, :, i:i + H, j:j + W]).mean(1) for i in range(2 * d + 1) for j in range(2 * d + 1)], 1)


def _resize(x, size):
    return F.interpolate(x, size=tuple(size), mode="bilinear", align_corners=True)


def _estimator(p, x, mask):
    """-> (pooled-and-predicted segment vectors [B, M, 2], flow_direct [B, 2, h, w])"""
    e = "flow_estimators."
    x1 = _conv(p, e + "conv1.0", x)
    x2 = _conv(p, e + "conv2.0", x1)
    x3 = _conv(p, e + "conv3.0", torch.cat([x1, x2], 1))
    x4 = _conv(p, e + "conv4.0", torch.cat([x2, x3], 1))
    x5 = _conv(p, e + "conv5.0", torch.cat([x3, x4], 1))
    feat = torch.cat([x4, x5], 1)
    direct = _conv(p, e + "predict_flow2.0", _conv(p, e + "predict_flow1.0", feat), relu=False)
    pooled = torch.einsum("bchw,bmhw->bmc", feat, mask) / mask.sum((2, 3))[..., None]
    w1, w2 = p[e + "predict_flow1.0.weight"].flatten(1), p[e + "predict_flow2.0.weight"].flatten(1)
    hid = F.leaky_relu(F.linear(pooled, w1, p[e + "predict_flow1.0.bias"]), SLOPE)
    return F.linear(hid, w2, p[e + "predict_flow2.0.bias"]), direct


def _two_frames(p, pyr1, pyr2, mask):
    B, M = mask.shape[:2]
    flows, flows_all = [], []
    flow = flow_all = sum_group = None
    minus_one = torch.full((B, 1, 2), -1.0, dtype=mask.dtype, device=mask.device)
    for l in range(OUT_LEVELS):
        x1, x2 = pyr1[l], pyr2[l]
        h, w = x1.shape[2:]
        if l == 0:
            flow = torch.zeros((B, 2, h, w), dtype=mask.dtype, device=mask.device)
        else:
            flow, flow_all, sum_group = _resize(flow * 2, (h, w)), _resize(flow_all * 2, (h, w)), sum_group * 2
            x2 = _warp(x2, flow)
        corr = F.leaky_relu(_corr(x1, x2), SLOPE)
        mask_l = _resize(mask, (h, w))
        vec, direct = _estimator(p, torch.cat([corr, _conv(p, f"conv_1x1.{l}.0", x1), flow], 1), mask_l)
        group = torch.cat([minus_one, vec], 1)
        sum_group = group if sum_group is None else sum_group + group
        flow = torch.einsum("bmhw,bmc->bchw", mask_l, sum_group[:, 1:])
        flow_all = direct if flow_all is None else flow_all + direct
        flows.append(flow)
        flows_all.append(flow_all)
    flows = [_resize(f * 4, (4 * f.shape[2], 4 * f.shape[3])) for f in flows]
    flows_all = [_resize(f * 4, (4 * f.shape[2], 4 * f.shape[3])) for f in flows_all]
    H, W = flows[-1].shape[2:]
    groups = [(sum_group[:, i] * 4).reshape(B, 2, 1, 1).expand(B, 2, H, W) for i in range(M + 1)]
    return flows[::-1], flows_all[::-1], groups


def net_ref(p, x, masks, with_bk=True):
    """p: {name: tensor}; x [B, 6, H, W]; masks: (mask of frame 1, mask of frame 2) -> the reference's res_dict"""
    pyr = [_features(p, x[:, :3]), _features(p, x[:, 3:])]
    res = {}
    res["flows_fw"], res["flows_fw_all"], res["flows_fw_group"] = _two_frames(p, pyr[0], pyr[1], masks[1])
    if with_bk:
        res["flows_bw"], res["flows_bw_all"], res["flows_bw_group"] = _two_frames(p, pyr[1], pyr[0], masks[0])
    return res


def kink_distance(c, seed=None):
    """the smallest |pre-activation| of any LeakyReLU conv of the float64 run, relative to its layer's largest: a float32 run whose
    rounding reaches it decides that element's slope differently, and one such element moves a bias gradient by 1e-4 of its range"""
    global KINKS
    seed = c.seed if seed is None else seed
    frames, masks = draw_inputs(c, seed)
    p = {k: T(v).double() for k, v in draw_params(seed).items()}
    KINKS = []
    try:
        with torch.no_grad():
            net_ref(p, T(frames).double(), [T(masks[i]).double() for i in range(2)])
        return min(KINKS)
    finally:
        KINKS = None


# 4 ulp of the layer's range: a float32 dot product whose partial sums stay under the layer's largest value lands within a few ulp of
# that value, whatever the order of its sums -- no float32 run, the reference's or the kernels', then decides a slope differently.
# (About one draw in fifty of the larger case clears it: its two million activations leave ~5 within 3e-7 on average.)
MIN_KINK_DISTANCE = 2.0 ** -22


def run_ref(c, dtype=torch.float64, device="cpu", net=net_ref):
    """outputs and the functional's gradients of one fixture case -> ({key: tensor}, {name: grad}, [dmask0, dmask1])"""
    frames, masks = draw_inputs(c)
    p = {k: T(v).to(device=device, dtype=dtype).requires_grad_(True) for k, v in draw_params(c.seed).items()}
    m = [T(masks[i]).to(device=device, dtype=dtype).requires_grad_(True) for i in range(2)]
    res = net(p, T(frames).to(device=device, dtype=dtype), m)
    functional(res, c.seed).backward()
    return {k: t.detach() for k, t in output_items(res)}, {k: v.grad for k, v in p.items()}, [t.grad for t in m]


# ======================================================================================================= kernel restatements
def pool_ref(feat, mask):
    """feat [B, h, w, C], mask [B, M, h, w] (float64 tensors) -> pooled [B, M, C], msum [B, M], mass of pooled"""
    s = torch.einsum("bhwc,bmhw->bmc", feat, mask)
    ms = mask.sum((2, 3))
    with np.errstate(all="ignore"):
        return s / ms[..., None], ms, torch.einsum("bhwc,bmhw->bmc", feat.abs(), mask.abs()) / ms.abs()[..., None]


def pool_bwd_ref(feat, mask, pooled, msum, dpooled):
    """-> dfeat [B, h, w, C], dmask [B, M, h, w] and their masses (the sums of the absolute terms)"""
    q = dpooled / msum[..., None]
    dfeat = torch.einsum("bmhw,bmc->bhwc", mask, q)
    mfeat = torch.einsum("bmhw,bmc->bhwc", mask.abs(), q.abs())
    dot = (pooled * dpooled).sum(2)
    dmask = (torch.einsum("bhwc,bmc->bmhw", feat, dpooled) - dot[..., None, None]) / msum[..., None, None]
    mmask = (torch.einsum("bhwc,bmc->bmhw", feat.abs(), dpooled.abs()) + (pooled * dpooled).abs().sum(2)[..., None, None]) / msum.abs()[..., None, None]
    return dfeat, dmask, mfeat, mmask


def flow_ref(mask, group):
    return torch.einsum("bmhw,bmc->bchw", mask, group), torch.einsum("bmhw,bmc->bchw", mask.abs(), group.abs())


def flow_bwd_ref(mask, group, dflow):
    dmask, mmask = torch.einsum("bchw,bmc->bmhw", dflow, group), torch.einsum("bchw,bmc->bmhw", dflow.abs(), group.abs())
    return dmask, torch.einsum("bmhw,bchw->bmc", mask, dflow), mmask, torch.einsum("bmhw,bchw->bmc", mask.abs(), dflow.abs())


def resize_adjoint_ref(dy, Hi, Wi, align):
    """planar dy [P, Ho, Wo] float64 -> (dx [P, Hi, Wi], mass, terms [Hi, Wi]): the taps in float32 as the kernels and torch compute
    them, the sums in float64 (tests/spatial_cases.py)"""
    dx, mass, terms = sc.resize_bwd_ref(dy.permute(1, 2, 0)[None], Hi, Wi, align)
    return dx[0].permute(2, 0, 1), mass[0].permute(2, 0, 1), terms


def resize_fwd_ref(x, Ho, Wo, align):
    out, _ = sc.resize_fwd_ref(x.permute(1, 2, 0)[None], Ho, Wo, align)
    return out[0].permute(2, 0, 1)


def leaky_bwd_ref(dy, y, slope=SLOPE):
    return torch.where(y > 0, dy, dy * slope)


def pack_ref(corr, flow, buf, c0):
    """corr [B, D, h, w], flow [B, 2, h, w], buf [B, h, w, C] -> the buffer after the pack"""
    D = corr.shape[1]
    end = (c0 + D + 2 + 3) // 4 * 4
    out = buf.clone()
    out[..., c0:c0 + D] = corr.permute(0, 2, 3, 1)
    out[..., c0 + D:c0 + D + 2] = flow.permute(0, 2, 3, 1)
    out[..., c0 + D + 2:end] = 0
    return out


def unpack_ref(dbuf, c0, D):
    return dbuf[..., c0:c0 + D].permute(0, 3, 1, 2), dbuf[..., c0 + D:c0 + D + 2].permute(0, 3, 1, 2)


def rel_err(got, want):
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-300))


def margin(got, ref, bound):
    return sc.elem_margin(got, ref, bound)


# ============================================================================================================ the case tables
def geometry():
    from rcf_amd import _lib
    lib = _lib.load()
    return tuple(lib.rcf_pwc_geometry(i) for i in range(5))          # chunk, max M, max C, pack tile, pack channels


Seg = collections.namedtuple("Seg", "name B M C h w pitch c0 mask beta")


def seg_cases():
    """pool and compose: pixel counts about the chunk, every M, the two channel counts, a nearly empty mask, both betas"""
    chunk, maxm = geometry()[:2]
    cs = [Seg("two_pixels", 2, 5, 96, 1, 2, 448, 352, "softmax", 0),
          Seg("under_chunk", 2, 2, 96, 16, 32, 448, 352, "softmax", 1),
          Seg("ragged", 2, 5, 4, 1, chunk + chunk // 2 - 3, 8, 4, "softmax", 0),
          Seg("one_past", 1, 1, 4, 1, chunk + 1, 4, 0, "softmax", 1),
          Seg("several", 2, 2, 96, 3 * chunk // 64 + 1, 64, 448, 352, "softmax", 0),
          Seg("most_masks", 1, maxm, 4, 7, 9, 12, 8, "softmax", 1),
          Seg("tiny_sum", 2, 2, 4, 5, 7, 4, 0, "tiny", 0)]
    return cs


def seg_inputs(c):
    g = torch.Generator().manual_seed(sum(map(ord, c.name)) + 3 * c.h)
    wide = torch.randn(c.B, c.h, c.w, c.pitch, generator=g)
    if c.mask == "tiny":
        mask = torch.rand(c.B, c.M, c.h, c.w, generator=g)
        mask = mask / mask.sum((2, 3), keepdim=True) * 1e-6
    else:
        mask = torch.softmax(1.5 * torch.randn(c.B, c.M, c.h, c.w, generator=g), 1)
    return {"wide": wide, "mask": mask.contiguous(), "dpooled": torch.randn(c.B, c.M, c.C, generator=g),
            "old": torch.randn(c.B, c.h, c.w, c.pitch, generator=g), "group": torch.randn(c.B, c.M, 2, generator=g) * 3,
            "dflow": torch.randn(c.B, 2, c.h, c.w, generator=g), "old_mask": torch.randn(c.B, c.M, c.h, c.w, generator=g)}


# planes, (Hi, Wi) -> (Ho, Wo)
RESIZE = [(3, 1, 2, 2, 4), (3, 3, 5, 6, 10), (2, 5, 7, 20, 28), (4, 24, 40, 6, 10), (2, 9, 11, 9, 11)]
LEAKY = [(37, 4, 4, 4, 4), (37, 4, 12, 8, 4), (26, 448, 448, 448, 448), (26, 32, 448, 448, 32)]      # rows, C, dy / y / g pitches
PACK = [(2, 1, 2), (2, 5, 27)]                                                                      # B, h, w (the second crosses a tile)
