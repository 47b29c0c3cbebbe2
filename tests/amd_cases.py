"""What the AMDModel tests share (tests/test_amd_cpu.py, tests/test_amd_gpu.py, tests/golden/make_golden_amd.py, tools/time_amd.py):
the fixture's model settings, seeded weights and batch; float64 restatements of the three kernels of csrc/amd.hip with the sums of
absolute terms their bounds are stated in; and the edge-case tables of the sweep, derived from the library's geometry query.  None of
it is the reference's text."""
import collections
import copy

import numpy as np
import torch

import pwc_cases as pc
import spatial_cases as sc

U32 = 2.0 ** -24
DENORM = 2.0 ** -149                 # the spacing of float32 below FLT_MIN
MEAN = (123.675, 116.28, 103.53)     # models/fcn_head.py:160-161
STD = (58.395, 57.12, 57.375)
FLOW_SIZE = (384, 640)

# the fixture (tests/golden/amd.npz): B pairs of H x W frames, M masks; B = 2 so that a frame-major / batch-major mix-up shows
B, I, H, W, M, SEED = 2, 2, 96, 160, 5, 5119        # the seed: make_golden_amd.py --scan
SAMPLED = ["backbone2.layer2.1.conv2.weight", "backbone2.bn1.bias", "backbone2.layer4.0.downsample.0.weight",
           "decode_head2.convs.0.conv.weight", "decode_head2.convs.1.bn.weight", "decode_head2.conv_seg.bias",
           "decode_head.flownet.feature_pyramid_extractor.convs.0.0.0.weight", "decode_head.flownet.flow_estimators.conv1.0.weight",
           "decode_head.flownet.flow_estimators.predict_flow2.0.bias", "decode_head.flownet.conv_1x1.4.0.bias"]
FLOWNET = "decode_head.flownet."


def model_kwargs():
    """configs/amd/amd.yaml's model with the stand-ins of make_golden.py: BN for SyncBN, dropout 0, no visualisation step"""
    from rcf_amd import config
    kw = config.amd_model_kwargs(mask_layer=M, dropout=0.0, norm="BN", log_interval=10 ** 9)
    kw["train_iter"] = 1
    return copy.deepcopy(kw)


def state_dict(shapes, seed=SEED):
    """seeded, regenerable weights for a state-dict `shapes` mapping: synth.fill_state_dict, the flow network from pwc_cases.draw_params"""
    from rcf_amd import synth
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.fill_state_dict(shapes, seed=seed).items()}
    for k, v in pc.draw_params(seed).items():
        assert tuple(shapes[FLOWNET + k]) == v.shape
        sd[FLOWNET + k] = torch.from_numpy(v)
    return sd


def batch(device="cpu", dtype=torch.float32):
    from rcf_amd import synth
    nb = synth.make_batch(B, H, W, config_id=1)
    return {"imgs": [torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dtype) for a in nb["imgs"]],
            "seq_ids": nb["seq_ids"], "seq_names": nb["seq_names"], "paths": nb["paths"]}


def flat_shapes(shapes):
    """a list of shapes as one int64 vector, -1 after each (the layout of pwclite.npz)"""
    return np.asarray(sum(([*s, -1] for s in shapes), []), dtype=np.int64)


def unflat_shapes(v):
    out, cur = [], []
    for x in v:
        if x < 0:
            out.append(tuple(cur))
            cur = []
        else:
            cur.append(int(x))
    return out


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def grad_norms(named):
    out = {}
    for name, p in named:
        if p.grad is not None:
            top = name.split(".")[0]
            out[top] = out.get(top, 0.0) + float(p.grad.double().pow(2).sum())
    return {k: float(np.sqrt(v)) for k, v in out.items()}


# ======================================================================================================= kernel restatements
def softmax_ref(logits, B, I, M):
    """logits [B I, h, w, C >= M] float64, image n = b I + i -> masks [I, B, M, h, w]: exp(x - max) / sum, written out"""
    N, h, w, _ = logits.shape
    x = logits[..., :M].reshape(B, I, h, w, M)
    e = torch.exp(x - x.amax(-1, keepdim=True))
    return (e / e.sum(-1, keepdim=True)).permute(1, 0, 4, 2, 3).contiguous()


def softmax_bwd_ref(masks, dmasks):
    """masks [I, B, M, h, w] float64, dmasks: I tensors [B, M, h, w] or None (zeros) -> (dlogits [B I, h, w, M], mass):
    dl_c = p_c (dp_c - sum_k p_k dp_k), mass = |p_c| (|dp_c| + sum_k |p_k dp_k|)"""
    I, B, M, h, w = masks.shape
    dp = torch.stack([torch.zeros_like(masks[0]) if d is None else d for d in dmasks])
    dot, adot = (masks * dp).sum(2, keepdim=True), (masks * dp).abs().sum(2, keepdim=True)
    dl, mass = masks * (dp - dot), masks.abs() * (dp.abs() + adot)
    nhwc = lambda t: t.permute(1, 0, 3, 4, 2).reshape(B * I, h, w, M)
    return nhwc(dl), nhwc(mass)


def denorm_ref(frames):
    """[B, 2, 3, H, W] float64 -> ((x std + mean) / 255, (|x| std + mean) / 255) as [B, 6, H, W]"""
    std = torch.tensor(STD, dtype=torch.float64).view(1, 1, 3, 1, 1)
    mean = torch.tensor(MEAN, dtype=torch.float64).view(1, 1, 3, 1, 1)
    flat = lambda t: t.reshape(t.shape[0], 6, *t.shape[3:])
    return flat((frames * std + mean) / 255.0), flat((frames.abs() * std + mean) / 255.0)


def frame_pair_ref(frames, size):
    """-> (two_frame [B, 6, Ho, Wo], mass): de-normalise, then bilinear align_corners=True with float32 sample positions and float64
    values (spatial_cases.axis_matrix), as in tests/warp_cases.py"""
    v, a = denorm_ref(frames.double())
    Hi, Wi = v.shape[2:]
    Ay, Ax = sc.axis_matrix(size[0], Hi, True), sc.axis_matrix(size[1], Wi, True)
    rs = lambda t: torch.einsum("oh,bchw,pw->bcop", Ay, t, Ax)
    return rs(v), rs(a)


FRAME_PAIR_K = 19          # csrc/amd.hip: 3 roundings de-normalise a tap, then spatial_cases.fwd_bound's 16


def denorm_f32(frames):
    """the de-normalised frames as IEEE float32 arithmetic gives them (product, sum, division): numpy, [B, 6, H, W]"""
    x = frames.numpy().astype(np.float32)
    std = np.asarray(STD, dtype=np.float32).reshape(1, 1, 3, 1, 1)
    mean = np.asarray(MEAN, dtype=np.float32).reshape(1, 1, 3, 1, 1)
    out = (x * std + mean) / np.float32(255.0)
    assert out.dtype == np.float32
    return out.reshape(x.shape[0], 6, *x.shape[3:])


# ============================================================================================================ the case tables
def geometry():
    from rcf_amd import _lib
    lib = _lib.load()
    return tuple(lib.rcf_amd_geometry(i) for i in range(3))          # pixels per workgroup, max M, max I


Soft = collections.namedtuple("Soft", "name I B M Cp pitch h w kind absent")


def softmax_cases():
    """pixel counts about a workgroup's share, every M the issue names, both channel paddings, a wider pitch, two batch shapes; kinds:
    'normal' logits, 'pm80' (+-80), 'equal', 'naninf' (one NaN and one +inf logit); absent: the frame whose gradient is None"""
    pix, maxm, _ = geometry()
    return [Soft("one_pixel_m1", 2, 1, 1, 4, 4, 1, 1, "normal", None),
            Soft("under_share_m2", 2, 3, 2, 4, 4, 1, pix - 1, "normal", None),
            Soft("over_share_m5", 2, 1, 5, 8, 8, 1, pix + 1, "normal", 0),
            Soft("ragged_wide_pitch", 2, 3, 5, 8, 12, 7, 43, "normal", 1),
            Soft("most_masks", 2, 1, maxm, 8, 8, 5, 13, "normal", None),
            Soft("m1_wide_pitch", 2, 3, 1, 4, 8, 3, 5, "normal", None),
            Soft("pm80", 2, 1, 5, 8, 8, 3, 50, "pm80", None),
            Soft("equal", 2, 3, 2, 4, 8, 2, 9, "equal", None),
            Soft("naninf", 2, 1, 5, 8, 8, 4, 37, "naninf", None)]


def softmax_inputs(c):
    """-> (wide [B I, h, w, pitch] float32 with 7.0 in the channels from Cp up, dmasks: I tensors [B, M, h, w] or None)"""
    g = torch.Generator().manual_seed(sum(map(ord, c.name)) + 5 * c.w)
    N = c.I * c.B
    wide = torch.full((N, c.h, c.w, c.pitch), 7.0)
    x = 1.5 * torch.randn(N, c.h, c.w, c.Cp, generator=g)
    if c.kind == "pm80":
        x = torch.where(torch.rand(N, c.h, c.w, c.Cp, generator=g) < 0.5, torch.tensor(-80.0), torch.tensor(80.0))
        x[0, 0, 0, :c.M] = 80.0
        x[0, 0, 1, :c.M] = -80.0
    elif c.kind == "equal":
        x = torch.full((N, c.h, c.w, c.Cp), 0.3125)
    elif c.kind == "naninf":
        x[0, 1, 2, 1] = float("nan")
        x[1, 2, 3, 0] = float("inf")
        x[1, 0, 5, 2] = float("-inf")
    wide[..., :c.Cp] = x
    dm = [None if i == c.absent else torch.randn(c.B, c.M, c.h, c.w, generator=g) for i in range(c.I)]
    return wide, dm


Pair = collections.namedtuple("Pair", "name B Hi Wi Ho Wo")
# identity, the fixture's 96 x 160 -> 384 x 640, non-integer ratios up and down, one input row / column / pixel, the smallest size PWCLite takes
PAIRS = [Pair("identity", 3, 7, 9, 7, 9), Pair("model", 1, 96, 160, 384, 640), Pair("up", 3, 5, 7, 13, 11), Pair("down", 1, 24, 40, 7, 9),
         Pair("one_row", 1, 1, 9, 4, 9), Pair("one_column", 1, 8, 1, 8, 5), Pair("one_pixel", 3, 1, 1, 4, 6), Pair("smallest_net", 1, 24, 40, 64, 128)]
# (Hi, Wi, Ho, Wo) whose align_corners scales (in - 1) / (out - 1) are dyadic: float32 and float64 sample positions coincide
DYADIC = [(7, 9, 7, 9), (3, 5, 5, 9), (5, 3, 17, 9), (9, 17, 5, 5), (1, 4, 3, 4), (2, 2, 1, 1)]


def pair_inputs(c, seed=0):
    g = torch.Generator().manual_seed(100 * c.Hi + c.Wo + seed)
    return 1.2 * torch.randn(c.B, 2, 3, c.Hi, c.Wi, generator=g)
