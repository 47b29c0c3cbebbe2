"""The AMD baseline's flow network (models/amd/pwc_lite.py) on the native convs, the cost volume, the warp and csrc/pwc.hip.

`PWCLite(mask_layer)` keeps the reference's constructor, attributes, parameter names and shapes -- a reference checkpoint loads with
strict=True -- and its forward(x, mask, with_bk=True) -> res_dict.  Gradients reach every parameter and both mask tensors.

How it runs (float32 only, no CPU path):
  * activations are NHWC; both frames go through the feature extractor as one batch of 2 B images; every conv is one autograd
    Function over ops.conv2d_fwd (bias and LeakyReLU(0.1) fused), ops.leaky_bwd + ops.conv2d_dgrad, ops.conv2d_wgrad, ops.colsum;
  * one level of FlowEstimatorReduce is ONE Function that owns its buffers: the conv1 input [x1_1by1 32 | corr 81 | flow 2 | zero 1]
    (the level's 1x1 conv writes its slice in place, ops.pwc_pack the rest; conv1 runs on a re-ordered, zero-padded copy of its
    [128, 115, 3, 3] weight) and x1 .. x5 as channel slices 0:128 | 128:256 | 256:352 | 352:416 | 416:448 of one buffer, so that
    every torch.cat of the reference is a contiguous slice and no activation is copied; the gradient buffer has the same shape;
  * the segment flows stay vectors: ops.segment_pool gives pooled [B, M, 96], the two predict_flow parameters act on those B M rows
    through F.linear (autograd adds both uses' gradients into the one parameter), sum_group is [B, M + 1, 2] and is doubled per
    level where the reference interpolates spatially constant maps; the `*_group` entries are expanded views;
  * the cost volume and the warp are planar: ops.nhwc_to_nchw / ops.nchw_to_nhwc sit between them and the convs."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, ops
from .correlation import Correlation

SLOPE = 0.1
EST_SLICES = {"x1": (0, 128), "x2": (128, 256), "x3": (256, 352), "x4": (352, 416), "x5": (416, 448)}
EST_WIDTH = 448
IN_1BY1, IN_CORR = 0, 32            # conv1's input buffer: [x1_1by1 32 | corr 81 | flow 2 | zero 1]


def _pad4(n):
    return (n + 3) // 4 * 4


class _exact_convs:
    """the convs of this network run on the exact fp32 matrix-core kernels (RCF_CONV_FP32_MFMA): the fp16-pair / bf16-triple
    kernels' 2^-22 per product puts a third of the parameter gradients outside 6 x the reference's own float32 error (measured:
    profiles/pwclite_parity.txt), and these convs are small.  The flag travels with each call; the process-wide switches stay"""

    def __enter__(self):
        self.old = ops.CONV_FLAGS
        if not (self.old >> 12) & 7:
            ops.CONV_FLAGS = self.old | _lib.CONV_FP32_MFMA(0)

    def __exit__(self, *exc):
        ops.CONV_FLAGS = self.old
        return False


class _Conv(nn.Module):
    """weight [Cout, Cin, k, k] (channels_last in memory, what the kernels read) and bias of one reference conv; `packed()` is the
    operand pair the kernels take: input channels re-ordered by `in_perm` (new position -> reference channel) and both channel
    counts zero-padded to multiples of 4, made once per weight version"""

    def __init__(self, cin, cout, k=3, stride=1, relu=True, in_perm=None):
        super().__init__()
        self.cin, self.cout, self.k, self.stride, self.pad, self.relu = cin, cout, k, stride, (k - 1) // 2, relu
        self.in_perm = in_perm
        self.weight = nn.Parameter(torch.empty(cout, cin, k, k).contiguous(memory_format=torch.channels_last))
        self.bias = nn.Parameter(torch.empty(cout))
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        bound = 1.0 / math.sqrt(cin * k * k)
        nn.init.uniform_(self.bias, -bound, bound)
        self._cache = None

    @property
    def plain(self):
        return self.in_perm is None and self.cin % 4 == 0 and self.cout % 4 == 0

    def packed(self):
        if self.plain:
            return self.weight.detach(), self.bias.detach()
        key = (ops.weight_key(self.weight), ops.weight_key(self.bias))
        if self._cache is None or self._cache[0] != key:
            w = self.weight.detach()
            if self.in_perm is not None:
                w = w[:, self.in_perm]
            w = F.pad(w, (0, 0, 0, 0, 0, _pad4(self.cin) - self.cin, 0, _pad4(self.cout) - self.cout))
            b = F.pad(self.bias.detach(), (0, _pad4(self.cout) - self.cout))
            self._cache = (key, w.contiguous(memory_format=torch.channels_last), b)
        return self._cache[1], self._cache[2]

    def param_grads(self, x, g, wp):
        """the gradients of weight and bias, in the parameters' own order, from the conv's input and the gradient behind its bias"""
        dwp = torch.empty_like(wp)
        ops.conv2d_wgrad(x, g, wp, dwp, self.stride, self.pad, 1, beta=0)
        db = torch.empty(wp.shape[0], dtype=torch.float32, device=g.device)
        ops.colsum(g, db, beta=0)
        if self.plain:
            return dwp, db
        dw = dwp[:self.cout, :self.cin]
        if self.in_perm is not None:
            inv = [0] * self.cin
            for new, old in enumerate(self.in_perm):
                inv[old] = new
            dw = dw[:, inv]
        return dw, db[:self.cout]

    def fwd(self, x, out=None):
        wp, bp = self.packed()
        with _exact_convs():
            return ops.conv2d_fwd(x, wp, bp, self.stride, self.pad, 1, act=1 if self.relu else 0, slope=SLOPE, out=out)

    def bwd(self, x, y, dy, need_dx=True, dx_out=None, beta=0):
        """dy: the gradient of the conv's (activated) output y -> (dx or None, dweight, dbias)"""
        wp, _ = self.packed()
        g = ops.leaky_bwd(dy, y, SLOPE) if self.relu else dy
        with _exact_convs():
            dw, db = self.param_grads(x, g, wp)
            dx = ops.conv2d_dgrad(g, wp, tuple(x.shape), self.stride, self.pad, 1, out=dx_out, beta=beta) if need_dx else None
        return dx, dw, db


def _block(*a, **k):
    return nn.Sequential(_Conv(*a, **k))          # the reference's nn.Sequential(nn.Conv2d, nn.LeakyReLU): parameters under ".0."


class _ConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, conv):
        y = conv.fwd(x)
        ctx.conv = conv
        ctx.save_for_backward(x, y)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y = ctx.saved_tensors
        dx, dw, db = ctx.conv.bwd(x, y, dy.contiguous(), need_dx=ctx.needs_input_grad[0])
        return dx, dw, db, None


class _ToPlanar(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return ops.nhwc_to_nchw(x)

    @staticmethod
    def backward(ctx, d):
        return ops.nchw_to_nhwc(d.contiguous())


class _ResizeFn(torch.autograd.Function):
    """bilinear, align_corners=True, planar"""

    @staticmethod
    def forward(ctx, x, size):
        ctx.in_size = tuple(x.shape[-2:])
        return ops.resize_nchw(x.contiguous(), size, align_corners=True)

    @staticmethod
    def backward(ctx, d):
        return ops.resize_nchw_bwd(d, ctx.in_size, align_corners=True), None


class _WarpFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, flow):
        ctx.save_for_backward(x, flow)
        return ops.flow_warp(x, flow)

    @staticmethod
    def backward(ctx, d):
        x, flow = ctx.saved_tensors
        return ops.flow_warp_bwd(x, flow, d, need_dx=ctx.needs_input_grad[0], need_dflow=ctx.needs_input_grad[1])


class _SegFlowFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mask, group):
        ctx.save_for_backward(mask, group)
        return ops.segment_flow(mask, group)

    @staticmethod
    def backward(ctx, d):
        mask, group = ctx.saved_tensors
        return ops.segment_flow_bwd(mask, group, d, need_dmask=ctx.needs_input_grad[0])


class _EstimatorFn(torch.autograd.Function):
    """(x1 NHWC, corr planar, flow planar, mask planar, the 16 parameters) -> (pooled [B, M, 96], flow_direct [B, 2, h, w])"""

    @staticmethod
    def forward(ctx, x1, corr, flow, mask, est, c1x1, *params):
        B, h, w, _ = x1.shape
        dev = x1.device
        inp = torch.empty((B, h, w, _pad4(est.conv1[0].cin)), dtype=torch.float32, device=dev)
        c1x1.fwd(x1, out=inp[..., IN_1BY1:IN_CORR])
        ops.pwc_pack(corr, flow, inp, IN_CORR)
        buf = torch.empty((B, h, w, EST_WIDTH), dtype=torch.float32, device=dev)
        for conv, src, dst in est.plan():
            conv.fwd(inp if src is None else buf[..., src[0]:src[1]], out=buf[..., dst[0]:dst[1]])
        feat = buf[..., EST_SLICES["x4"][0]:EST_SLICES["x5"][1]]
        h1 = est.predict_flow1[0].fwd(feat)
        direct = ops.nhwc_to_nchw(est.predict_flow2[0].fwd(h1), 2)
        pooled, msum = ops.segment_pool(feat, mask)
        ctx.est, ctx.c1x1 = est, c1x1
        ctx.save_for_backward(x1, mask, inp, buf, h1, pooled, msum)
        return pooled, direct

    @staticmethod
    def backward(ctx, dpooled, ddirect):
        x1, mask, inp, buf, h1, pooled, msum = ctx.saved_tensors
        est, c1x1 = ctx.est, ctx.c1x1
        gbuf = torch.empty_like(buf)
        lo, hi = EST_SLICES["x4"][0], EST_SLICES["x5"][1]
        gbuf[..., :lo].zero_()                                   # x1 .. x3 are first written by a launch that also adds onto x2 .. x4
        feat, gfeat = buf[..., lo:hi], gbuf[..., lo:hi]
        grads = {}
        # predict_flow2 (no activation, 2 of 4 output channels real), predict_flow1
        d4 = ops.nchw_to_nhwc(ddirect.contiguous(), 4)
        dh1, grads["pf2w"], grads["pf2b"] = est.predict_flow2[0].bwd(h1, None, d4)
        _, grads["pf1w"], grads["pf1b"] = est.predict_flow1[0].bwd(feat, h1, dh1, dx_out=gfeat, beta=0)
        _, dmask = ops.segment_pool_bwd(feat, mask, pooled, msum, dpooled.contiguous(), dfeat=gfeat, beta=1)
        ginp = None
        for i, (conv, src, dst) in reversed(list(enumerate(est.plan()))):
            x = inp if src is None else buf[..., src[0]:src[1]]
            if src is None:
                ginp = torch.empty_like(inp)
                dx_out, beta = ginp, 0
            else:
                dx_out, beta = gbuf[..., src[0]:src[1]], 1
            _, grads[f"c{i}w"], grads[f"c{i}b"] = conv.bwd(x, buf[..., dst[0]:dst[1]], gbuf[..., dst[0]:dst[1]], dx_out=dx_out, beta=beta)
        y1 = inp[..., IN_1BY1:IN_CORR]
        dx1, dw1, db1 = c1x1.bwd(x1, y1, ginp[..., IN_1BY1:IN_CORR], need_dx=ctx.needs_input_grad[0])
        dcorr, dflow = ops.pwc_unpack(ginp, IN_CORR, est.dim_corr)
        out = [dx1, dcorr, dflow if ctx.needs_input_grad[2] else None, dmask if ctx.needs_input_grad[3] else None, None, None, dw1, db1]
        for i in range(5):
            out += [grads[f"c{i}w"], grads[f"c{i}b"]]
        out += [grads["pf1w"], grads["pf1b"], grads["pf2w"], grads["pf2b"]]
        return tuple(out)


class FeatureExtractor(nn.Module):
    def __init__(self, num_chs):
        super().__init__()
        self.num_chs = num_chs
        self.convs = nn.ModuleList(nn.Sequential(_block(ci, co, stride=2), _block(co, co))
                                   for ci, co in zip(num_chs[:-1], num_chs[1:]))

    def forward(self, x):
        """x: NHWC, 3 channels padded to 4 -> the pyramid, coarsest first"""
        pyramid = []
        for layer in self.convs:
            for blk in layer:
                c = blk[0]
                x = _ConvFn.apply(x, c.weight, c.bias, c)
            pyramid.append(x)
        return pyramid[::-1]


class FlowEstimatorReduce(nn.Module):
    def __init__(self, ch_in, mask_layer=1, dim_corr=81):
        super().__init__()
        self.dim_corr = dim_corr
        # the reference's input order is [corr | x1_1by1 32 | flow 2]; the buffer holds [x1_1by1 | corr | flow | zero]
        perm = list(range(dim_corr, dim_corr + 32)) + list(range(dim_corr)) + [dim_corr + 32, dim_corr + 33]
        self.conv1 = _block(ch_in, 128, in_perm=perm)
        self.conv2 = _block(128, 128)
        self.conv3 = _block(128 + 128, 96)
        self.conv4 = _block(128 + 96, 64)
        self.conv5 = _block(96 + 64, 32)
        self.feat_dim = 32
        self.predict_flow1 = _block(64 + 32, 64, k=1)
        self.predict_flow2 = _block(64, 2, k=1, relu=False)
        self.mask_layer = mask_layer

    def plan(self):
        """(conv, input slice of the x1 .. x5 buffer or None for conv1's own input, output slice)"""
        s = EST_SLICES
        return [(self.conv1[0], None, s["x1"]), (self.conv2[0], s["x1"], s["x2"]), (self.conv3[0], (s["x1"][0], s["x2"][1]), s["x3"]),
                (self.conv4[0], (s["x2"][0], s["x3"][1]), s["x4"]), (self.conv5[0], (s["x3"][0], s["x4"][1]), s["x5"])]

    def params(self):
        out = []
        for blk in (self.conv1, self.conv2, self.conv3, self.conv4, self.conv5, self.predict_flow1, self.predict_flow2):
            out += [blk[0].weight, blk[0].bias]
        return out

    def segment_vectors(self, pooled):
        """predict_flow2(predict_flow1(.)) on the pooled rows [B, M, 96] -> [B, M, 2]"""
        p1, p2 = self.predict_flow1[0], self.predict_flow2[0]
        hid = F.leaky_relu(F.linear(pooled, p1.weight.flatten(1), p1.bias), SLOPE)
        return F.linear(hid, p2.weight.flatten(1), p2.bias)


class PWCLite(nn.Module):
    def __init__(self, mask_layer):
        super().__init__()
        self.search_range = 4
        self.num_chs = [3, 16, 32, 64, 96, 128, 192]
        self.num_levels = 7
        self.output_level = 4
        self.mask_layer = mask_layer
        self.feature_pyramid_extractor = FeatureExtractor(self.num_chs)
        self.upsample = True
        self.n_frames = 2
        self.reduce_dense = True
        self.corr = Correlation(self.search_range, slope=SLOPE)
        self.dim_corr = (self.search_range * 2 + 1) ** 2
        self.num_ch_in = 32 + (self.dim_corr + 2) * (self.n_frames - 1)
        self.flow_estimators = FlowEstimatorReduce(self.num_ch_in, mask_layer, self.dim_corr)
        self.conv_1x1 = nn.ModuleList(_block(c, 32, k=1) for c in (192, 128, 96, 64, 32))

    def num_parameters(self):
        return sum([p.data.nelement() if p.requires_grad else 0 for p in self.parameters()])

    def init_weights(self):
        for m in self.modules():
            if isinstance(m, _Conv):
                nn.init.kaiming_normal_(m.weight)
                nn.init.constant_(m.bias, 0)

    def forward_2_frames(self, x1_pyramid, x2_pyramid, planar1, planar2, mask):
        """x*_pyramid: NHWC features, coarsest first; planar*: the same as NCHW; mask: [B, M, H / 4, W / 4]"""
        est, M = self.flow_estimators, self.mask_layer
        B = mask.shape[0]
        flows, flows_all = [], []
        flow = flow_all = None
        sum_group = None
        minus_one = torch.full((B, 1, 2), -1.0, dtype=torch.float32, device=mask.device)      # the reference's flow_group[0] = -1
        for l in range(self.output_level + 1):
            x1, x1p, x2p = x1_pyramid[l], planar1[l], planar2[l]
            h, w = x1.shape[1:3]
            if l == 0:
                flow = torch.zeros((B, 2, h, w), dtype=torch.float32, device=mask.device)
                x2_warp = x2p
            else:
                flow = _ResizeFn.apply(flow * 2, (h, w))
                flow_all = _ResizeFn.apply(flow_all * 2, (h, w))
                sum_group = sum_group * 2
                x2_warp = _WarpFn.apply(x2p, flow)
            corr = self.corr(x1p, x2_warp)
            mask_l = _ResizeFn.apply(mask, (h, w))
            c1 = self.conv_1x1[l][0]
            pooled, direct = _EstimatorFn.apply(x1, corr, flow, mask_l, est, c1, c1.weight, c1.bias, *est.params())
            group = torch.cat([minus_one, est.segment_vectors(pooled)], 1)
            sum_group = group if sum_group is None else sum_group + group
            flow = _SegFlowFn.apply(mask_l, sum_group[:, 1:])
            flow_all = direct if flow_all is None else flow_all + direct
            flows.append(flow)
            flows_all.append(flow_all)
        if self.upsample:
            H, W = 4 * flows[-1].shape[2], 4 * flows[-1].shape[3]
            flows = [_ResizeFn.apply(f * 4, (4 * f.shape[2], 4 * f.shape[3])) for f in flows]
            flows_all = [_ResizeFn.apply(f * 4, (4 * f.shape[2], 4 * f.shape[3])) for f in flows_all]
            sum_group = sum_group * 4
        else:
            H, W = flows[-1].shape[2:]
        groups = [sum_group[:, i].reshape(B, 2, 1, 1).expand(B, 2, H, W) for i in range(M + 1)]
        return flows[::-1], flows_all[::-1], groups

    def _check(self, x, mask):
        ts = [x] + list(mask)
        for t in ts:
            if not torch.is_tensor(t) or not t.is_cuda:
                raise _lib.RcfHipError("rcf_amd.PWCLite needs CUDA (HIP) tensors: there is no CPU fallback")
            if t.dtype != torch.float32:
                raise _lib.RcfHipError(f"rcf_amd.PWCLite takes float32 tensors, not {t.dtype}")
        if x.dim() != 4 or x.size(1) != 6:
            raise _lib.RcfHipError(f"rcf_amd.PWCLite takes frame pairs [B, 6, H, W], not {tuple(x.shape)}")
        if x.shape[2] % 64 or x.shape[3] % 64:
            raise _lib.RcfHipError(f"H and W must be multiples of 64 (six halvings, doubled back level by level): {x.shape[2]} x {x.shape[3]}")
        for m in mask:
            if m.dim() != 4 or m.shape[0] != x.shape[0] or m.shape[1] != self.mask_layer:
                raise _lib.RcfHipError(f"every mask must be [B, {self.mask_layer}, h, w] for mask_layer = {self.mask_layer}: {tuple(m.shape)}")

    def forward(self, x, mask, with_bk=True):
        if len(mask) != 2:
            raise _lib.RcfHipError("mask holds the masks of the two frames")
        self._check(x, mask)
        B, _, H, W = x.shape
        both = x.reshape(B, 2, 3, H, W).transpose(0, 1).reshape(2 * B, 3, H, W).contiguous()      # frame 1 of every pair, then frame 2
        pyramid = self.feature_pyramid_extractor(ops.nchw_to_nhwc(both, 4))[:self.output_level + 1]
        planar = [_ToPlanar.apply(f) for f in pyramid]
        p1, p2 = [f[:B] for f in pyramid], [f[B:] for f in pyramid]
        q1, q2 = [f[:B] for f in planar], [f[B:] for f in planar]
        res = {}
        res["flows_fw"], res["flows_fw_all"], res["flows_fw_group"] = self.forward_2_frames(p1, p2, q1, q2, mask[1])
        if with_bk:
            res["flows_bw"], res["flows_bw_all"], res["flows_bw_group"] = self.forward_2_frames(p2, p1, q2, q1, mask[0])
        return res
