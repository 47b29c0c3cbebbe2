"""The AMD baseline's unsupervised flow loss (models/amd/flow_loss.py) on the fused kernels of csrc/unflow.hip.

`unFlowLoss(cfg)` keeps the reference's constructor -- cfg is anything with attribute access and keys(): w_l1, w_ssim, w_ternary,
ssim_sz (1, 2 or 3), w_scales, w_sm_scales, w_real_smooth, smooth_2nd (optional), alpha, occ_from_back, warp_pad ('border'),
with_bk -- and its forward(output, target) -> (total_loss, warp_loss, smooth_loss, pyramid_flows[0].abs().mean()), all 0-dim device
tensors, with `pyramid_occu_mask1` / `pyramid_occu_mask2` filled as the reference fills them.  Every (level, direction) is one
autograd Function over ops.unflow_photo / ops.unflow_smooth and their backwards: the gradient goes to the flows, the frames and
the masks are constants.  The level-0 masks come from ops.occu_mask_backward / ops.occu_mask_bidirection; deeper levels read them
by torch's nearest rule inside the kernel, and the resized mask tensors of `pyramid_occu_mask*` are only made for the caller.
The area pyramid of `target` is cached by the tensor's identity and version: the second call of a training step (whole-image
flows on the same frame pair) reuses it, an in-place change of the frames rebuilds it.  There is no CPU path."""
import weakref

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, ops

SSIM_SIZES = (1, 2, 3)          # what csrc/unflow.hip instantiates


class _PhotoFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, flow, im, other, occ, md, w_l1, w_ssim, w_ternary):
        loss, stats = ops.unflow_photo(im, other, flow, occ, md, w_l1, w_ssim, w_ternary)
        ctx.args = (md, w_l1, w_ssim, w_ternary)
        ctx.save_for_backward(flow, im, other, occ, stats)
        return loss.clone()

    @staticmethod
    def backward(ctx, dloss):
        flow, im, other, occ, stats = ctx.saved_tensors
        dflow = ops.unflow_photo_bwd(im, other, flow, occ, stats, dloss, *ctx.args) if ctx.needs_input_grad[0] else None
        return (dflow,) + (None,) * 7


class _SmoothFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, flow, im, alpha, s, second):
        ctx.args = (alpha, s, second)
        ctx.save_for_backward(flow, im)
        return ops.unflow_smooth(flow, im, alpha, s, second).clone()

    @staticmethod
    def backward(ctx, dloss):
        flow, im = ctx.saved_tensors
        dflow = ops.unflow_smooth_bwd(flow, im, dloss, *ctx.args) if ctx.needs_input_grad[0] else None
        return dflow, None, None, None, None


class unFlowLoss(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        self.ssim_sz = cfg.ssim_sz
        if cfg.warp_pad != "border":
            raise NotImplementedError(f"warp_pad {cfg.warp_pad!r}: the native flow loss samples in 'border' mode only")
        if self.ssim_sz not in SSIM_SIZES:
            raise NotImplementedError(f"ssim_sz {self.ssim_sz!r}: the native flow loss is built for {SSIM_SIZES}")
        self.pyramid_occu_mask1, self.pyramid_occu_mask2 = [], []
        self._pyramid = None            # (weakref to target, its version, {(h, w): (im1, im2)})

    # ------------------------------------------------------------------------------------------------------ the area pyramid
    def _images(self, target, size):
        cache = self._pyramid
        if cache is None or cache[0]() is not target or cache[1] != target._version:
            cache = self._pyramid = (weakref.ref(target), target._version, {})
        if size not in cache[2]:
            cache[2][size] = (ops.area_resize(target[:, :3], size), ops.area_resize(target[:, 3:], size))
        return cache[2][size]

    def _smooth(self, flow, im, s):
        second = "smooth_2nd" in self.cfg.keys() and bool(self.cfg.smooth_2nd)
        return _SmoothFn.apply(flow, im, float(self.cfg.alpha), float(s), second)

    def forward(self, output, target):
        """output: multi-scale forward / backward flows, n x [B, 4, h, w]; target: frame pairs [B, 6, H, W]"""
        cfg = self.cfg
        pyramid_flows = output
        md = int(self.ssim_sz)
        for i, flow in enumerate(pyramid_flows):
            if cfg.w_scales[i] != 0 and min(flow.shape[2:]) < 2 * md + 1:
                raise _lib.RcfHipError(f"level {i} is {flow.shape[2]} x {flow.shape[3]}: smaller than the {2 * md + 1} x {2 * md + 1} SSIM window")
        for t in list(pyramid_flows) + [target]:
            if not t.is_cuda:
                raise _lib.RcfHipError("rcf_amd.unFlowLoss needs CUDA (HIP) tensors: there is no CPU fallback")
            if t.dtype != torch.float32:
                raise _lib.RcfHipError(f"rcf_amd.unFlowLoss takes float32 tensors, not {t.dtype}")
        weights = (md, float(cfg.w_l1), float(cfg.w_ssim), float(cfg.w_ternary))
        smooth_on = cfg.w_real_smooth > 0
        zero = torch.zeros((), dtype=torch.float32, device=target.device)
        self.pyramid_occu_mask1, self.pyramid_occu_mask2 = [], []
        warp_loss, smooth_sum = zero, zero
        occ1 = occ2 = None
        s = 1.0
        for i, flow in enumerate(pyramid_flows):
            if cfg.w_scales[i] == 0:
                continue
            h, w = flow.shape[2:]
            im1, im2 = self._images(target, (h, w))
            f12, f21 = flow[:, :2], flow[:, 2:]
            if occ1 is None:
                if i != 0:
                    raise _lib.RcfHipError("w_scales[0] is 0: the reference takes its masks from level 0 and fails without it")
                with torch.no_grad():
                    if cfg.occ_from_back:
                        occ1 = 1 - ops.occu_mask_backward(f21, th=0.2)
                        occ2 = 1 - ops.occu_mask_backward(f12, th=0.2)
                    else:
                        occ1 = 1 - ops.occu_mask_bidirection(f12, f21)
                        occ2 = 1 - ops.occu_mask_bidirection(f21, f12)
                s = float(min(h, w))
                self.pyramid_occu_mask1.append(occ1)
                self.pyramid_occu_mask2.append(occ2)
            else:
                self.pyramid_occu_mask1.append(F.interpolate(occ1, (h, w), mode="nearest"))
                self.pyramid_occu_mask2.append(F.interpolate(occ2, (h, w), mode="nearest"))
            loss_warp = _PhotoFn.apply(f12, im1, im2, occ1, *weights)
            loss_smooth = self._smooth(f12, im1, s) if smooth_on else zero
            if cfg.with_bk:
                loss_warp = (loss_warp + _PhotoFn.apply(f21, im2, im1, occ2, *weights)) / 2.
                if smooth_on:
                    loss_smooth = (loss_smooth + self._smooth(f21, im2, s)) / 2.
            warp_loss = warp_loss + loss_warp * cfg.w_scales[i]
            smooth_sum = smooth_sum + loss_smooth * cfg.w_sm_scales[i]
        if smooth_on:
            smooth_loss = cfg.w_real_smooth * smooth_sum
            total_loss = warp_loss + smooth_loss
        else:
            smooth_loss = zero
            total_loss = warp_loss
        return total_loss, warp_loss, smooth_loss, pyramid_flows[0].abs().mean()
