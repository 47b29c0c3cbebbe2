"""AMDModel -- the AMD baseline (models/amd/amd_model.py) end to end on the native path: drop-in for the reference's class, same
constructor keywords (the YAML under `model_kwargs` of configs/amd/amd.yaml), same state-dict keys (`backbone2.*`,
`decode_head.flownet.*`, `decode_head2.*`), same return contract (training: the 0-dim tensor w_seg * loss_seg whose `.backward()`
fills every parameter's `.grad`; evaluation: the softmax masks of frame 0, [B, M, h, w]).

Two autograd worlds meet here.  The segmentation network (`backbone2`, `decode_head2`) runs on the HIP tape exactly as in RCFModel;
the flow network and its loss (`decode_head`: PWCLite, unFlowLoss) are torch autograd Functions over native kernels.  `_MaskBridge`
is the seam: its inputs are the tape's trainable parameters, its outputs the frames' softmax masks (ops.mask_softmax, frame-major,
so that each frame's mask is the contiguous tensor PWCLite.forward takes); its backward turns the mask gradients into the logits'
gradient (ops.mask_softmax_bwd), runs the tape and hands the parameters' gradients back to autograd -- so `loss.backward()` reaches
every parameter, torch DDP's hooks see each one once, and the flow network's parameters get theirs from torch autograd.

float32 only: the flow network has no 16-bit path.  The training visualisations every `log_interval` steps (amd_model.py:213-264)
are written as for RCFModel (SegModelBase.train_vis_due, flowvis.py): masks, frame, segment flow and whole-image flow of every
sample, the flows coloured on the device.  Only such a step computes the whole-image flows and their loss, which nothing else reads
(flow_forward(need_whole=True)); every other step skips them."""
import torch

from . import flowvis, ops
from .layers import Tape
from .model import REGISTRY, SegModelBase, grads_through_flat_buffer


class _MaskBridge(torch.autograd.Function):
    """(the tape's trainable parameters) -> the I frames' softmax masks [B, M, h, w], views of one frame-major buffer"""

    @staticmethod
    def forward(ctx, logits, tape, B, I, M, *params):
        masks = ops.mask_softmax(logits.t, B, I, M)
        ctx.logits, ctx.tape, ctx.masks, ctx.params = logits, tape, masks, params
        ctx.set_materialize_grads(False)             # a frame whose mask no loss read arrives as None: the kernel takes it as zeros
        return tuple(masks[i] for i in range(I))

    @staticmethod
    def backward(ctx, *dmasks):
        logits, tape, masks = ctx.logits, ctx.tape, ctx.masks

        def run():
            logits.grad = ops.mask_softmax_bwd(masks, list(dmasks), logits.t.shape[3])
            tape.backward()
        return (None,) * 5 + grads_through_flat_buffer(list(ctx.params), run)


class AMDModel(SegModelBase):
    def __init__(self, args, backbone2, decode_head, decode_head2, w_seg=2.0, mask_layer=1, train_iter=0, train_cfg=None,
                 test_cfg=None, log_interval=50):
        super().__init__()
        self._init_dirs(args)

        def build(cfg):                              # like the reference (amd_model.py:39,63-69) this pops 'type' from the caller's dict
            return REGISTRY[cfg.pop("type")](**cfg)
        self.backbone2 = build(backbone2)
        self.mask_layer = mask_layer
        self.decode_head = build(decode_head)
        self.decode_head2 = build(decode_head2)
        if not getattr(self.decode_head, "create_flownet", False):
            raise NotImplementedError("AMDModel: decode_head must be an FCNHead with create_flownet=True (it holds the flow network)")
        if self.decode_head.mask_layer != mask_layer or self.decode_head2.num_classes != mask_layer:
            raise ValueError(f"mask_layer {mask_layer} must be decode_head.mask_layer and decode_head2.num_classes")
        self.align_corners, self.num_classes = self.decode_head2.align_corners, self.decode_head2.num_classes
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self.backbone2.init_weights()
        self.train_iter, self.w_seg, self.log_interval = train_iter, w_seg, log_interval
        self.register_load_state_dict_post_hook(lambda module, incompatible_keys: ops.weights_changed())
        self.precision = None            # None or "fp32"; anything else raises (_select_precision)
        self.dist = None
        self._loss = None                # the last training forward's loss with its graph (run_backward)
        self._act_dtype = torch.float32

    def _select_precision(self):
        autocast = torch.is_autocast_enabled("cuda") or torch.is_autocast_enabled("cpu")
        if self.precision not in (None, "fp32") or autocast:
            raise NotImplementedError("AMDModel runs in float32 only: the flow network (PWCLite) has no 16-bit path -- "
                                      f"precision {self.precision!r}, autocast {'on' if autocast else 'off'}")
        return "fp32"

    def run_backward(self, grad_out=None):
        """Backward of the last forward_train with the loss scaled by grad_out: fills param.grad (accumulating)."""
        if self._loss is None:
            raise RuntimeError("backward called twice or before forward")
        loss, self._loss = self._loss, None
        loss.backward(None if grad_out is None else torch.full_like(loss, float(grad_out)))

    # ------------------------------------------------------------------ training forward (amd_model.py:194-266)
    def forward_train(self, imgs, seq_ids=None, seq_names=None, paths=None):
        B, I = imgs.shape[:2]
        assert I == 2, "Other im_num not implemented"          # amd_model.py:207,236
        self._select_precision()
        dist = self._dist()
        tape = Tape(act_dtype=torch.float32)
        logits = self.decode_head2.fwd(self.backbone2.fwd(self._images_nhwc(imgs), tape, dist), tape, dist)     # Act [B*I,h,w,Cp]
        self.last_logits = logits.t
        params = [p for m in (self.backbone2, self.decode_head2) for p in m.parameters() if p.requires_grad]
        vis_due = self.train_vis_due(paths)
        with torch.enable_grad():        # also under a trainer's no_grad: run_backward differentiates the stored loss
            masks = _MaskBridge.apply(logits, tape, B, I, self.mask_layer, *params)
            flows, flow_loss, _, _, _ = self.decode_head.flow_forward(imgs, list(masks), need_whole=vis_due)
            loss = flow_loss["seg"] * self.w_seg
        self._loss = loss
        if vis_due:
            self._write_train_vis(imgs, masks, flows, seq_ids, seq_names, paths)
        self.train_iter += 1
        return loss if torch.is_grad_enabled() else loss.detach()

    @torch.no_grad()
    def _write_train_vis(self, imgs, masks, flows, seq_ids, seq_names, paths):
        """amd_model.py:207-264: the M mask panels, the frame, the segment and the whole-image flow (normalised, resized to the mask
        shape; frame 0 from the first two channels, frame 1 from the last two) of every sample as one JPEG"""
        B, I = imgs.shape[:2]
        h, w = masks[0].shape[-2:]
        assert len(flows["seg"]) == 1 and len(flows["whole"]) == 1
        kinds = flowvis.AMD_FLOW_KINDS
        fl = torch.stack([self.resize(flows[k][0].detach(), (h, w)) for k in kinds], 1)               # [B, K, 4, h, w]
        fl = fl.view(B, len(kinds), I, 2, h, w).permute(2, 0, 1, 3, 4, 5).contiguous().view(I * B, len(kinds), 2, h, w)
        tosave = self.train_grid(torch.stack([m.detach() for m in masks]), imgs, fl, kinds)
        self.save_train_visualizations(tosave, paths, seq_ids, seq_names)

    # ------------------------------------------------------------------ eval forward (amd_model.py:155-192)
    @torch.no_grad()
    def forward_eval(self, imgs, seq_ids=None, seq_names=None, paths=None, return_pred_vis_list=False):
        B, I = imgs.shape[:2]
        self._select_precision()
        t = Tape(enabled=False)
        logits = self.decode_head2.fwd(self.backbone2.fwd(self._images_nhwc(imgs), t), t)
        pred_masks = ops.mask_softmax(logits.t, B, I, self.mask_layer)[0]
        return self._eval_outputs(imgs, pred_masks, seq_ids, seq_names, paths, return_pred_vis_list)

    def forward(self, x, return_pred_vis_list=False):
        imgs = torch.stack(x["imgs"], dim=1)
        if self.training:
            return self.forward_train(imgs, x.get("seq_ids"), x.get("seq_names"), x.get("paths"))
        return self.forward_eval(imgs, x.get("seq_ids"), x.get("seq_names"), x.get("paths"), return_pred_vis_list)


REGISTRY["AMDModel"] = AMDModel
