"""Flow colours and the training visualisation grid (models/rcf_model.py:222-234,456-462,562-608, models/amd/amd_model.py:213-262).

`flow_to_color` has the signature of the `flow_vis` package's function and runs on the device colour kernel (ops.flow_color,
csrc/flowvis.hip).  The grid is one image per (frame, sample), the panels stacked along dimension 2 as the reference's
`torch.cat(..., dim=2)` stacks them: the M mask panels, the frame, the flow panels, then the pseudo-label mask when there is one.
`grid_panels` names the panels in order, `assemble_grid` is the reference's concatenation for panels given as tensors (host or
device; the tests rebuild a grid with it), `new_canvas` / `panel` are what the models write into directly.
"""
import numpy as np
import torch

from . import ops

RCF_FLOW_KINDS = ("pred", "gt", "agg", "aff", "adj")          # the reference's order: Pred, GT, Agg, Affine, Adj
AMD_FLOW_KINDS = ("seg", "whole")


def flow_to_color(flow_uv, clip_flow=None, convert_to_bgr=False):
    """flow_vis.flow_to_color: [h, w, 2] float32 flow -> [h, w, 3] uint8 colours, of the same kind as the input (a CUDA tensor, or
    a numpy array that is uploaded, coloured and brought back)."""
    assert flow_uv.ndim == 3, "input flow must have three dimensions"
    assert flow_uv.shape[2] == 2, "input flow must have shape [H,W,2]"
    is_numpy = isinstance(flow_uv, np.ndarray)
    t = torch.from_numpy(np.ascontiguousarray(flow_uv, dtype=np.float32)).cuda() if is_numpy else flow_uv
    out = torch.empty(tuple(t.shape[:2]) + (3,), dtype=torch.uint8, device=t.device)
    ops.flow_color(t.permute(2, 0, 1), out=out.permute(2, 0, 1), convert_to_bgr=convert_to_bgr, clip_flow=clip_flow)
    return out.cpu().numpy() if is_numpy else out


def rcf_flow_kinds(affine):
    return tuple(k for k in RCF_FLOW_KINDS if affine or k != "aff")


def grid_panels(mask_layer, flow_kinds, with_pl=False):
    """the panels of one grid image in stacking order; panel i covers rows [i h, (i + 1) h) of the [2B, 3, P h, w] grid"""
    return [f"mask{m}" for m in range(mask_layer)] + ["frame"] + [f"flow_{k}" for k in flow_kinds] + (["pl"] if with_pl else [])


def assemble_grid(masks, frames, flows, pl=None):
    """The reference's concatenation.  masks [I, B, M, h, w], frames [I, B, 3, h, w] (already (x + 2) / 4), flows: one [I, B, 3, h, w]
    colour tensor (values 0 .. 1) per kind, pl [I, B, h, w] or None -> [I B, 3, P h, w]: rows 0 .. B - 1 are frame 0."""
    I, B, M, h, w = masks.shape
    panels = [masks[:, :, m:m + 1].expand(I, B, 3, h, w) for m in range(M)] + [frames] + list(flows)
    if pl is not None:
        panels.append(pl[:, :, None].expand(I, B, 3, h, w))
    return torch.cat([p.reshape(I * B, 3, h, w).float() for p in panels], dim=2)


def new_canvas(I, B, panels, h, w, device):
    return torch.empty((I * B, 3, len(panels) * h, w), dtype=torch.float32, device=device)


def panel(canvas, panels, name, I, count=1):
    """the window of `count` consecutive panels starting at `name`: a view [I, B, 3, count, h, w] of the canvas"""
    N, _, Ph, w = canvas.shape
    h = Ph // len(panels)
    i = panels.index(name)
    return canvas.view(I, N // I, 3, len(panels), h, w)[:, :, :, i:i + count]


def fill_grid(canvas, panels, masks, frames, flows, pl=None):
    """masks [I, B, M, h, w] (any strides), frames [I B, 3, h, w] frame-major (already (x + 2) / 4), flows [I B, K, 2, h, w]
    frame-major (row i B + b holds sample b's K flow images of frame i), pl [I, B, h, w] or None.  The flow panels are coloured
    straight into their window by ONE ops.flow_color call; the other panels are strided copies."""
    I, B, M, h, w = masks.shape
    K = flows.shape[1]
    panel(canvas, panels, "mask0", I, M).copy_(masks[:, :, None])
    panel(canvas, panels, "frame", I)[:, :, :, 0].copy_(frames.view(I, B, 3, h, w))
    window = canvas.view(I * B, 3, len(panels), h, w)[:, :, M + 1:M + 1 + K]         # the K flow panels of every grid image
    ops.flow_color(flows, out=window.permute(0, 2, 1, 3, 4))                           # [I B, K, 3, h, w], a view: nothing is copied
    if pl is not None:
        panel(canvas, panels, "pl", I)[:, :, :, 0].copy_(pl[:, :, None])
    return canvas
