"""Image export of the evaluation path (models/rcf_model.py:241-273): a stand-in for
`torchvision.utils.save_image` (make_grid + round-to-u8 + PIL encode), which the reference uses to write the
evaluation JPEG and the `pred_seg_*.png` masks that the offline stages (CRF post-processing, semantic
constraints) read back.  Host-side plumbing: nothing here is on the training hot path.
"""
import math
import os

import torch


def make_grid(t, nrow=8, padding=2, pad_value=0.0):
    """torchvision.utils.make_grid for a [B,C,H,W] (or [C,H,W] / [H,W]) float tensor, default arguments."""
    if t.dim() == 2:
        t = t.unsqueeze(0)
    if t.dim() == 3:
        if t.shape[0] == 1:
            t = torch.cat((t, t, t), 0)
        t = t.unsqueeze(0)
    if t.dim() == 4 and t.shape[1] == 1:
        t = torch.cat((t, t, t), 1)
    if t.shape[0] == 1:
        return t.squeeze(0)
    nmaps = t.shape[0]
    xmaps = min(nrow, nmaps)
    ymaps = int(math.ceil(float(nmaps) / xmaps))
    height, width = int(t.shape[2] + padding), int(t.shape[3] + padding)
    grid = t.new_full((t.shape[1], height * ymaps + padding, width * xmaps + padding), pad_value)
    k = 0
    for y in range(ymaps):
        for x in range(xmaps):
            if k >= nmaps:
                break
            grid.narrow(1, y * height + padding, height - padding).narrow(2, x * width + padding, width - padding).copy_(t[k])
            k += 1
    return grid


def to_uint8_hwc(t):
    """the rounding of torchvision.utils.save_image: x*255 + 0.5, clamp, truncate"""
    grid = make_grid(t)
    return grid.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to("cpu", torch.uint8).numpy()


def save_image(t, path):
    from PIL import Image                               # present in the image; fails loudly if not
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    Image.fromarray(to_uint8_hwc(t.detach().float())).save(path)


# ---- the batched route: one kernel call and one device -> host copy per batch, encoding on writer threads ---------------------
def grid_geometry(B, H, W, nrow=8, padding=2):
    """make_grid's canvas for B images of H x W as (canvas height, canvas width, offset of cell 0, cell height, cell width, cells
    per row): image k sits at row offset + (k // per_row) cell height, column offset + (k % per_row) cell width.  B == 1: the
    image itself (make_grid squeezes, no padding)."""
    if B == 1:
        return H, W, 0, H, W, 1
    xmaps = min(nrow, B)
    ymaps = int(math.ceil(float(B) / xmaps))
    return (H + padding) * ymaps + padding, (W + padding) * xmaps + padding, padding, H + padding, W + padding, xmaps


def _save_array(arr, path):
    from PIL import Image
    try:
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        Image.fromarray(arr).save(path)
    except Exception as e:                                  # the reference logs and carries on
        print(f"Error in saving: {path} {e}")


class _ExportSet:
    """one device buffer and its pinned twin, laid out for one batch geometry: [S, B, Ho, Wo, 3] PNG arrays, then the grid canvas"""

    def __init__(self, key, device):
        S, B, Ho, Wo, P = key
        self.key = key
        self.png_bytes = (S * B * Ho * Wo * 3 + 15) // 16 * 16
        self.grid = grid_geometry(B, P * Ho, Wo) if P else None
        nbytes = self.png_bytes + (self.grid[0] * self.grid[1] * 3 if P else 0)
        self.dev = torch.zeros(max(nbytes, 1), dtype=torch.uint8, device=device)      # the canvas padding stays 0: only windows are written
        self.host = torch.empty(max(nbytes, 1), dtype=torch.uint8).pin_memory()
        self.copied = None           # event: the last device -> host copy out of `dev` (copy stream)
        self.futures = []            # the writes that still read `host`

    def views(self, t):
        S, B, Ho, Wo, P = self.key
        png = t[:S * B * Ho * Wo * 3].view(S, B, Ho, Wo, 3) if S else None
        canvas = t[self.png_bytes:].view(self.grid[0], self.grid[1], 3) if P else None
        return png, canvas


class MaskExporter:
    """The evaluation export of a batch (SegModelBase._eval_outputs: the `pred_seg_*.png` masks and the grid JPEG) without a host
    synchronisation on the calling thread: ops.export_panels_u8 writes every panel into a device buffer, ONE non-blocking copy on a
    copy stream moves it into one of `sets` pinned buffers, and a pool of min(workers, 16) threads waits for that copy's event and
    encodes with Pillow into the file names the model writes today.  A pinned set is handed out again only after its writes have
    finished (the pattern of data_pipeline.BatchUploader.stage).  `flush()` blocks until everything is on disk; a failed write
    prints `Error in saving: ...` like the reference and is not raised.  sync=True does the same work inline."""

    MAX_WORKERS = 16

    def __init__(self, device, workers=4, sets=2, sync=False):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("MaskExporter writes device buffers: there is no CPU path")
        self.sync = bool(sync)
        self.workers = max(1, min(int(workers), self.MAX_WORKERS))
        self.sets = [None] * max(1, int(sets))
        self.cur = 0
        self.copy_stream = None if self.sync else torch.cuda.Stream(device=self.device)
        self.pool = None
        if not self.sync:
            from concurrent.futures import ThreadPoolExecutor
            self.pool = ThreadPoolExecutor(max_workers=self.workers, thread_name_prefix="rcf-export")
        self.batches = 0

    def pending(self):
        """writes handed to the pool that have not finished"""
        return sum(1 for s in self.sets if s is not None for f in s.futures if not f.done())

    @staticmethod
    def _wait(futures):
        for f in futures:
            f.result()                       # (_save_array catches its own errors)
        del futures[:]

    def flush(self):
        for s in self.sets:
            if s is not None:
                self._wait(s.futures)
                if s.copied is not None:
                    s.copied.synchronize()

    def close(self):
        self.flush()
        if self.pool is not None:
            self.pool.shutdown(wait=True)
            self.pool = None

    def submit(self, masks, frames, size, align_corners, png_channels=(), png_names=(), grid_sources=(), grid_name=None):
        """masks [B, C, h, w], frames [B, 3, H, W] (normalised; may be None without a grid).  png_channels: the mask channels
        written as PNGs, png_names[j][b] the file of channel png_channels[j] and sample b.  grid_sources: the panels of a sample
        from the top (ops.EXPORT_FRAME or a mask channel) of the grid JPEG `grid_name`."""
        from . import ops
        png_channels, grid_sources = list(png_channels), list(grid_sources) if grid_name is not None else []
        if not png_channels and not grid_sources:
            return
        B, (Ho, Wo) = masks.shape[0], (int(size[0]), int(size[1]))
        key = (len(png_channels), B, Ho, Wo, len(grid_sources))
        i = self.cur
        self.cur = (i + 1) % len(self.sets)
        s = self.sets[i]
        if s is not None:
            self._wait(s.futures)            # the set's pinned buffer is free again
        comp = torch.cuda.current_stream(self.device)
        if s is None or s.key != key:
            if s is not None and s.copied is not None:
                s.copied.synchronize()       # nothing queued still reads the buffers that are dropped here
            s = self.sets[i] = _ExportSet(key, self.device)
        elif s.copied is not None:
            comp.wait_event(s.copied)        # the previous copy out of this device buffer
        png_d, canvas_d = s.views(s.dev)
        layouts = []
        if png_channels:
            layouts.append(ops.export_contiguous_layout(png_d, png_channels))
        if grid_sources:
            _, cw, off, cell_h, cell_w, per_row = s.grid
            layouts.append(ops.export_layout(canvas_d, grid_sources, image=cell_w * 3, image_row=cell_h * cw * 3, slot=Ho * cw * 3,
                                             row=cw * 3, x=off, y=off, per_row=per_row))
        ops.export_panels_u8(masks, frames, layouts, (Ho, Wo), align_corners)
        png_h, canvas_h = s.views(s.host)
        jobs = [(png_h[j, b].numpy(), png_names[j][b]) for j in range(len(png_channels)) for b in range(B)]
        if grid_sources:
            jobs.append((canvas_h.numpy(), grid_name))
        self.batches += 1
        if self.sync:
            s.host.copy_(s.dev)              # blocking: the A/B leg and the debugging form
            for arr, fn in jobs:
                _save_array(arr, fn)
            return
        done = torch.cuda.Event()
        done.record(comp)
        self.copy_stream.wait_event(done)
        with torch.cuda.stream(self.copy_stream):
            s.host.copy_(s.dev, non_blocking=True)
            ready = torch.cuda.Event()
            ready.record(self.copy_stream)
        s.copied = ready

        def write(arr, fn):
            ready.synchronize()
            _save_array(arr, fn)
        s.futures = [self.pool.submit(write, arr, fn) for arr, fn in jobs]
