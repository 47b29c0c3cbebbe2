"""PWC-Lite's cost volume as a module (models/amd/correlation_native.py:6-23) on the native kernels of csrc/correlation.hip.

`Correlation(max_displacement=4)` keeps the reference's constructor -- further positional and keyword arguments (the external
CUDA package's kernel_size, stride1, ... that models/amd/pwc_lite.py passes) are accepted and ignored -- and its `output_dim` /
`pad_size` attributes.  `slope=0.1` fuses the LeakyReLU that PWC-Lite applies to every cost volume (pwc_lite.py:202-203).
forward(x1, x2) goes through one autograd Function over ops.correlation / ops.correlation_bwd, so a torch graph around it trains.
There is no CPU path: a CPU tensor raises RcfHipError."""
import torch
import torch.nn as nn

from . import ops

MAX_DISPLACEMENTS = (1, 2, 3, 4)          # what csrc/correlation.hip instantiates


class _CorrelationFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x1, x2, max_displacement, slope):
        out = ops.correlation(x1, x2, max_displacement, slope)
        ctx.max_displacement, ctx.slope = max_displacement, slope
        ctx.save_for_backward(x1, x2, out if slope != 1.0 else None)
        return out

    @staticmethod
    def backward(ctx, dout):
        x1, x2, out = ctx.saved_tensors
        need1, need2 = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        dx1 = dx2 = None
        if need1 or need2:
            dx1, dx2 = ops.correlation_bwd(x1, x2, dout, out, ctx.max_displacement, ctx.slope, need1, need2)
        return dx1, dx2, None, None


class Correlation(nn.Module):
    def __init__(self, max_displacement=4, *args, slope=1.0, **kwargs):
        super().__init__()
        if max_displacement not in MAX_DISPLACEMENTS:
            raise NotImplementedError(f"max_displacement {max_displacement!r}: the native cost volume is built for {MAX_DISPLACEMENTS}")
        self.max_displacement = int(max_displacement)
        self.output_dim = 2 * self.max_displacement + 1
        self.pad_size = self.max_displacement
        self.slope = float(slope)

    def forward(self, x1, x2):
        return _CorrelationFn.apply(x1, x2, self.max_displacement, self.slope)
