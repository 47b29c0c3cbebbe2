"""Edge cases of the optimiser passes (csrc/optim.hip: adam_kernel, ema_kernel, fill_kernel) and their reference.

Shared by tests/test_optim_sweep_cpu.py (the table reaches what it names; the reference's own float32 error) and
tests/test_optim_sweep_gpu.py (the kernels against the float64 truth).  The reference is the update of torch.optim.Adam
(coupled weight decay, no amsgrad) written out term by term in the dtype asked for; nothing of the HIP package enters this
module.

Launch geometry restated to CHOOSE sizes (never as a reference for a value): ew_blocks caps the grid at 4096 workgroups of 256
threads, so a thread's stride loop makes a second trip from n = 4096 * 256 + 1 and a third from 2 * 4096 * 256 + 1.

What each n is for:
  1              one element, 255 idle threads
  255 / 257      one thread short of a workgroup / a second workgroup with one element
  GRID - 1       the cap is reached, the last thread has nothing
  GRID + 5       five threads make a second trip
  2 GRID + 3     three threads make a third trip (the largest buffer of the sweep: 8 MB)

A run is four calls on one state: steps 1, 2, 3 and then one call numbered 1000 (bias corrections near 1 - 0.9^1000 = 1 and
1 - 0.999^1000 = 0.63 on moments three steps old).  (weight_decay, grad_scale) is (0, 1) or (1e-2, 1 / 1024).  The effective
gradients (after grad_scale) span 1e-6 .. 1e2 in magnitude with both signs; every tenth element (i % 10 == 3) has a zero
gradient in every call (with weight_decay = 0 both moments stay 0, the denominator is eps alone and p must not move), and a
further tenth is zero in any one call.  p0 = 1e-2 normal with lr = 1e-3: a sign-like update of 1e-3 is 1e6 ulp of p.

The hyper-parameters travel through the C ABI as float.  The truth is Adam at the values the kernel is handed -- beta2 =
float32(0.999) = 0.99900001287..., whose 1 - beta2 is 1.3e-5 (relative) off 0.001 -- as for every other input of the sweep: what
the caller's rounding of a hyper-parameter does is no statement about the kernel's arithmetic.  The bias corrections are
formed from those values in float64 (the entry point does the same and then rounds them to float: that rounding is the
kernel's).

Two comparisons, because a trajectory's error is mostly inherited: with weight decay, p's divergence after call 1 (below) comes
back through weight_decay * p into every later gradient, and a moment carries on what an earlier call cancelled.
  per call     every call of the run is compared with ONE float64 update from the very state that call started from (the
               kernel's own p, exp_avg, exp_avg_sq before the call): what is measured is that call's arithmetic and nothing
               else.  Errors are per element, scaled by the sum of the magnitudes of the addends that formed the element, so
               the cancellation between g and weight_decay * p is not charged to anybody:
                 exp_avg      beta1 |m| + (1 - beta1) (|g grad_scale| + |weight_decay p|)
                 exp_avg_sq   beta2 v + (1 - beta2) (|g grad_scale| + |weight_decay p|)^2
                 p            lr (one call's sign-like update)
               p is the sensitive one: where g grad_scale nearly cancels weight_decay * p the gradient is of the size of eps
               = 1e-8, the update lr g / (|g| + eps) turns on g's last bits, and among a million elements some do.
  trajectory   p after each call against the float64 trajectory from p0, in units of lr x calls (the project's own unit:
               test_adam_and_ema's error / total update).
"""
import dataclasses
import functools
import math

import numpy as np
import pytest
import torch

GRID = 4096 * 256
NS = (1, 255, 257, GRID - 1, GRID + 5, 2 * GRID + 3)
STEPS = (1, 2, 3, 1000)
HYPER = ((0.0, 1.0), (1e-2, 1.0 / 1024))                      # (weight_decay, grad_scale)
F32 = lambda v: float(np.float32(v))                          # the value a float argument of the C ABI carries
LR, B1, B2, EPS = F32(1e-3), F32(0.9), F32(0.999), F32(1e-8)
P0_SCALE = 1e-2
EMA_M = (0.0, 0.999, 1.0)
FILL_V = -2.5

# Floors.  Nothing in the project gives one for the moments, and for p only test_adam_and_ema's 5e-3 of the update, under which
# a missing bias correction passes.  Each is 4 x the float32 oracle's worst error over the final table (tests/
# test_optim_sweep_cpu.py prints them; profiles/optim_sweep_parity.txt), rounded up to one digit:
#   per call     p           1.54e-4 of lr          -> 6.2e-4 -> 7e-4   (n = GRID + 5 with weight decay, call 1: the cancellation above;
#                                                                        without weight decay the worst is 2.0e-6)
#                exp_avg     2.001e-7 of the addends -> 8.005e-7 -> 9e-7
#                exp_avg_sq  3.1e-7 of the addends  -> 1.2e-6 -> 2e-6
#   trajectory   p           1.54e-4 of lr x calls  -> 6.2e-4 -> 7e-4   (the same element, after call 1; never looser than 5e-3)
FLOOR_P, FLOOR_M, FLOOR_V, FLOOR_P_TRAJ = 7e-4, 9e-7, 2e-6, 7e-4


@dataclasses.dataclass(frozen=True)
class Run:
    n: int
    wd: float
    gs: float

    @property
    def name(self):
        return f"n{self.n}-wd{self.wd:g}-gs{self.gs:g}"


RUNS = [Run(n, F32(wd), gs) for n in NS for wd, gs in HYPER]
PARAMS = [pytest.param(r, id=r.name) for r in RUNS]


@functools.lru_cache(maxsize=2)
def inputs(run):
    """float32: p0 [n] and the four raw gradient buffers (the effective gradient is raw * grad_scale; 1 / grad_scale is a power
    of two, so the effective values are the ones drawn)"""
    g = torch.Generator().manual_seed(run.n % 100003 + (7 if run.wd else 0))
    n = run.n
    p0 = (P0_SCALE * torch.randn(n, generator=g)).float()
    always0 = torch.arange(n) % 10 == 3
    grads = []
    for _ in STEPS:
        eff = torch.pow(10.0, 8 * torch.rand(n, generator=g, dtype=torch.float64) - 6) * torch.sign(torch.randn(n, generator=g, dtype=torch.float64))
        eff[always0 | (torch.rand(n, generator=g) < 0.1)] = 0.0
        grads.append((eff / run.gs).float())
    return p0, tuple(grads)


def adam_call(p, graw, m, v, step, run):
    """one update in the dtype of the tensors, and the float64 scales of exp_avg and exp_avg_sq (from the same operands)"""
    g_s, wd_p = graw * run.gs, run.wd * p
    g = g_s + wd_p
    m_new = m + (1 - B1) * (g - m)                              # exp_avg.lerp_(grad, 1 - beta1)
    v_new = B2 * v + (1 - B2) * g * g
    bc1, bc2 = 1 - B1 ** step, 1 - B2 ** step
    denom = v_new.sqrt() / math.sqrt(bc2) + EPS
    p_new = p - (LR / bc1) * (m_new / denom)
    mag = g_s.abs().double() + wd_p.abs().double()
    return p_new, m_new, v_new, B1 * m.abs().double() + (1 - B1) * mag, B2 * v.double() + (1 - B2) * mag * mag


def trajectory(run, dtype):
    """[(p, exp_avg, exp_avg_sq)] after each of the four calls, from p0 and zero moments"""
    p0, grads = inputs(run)
    p, m, v = p0.to(dtype), torch.zeros(run.n, dtype=dtype), torch.zeros(run.n, dtype=dtype)
    out = []
    for step, graw in zip(STEPS, grads):
        p, m, v = adam_call(p, graw.to(dtype), m, v, step, run)[:3]
        out.append((p, m, v))
    return out


@functools.lru_cache(maxsize=2)
def truth(run):
    """the float64 trajectory, computed once and shared (callers leave it unchanged)"""
    return trajectory(run, torch.float64)


TINY = 1e-300


def scaled(got, ref, scale):
    """worst |got - ref| / scale over the elements; where the scale is 0 the value must be the reference's, exactly; NaN -> inf"""
    d = (got.double() - ref).abs()
    e = torch.where(scale > 0, d / scale.clamp_min(TINY), torch.where(d > 0, torch.tensor(math.inf, dtype=torch.float64), torch.zeros((), dtype=torch.float64)))
    return float("inf") if bool(torch.isnan(e).any()) else float(e.max())


def call_errors(before, got, run, call):
    """before / got: float32 (p, exp_avg, exp_avg_sq) on the CPU around call number `call` (1-based) of the run -> the errors of
    that call against one float64 update of `before`, and p against the float64 trajectory"""
    graw = inputs(run)[1][call - 1]
    p, m, v, sm, sv = adam_call(*(t.double() for t in (before[0], graw, before[1], before[2])), STEPS[call - 1], run)
    one = torch.ones((), dtype=torch.float64)
    return {"p": scaled(got[0], p, one * LR), "exp_avg": scaled(got[1], m, sm), "exp_avg_sq": scaled(got[2], v, sv),
            "p_traj": scaled(got[0], truth(run)[call - 1][0], one * (LR * call))}


FLOORS = {"p": FLOOR_P, "exp_avg": FLOOR_M, "exp_avg_sq": FLOOR_V, "p_traj": FLOOR_P_TRAJ}


def ema_ref(d, s, m):
    """the float32 formula of ema_kernel: d m + s (1 - m), every operation rounded to float32"""
    m32 = torch.tensor(m, dtype=torch.float32)
    return d * m32 + s * (torch.tensor(1.0, dtype=torch.float32) - m32)


@functools.lru_cache(maxsize=2)
def ema_inputs(n):
    g = torch.Generator().manual_seed(n % 100003 + 11)
    return torch.randn(n, generator=g), torch.randn(n, generator=g) * 3
