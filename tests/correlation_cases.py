"""Edge-shape cases of the cost-volume kernels (csrc/correlation.hip) and their float64 reference.

Shared by tests/test_correlation_cpu.py (the restatement equals the reference-made fixture tests/golden/correlation.npz; the table
reaches the branches it names) and tests/test_correlation_gpu.py (the kernels against the restatement).  numpy / torch on the
CPU; of the HIP package only the pure query rcf_correlation_geometry enters, so that the shapes sit on the kernel's real edges.

The restatement writes include/rcf_hip.h's three formulas out in float64 over the zero-padded operand -- the zeros are
MULTIPLIED (numpy makes inf * 0 = NaN as the kernels and F.pad's zeros do) -- and returns with every result its MASS, the same
sum over absolute values.  Bounds, u = 2^-24 (`U`), per element:
  forward         |err| <= (C + 2) u mass      C products and C - 1 additions in any order, the division by C, the activation.
                  mass is the one BEFORE the activation: where rounding moves corr across zero the error of out is still at most
                  the error of corr (corr and its error have opposite signs there), so the unscaled mass covers both branches.
  each gradient   |err| <= (D^2 + 2) u mass    the mask product, D^2 products and D^2 - 1 additions, the division by C.
Non-finite positions must equal the restatement's exactly (`margin` returns inf otherwise).  Overflow: float32 overflows where
float64 does not, so the restatement rounds corr to float32 BEFORE the activation and takes +-inf where that rounding gives it;
the `huge` inputs keep every other sum far from the float32 range's end (one +-3e38 channel, partners either within [-1, 1] or
+-3e38 themselves; dout scaled to 0.01 so that no gradient sum overflows).

With slope != 1 the backward takes the caller's `out`; the tests hand it a random tensor with exact zeros in it and the
restatement the same one, so there is no tie set.
"""
import dataclasses
import functools

import numpy as np
import torch

import rcf_amd  # noqa: F401  (package alias)
from rcf_amd import _lib

U = 2.0 ** -24
f32 = np.float32
GOLDEN_SHAPES = [(2, 3, 1, 7, 4), (1, 5, 3, 3, 1), (1, 7, 4, 6, 2), (2, 33, 9, 11, 4), (1, 192, 8, 14, 4)]       # B, C, H, W, d
COMPOSITION_SHAPE = (2, 33, 9, 11, 4)


@functools.lru_cache(maxsize=1)
def geometry():
    """(tile rows, tile columns, channels per trip) of csrc/correlation.hip"""
    lib = _lib.load()
    return tuple(int(lib.rcf_correlation_geometry(k)) for k in range(3))


# ============================================================================================================ restatement
def _pad(a, d):
    return np.pad(a, ((0, 0), (0, 0), (d, d), (d, d)))


def act_factor(out, slope):
    """out > 0 ? 1 : slope, the slope as the float32 the kernels receive"""
    return np.where(np.asarray(out) > 0, 1.0, float(f32(slope)))


def corr_ref(x1, x2, d, slope=1.0):
    """x1, x2 [B, C, H, W] -> (out, mass) float64 [B, D D, H, W]"""
    a, bz = x1.astype(np.float64), _pad(x2.astype(np.float64), d)
    B, C, H, W = a.shape
    D = 2 * d + 1
    out, mass = np.empty((B, D * D, H, W)), np.empty((B, D * D, H, W))
    with np.errstate(all="ignore"):
        for i in range(D):
            for j in range(D):
                win = bz[:, :, i:i + H, j:j + W]
                out[:, i * D + j] = (a * win).sum(1) / C
                mass[:, i * D + j] = (np.abs(a) * np.abs(win)).sum(1) / C
        r32 = out.astype(np.float32)
        out = np.where(np.isinf(r32), r32.astype(np.float64), out)          # float32's overflow, before the activation
        if slope != 1.0:
            out = out * act_factor(out, slope)
    return out, mass


def corr_bwd_ref(x1, x2, dout, d, slope=1.0, out=None):
    """-> (dx1, mass1, dx2, mass2) float64 [B, C, H, W]; `out` (needed when slope != 1) is the tensor whose sign masks dout"""
    a, b, g = x1.astype(np.float64), x2.astype(np.float64), dout.astype(np.float64)
    B, C, H, W = a.shape
    D = 2 * d + 1
    with np.errstate(all="ignore"):
        if slope != 1.0:
            g = g * act_factor(out, slope)
        bz = _pad(b, d)
        dx1, m1 = np.zeros_like(a), np.zeros_like(a)
        s2, m2 = np.zeros_like(bz), np.zeros_like(bz)           # the scatter into the padded copy; its border is dropped
        for i in range(D):
            for j in range(D):
                gk = g[:, i * D + j][:, None]
                win = bz[:, :, i:i + H, j:j + W]
                dx1 += gk * win
                m1 += np.abs(gk) * np.abs(win)
                s2[:, :, i:i + H, j:j + W] += gk * a
                m2[:, :, i:i + H, j:j + W] += np.abs(gk) * np.abs(a)
        inner = (slice(None), slice(None), slice(d, d + H), slice(d, d + W))
        return dx1 / C, m1 / C, s2[inner] / C, m2[inner] / C


def fwd_bound(mass, C):
    return (C + 2) * U * mass


def grad_bound(mass, d):
    return ((2 * d + 1) ** 2 + 2) * U * mass


def margin(got, ref, bound):
    """worst |got - ref| / bound over the finite elements of ref; inf when the non-finite elements differ (NaN where NaN, +-inf where
    the same infinity), when got is non-finite where ref is finite, or when an error sits under a zero bound"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape
    fin = np.isfinite(ref)
    if not np.array_equal(np.isnan(got), np.isnan(ref)) or not np.array_equal(got[np.isinf(ref)], ref[np.isinf(ref)]):
        return float("inf")
    if not np.isfinite(got[fin]).all():
        return float("inf")
    e = np.abs(got[fin] - ref[fin])
    if not e.size:
        return 0.0
    with np.errstate(all="ignore"):
        r = np.where(e == 0, 0.0, e / np.asarray(bound)[fin])
    return float(r.max())


# ================================================================================================================== cases
KINDS = ("gauss", "exact", "nan", "inf", "huge")


@dataclasses.dataclass(frozen=True)
class Case:
    B: int
    C: int
    H: int
    W: int
    d: int
    slope: float = 1.0
    kind: str = "gauss"

    @property
    def name(self):
        return f"b{self.B}-c{self.C}-{self.H}x{self.W}-d{self.d}-s{self.slope:g}-{self.kind}"

    @property
    def D(self):
        return 2 * self.d + 1

    @property
    def seed(self):
        return ((self.B * 211 + self.C) * 223 + self.H) * 227 + self.W * 11 + self.d + 5 * KINDS.index(self.kind) + (3 if self.slope != 1.0 else 0)


def _cases():
    TH, TW, CK = geometry()
    out = []
    # H, W in {1, 2, d, d + 1, 2 d + 1}, cyclic neighbours so that H != W: images smaller than the search window
    for d in (1, 2, 3, 4):
        v = sorted({1, 2, d, d + 1, 2 * d + 1})
        out += [Case(3 if k == 1 else 1, 3, v[k], v[(k + 1) % len(v)], d) for k in range(len(v))]
    # one below, at and above the tile's height and width, two tiles plus 3
    out += [Case(1, 3, TH - 1, TW, 4), Case(1, 2, TH, TW + 1, 4), Case(1, 3, TH + 1, TW - 1, 4), Case(1, 2, 2 * TH + 3, 2 * TW + 3, 2),
            Case(3, 2, TH + 1, 2 * TW + 3, 1), Case(1, 3, 2 * TH + 3, TW - 1, 3)]
    # channels: 1, 2, 3, around the chunk, 32, 33, 192
    out += [Case(1, C, 5, 6, 2) for C in (1, 2, CK - 1, CK, CK + 1)] + [Case(1, C, 3, 5, 4) for C in (32, 33, 192)]
    out += [Case(1, 2 * CK + 1, TH + 1, 5, 3)]
    # B = 3 with every d
    out += [Case(3, 4, d + 1, 2 * d + 2, d) for d in (1, 2, 3, 4)]
    # the fused LeakyReLU
    out += [Case(1, 3, 2, 9, 4, 0.1), Case(3, CK + 1, 4, 3, 1, 0.1), Case(1, 2, TH + 1, TW + 1, 2, 0.1), Case(1, 33, 5, 4, 3, 0.1),
            Case(1, 1, 9, 5, 4, 0.1), Case(1, 3, 1, 2, 4, 0.1)]
    # out == x2z, bit for bit
    out += [Case(2, 1, d, 2 * d + 2, d, kind="exact") for d in (1, 2, 3, 4)] + [Case(1, 1, TH + 1, TW + 3, 4, kind="exact")]
    # non-finite operands
    for s in (1.0, 0.1):
        out += [Case(1, 3, 5, 7, 4, s, "nan"), Case(2, 2, 6, 5, 2, s, "inf"), Case(1, 3, 7, 6, 4, s, "inf"), Case(2, 3, 6, 9, 3, s, "huge")]
    assert len({c.name for c in out}) == len(out)
    return out


CASES = _cases()


def exact_x2(c):
    """a distinct small integer per pixel and image (1 ..): float32 holds them, and their products with 1, exactly"""
    n = c.B * c.H * c.W
    return np.arange(1, n + 1, dtype=np.float32).reshape(c.B, 1, c.H, c.W)


@functools.lru_cache(maxsize=8)
def inputs(c):
    """float32 numpy x1, x2 [B, C, H, W], dout [B, D D, H, W] and `mask_out` (the `out` the backward is handed when slope != 1: random,
    30 % exact zeros).  Callers leave them unchanged."""
    g = torch.Generator().manual_seed(c.seed)
    B, C, H, W, D = c.B, c.C, c.H, c.W, c.D
    x1, x2 = torch.randn(B, C, H, W, generator=g).numpy(), torch.randn(B, C, H, W, generator=g).numpy()
    dout = torch.randn(B, D * D, H, W, generator=g).numpy()
    mask_out = (torch.randn(B, D * D, H, W, generator=g) * (torch.rand(B, D * D, H, W, generator=g) > 0.3)).numpy()
    if c.kind == "exact":
        x1, x2 = np.ones_like(x1), exact_x2(c)
    elif c.kind == "nan":
        x2[0, 1, H // 2, W // 2] = np.nan                          # one pixel of one channel
    elif c.kind == "inf":
        y, x = ((0, 0), (H - 1, W - 1))[c.d % 2]                   # an image corner: displacements that leave the image meet padding
        x1[0, 0, y, x] = np.inf
    elif c.kind == "huge":
        x1, x2 = np.clip(x1 / 3, -1, 1), np.clip(x2 / 3, -1, 1)
        k1, k2 = torch.rand(B, H, W, generator=g).numpy(), torch.rand(B, H, W, generator=g).numpy()
        x1[:, 0] = np.where(k1 < 0.15, f32(3e38), np.where(k1 < 0.3, f32(-3e38), x1[:, 0]))
        x2[:, 0] = np.where(k2 < 0.15, f32(3e38), np.where(k2 < 0.3, f32(-3e38), x2[:, 0]))
        dout = dout.clip(-1, 1) * f32(0.01)
    return dict(x1=np.ascontiguousarray(x1, dtype=np.float32), x2=np.ascontiguousarray(x2, dtype=np.float32),
                dout=np.ascontiguousarray(dout, dtype=np.float32), mask_out=np.ascontiguousarray(mask_out, dtype=np.float32))


@functools.lru_cache(maxsize=4)
def fwd_truth(c):
    d = inputs(c)
    return corr_ref(d["x1"], d["x2"], c.d, c.slope)


@functools.lru_cache(maxsize=4)
def bwd_truth(c):
    d = inputs(c)
    return corr_bwd_ref(d["x1"], d["x2"], d["dout"], c.d, c.slope, d["mask_out"] if c.slope != 1.0 else None)


def torch_composition(x1, x2, d, slope=1.0):
    """the 81-slice composition of models/amd/correlation_native.py restated in torch (any device, any dtype; autograd follows), with
    PWC-Lite's LeakyReLU when slope != 1"""
    H, W = x1.shape[2:]
    D = 2 * d + 1
    x2p = torch.nn.functional.pad(x2, [d] * 4)
    cv = [torch.mean(x1 * x2p[:, :, i:i + H, j:j + W], 1, keepdim=True) for i in range(D) for j in range(D)]
    out = torch.cat(cv, 1)
    return out if slope == 1.0 else torch.nn.functional.leaky_relu(out, slope)
