"""Conditioning of the cost-volume sweep (tests/correlation_cases.py) and the host side of the op, without a GPU: the float64
restatement equals the reference-made fixture (tests/golden/correlation.npz) within 1e-12 and the fixture's float32 forward lies
inside the forward bound; a float32 run of the 81-slice composition on random inputs stays inside every bound the GPU test
applies (a kernel that misses one is wrong, not unlucky); the case table reaches the branches it names, judged by the kernel's own
geometry query; the non-finite cases do what they promise; `Correlation` keeps the reference's constructor; the entry points
refuse bad arguments before they touch a device."""
import ctypes
import os

import numpy as np
import pytest
import torch

import correlation_cases as cc
import rcf_amd
from rcf_amd import _lib

T = torch.from_numpy


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "correlation.npz"))


# ----------------------------------------------------------------------------------------------------- against the reference
def test_fixture_is_small_and_holds_the_five_shapes(golden, golden_dir):
    assert os.path.getsize(os.path.join(golden_dir, "correlation.npz")) < 200 * 1024
    assert [tuple(int(v) for v in s) for s in golden["shapes"]] == cc.GOLDEN_SHAPES
    for k, (B, C, H, W, d) in enumerate(cc.GOLDEN_SHAPES):
        D = 2 * d + 1
        assert golden[f"x1_{k}"].shape == golden[f"x2_{k}"].shape == golden[f"dx1_64_{k}"].shape == golden[f"dx2_64_{k}"].shape == (B, C, H, W)
        assert golden[f"dout_{k}"].shape == golden[f"out64_{k}"].shape == golden[f"out32_{k}"].shape == (B, D * D, H, W)
        assert golden[f"out64_{k}"].dtype == np.float64 and golden[f"out32_{k}"].dtype == np.float32


@pytest.mark.parametrize("k", range(len(cc.GOLDEN_SHAPES)))
def test_restatement_equals_the_reference(golden, k):
    B, C, H, W, d = cc.GOLDEN_SHAPES[k]
    x1, x2, dout = golden[f"x1_{k}"], golden[f"x2_{k}"], golden[f"dout_{k}"]
    out, mass = cc.corr_ref(x1, x2, d)
    dx1, m1, dx2, m2 = cc.corr_bwd_ref(x1, x2, dout, d)
    e = [float(np.abs(a - golden[n]).max()) for a, n in ((out, f"out64_{k}"), (dx1, f"dx1_64_{k}"), (dx2, f"dx2_64_{k}"))]
    print(f"correlation golden {cc.GOLDEN_SHAPES[k]}: restatement vs the reference's float64 run, max abs difference out {e[0]:.1e} dx1 {e[1]:.1e} dx2 {e[2]:.1e}")
    assert max(e) <= 1e-12
    assert np.abs(golden[f"dx1_64_{k}"]).max() > 1 and np.abs(golden[f"dx2_64_{k}"]).max() > 1 and np.abs(out).max() > 0.1
    m = cc.margin(golden[f"out32_{k}"], out, cc.fwd_bound(mass, C))
    print(f"correlation golden {cc.GOLDEN_SHAPES[k]}: the reference's float32 forward, worst error / bound {m:.3f}")
    assert m <= 1.0


@pytest.mark.parametrize("shape", cc.GOLDEN_SHAPES + [(1, 8, 9, 33, 4), (2, 3, 2, 9, 4), (1, 32, 5, 6, 3)], ids=str)
@pytest.mark.parametrize("slope", [1.0, 0.1])
def test_float32_composition_is_inside_the_bounds(shape, slope):
    """random normal inputs: what the reference's arithmetic does in float32 (torch on the CPU, autograd for the gradients) against
    the restatement.  With slope != 1 the gradient mask comes from the float32 run's own output, which the restatement is handed,
    as the GPU test hands the kernel and the restatement one tensor."""
    B, C, H, W, d = shape
    g = torch.Generator().manual_seed(sum(shape) + int(10 * slope))
    D = 2 * d + 1
    x1, x2 = torch.randn(B, C, H, W, generator=g).requires_grad_(True), torch.randn(B, C, H, W, generator=g).requires_grad_(True)
    dout = torch.randn(B, D * D, H, W, generator=g)
    o = cc.torch_composition(x1, x2, d, slope)
    o.backward(dout)
    a, b = x1.detach().numpy(), x2.detach().numpy()
    out, mass = cc.corr_ref(a, b, d, slope)
    dx1, m1, dx2, m2 = cc.corr_bwd_ref(a, b, dout.numpy(), d, slope, o.detach().numpy())
    m = (cc.margin(o.detach().numpy(), out, cc.fwd_bound(mass, C)), cc.margin(x1.grad.numpy(), dx1, cc.grad_bound(m1, d)),
         cc.margin(x2.grad.numpy(), dx2, cc.grad_bound(m2, d)))
    print(f"correlation {shape} slope {slope}: float32 composition error / bound: out {m[0]:.3f} dx1 {m[1]:.3f} dx2 {m[2]:.3f}")
    assert max(m) <= 1.0


def test_restatement_equals_the_composition_in_float64():
    """the torch restatement the GPU test and tools/time_correlation.py run, against the numpy one, with the activation"""
    B, C, H, W, d = cc.COMPOSITION_SHAPE
    g = torch.Generator().manual_seed(33)
    x1, x2 = torch.randn(B, C, H, W, generator=g).double().requires_grad_(True), torch.randn(B, C, H, W, generator=g).double().requires_grad_(True)
    dout = torch.randn(B, 81, H, W, generator=g).double()
    for slope in (1.0, 0.1):
        x1.grad = x2.grad = None
        o = cc.torch_composition(x1, x2, d, slope)
        o.backward(dout)
        out, mass = cc.corr_ref(x1.detach().numpy(), x2.detach().numpy(), d, slope)
        dx1, m1, dx2, m2 = cc.corr_bwd_ref(x1.detach().numpy(), x2.detach().numpy(), dout.numpy(), d, slope, o.detach().numpy())
        # float32(0.1) is the slope of the restatement (what the kernel receives), 0.1 the composition's: 1.5e-8 apart
        tol = 1e-12 if slope == 1.0 else 2e-8
        assert np.abs(out - o.detach().numpy()).max() <= tol * max(1.0, np.abs(out).max())
        assert np.abs(dx1 - x1.grad.numpy()).max() <= tol * m1.max() and np.abs(dx2 - x2.grad.numpy()).max() <= tol * m2.max()


# ------------------------------------------------------------------------------------------------------------ the case table
def test_table_reaches_every_branch():
    TH, TW, CK = cc.geometry()
    assert TH > 0 and TW > 0 and CK > 0 and TH * TW == 256 and _lib.load().rcf_correlation_geometry(3) == 0
    cs = cc.CASES
    assert 50 <= len(cs) <= 70
    assert all(c.H != c.W for c in cs)                                                  # a transposed tile shows
    assert max(c.B * c.D ** 2 * c.H * c.W for c in cs) <= 40000 and max(c.B * c.C * c.H * c.W for c in cs) <= 8000
    for d in (1, 2, 3, 4):
        of_d = [c for c in cs if c.d == d]
        assert {1, 2, d, d + 1, 2 * d + 1} <= {c.H for c in of_d} and {1, 2, d, d + 1, 2 * d + 1} <= {c.W for c in of_d}
        assert any(c.B == 3 for c in of_d) and any(c.B == 1 for c in of_d)
        assert any(c.kind == "exact" for c in of_d)
    assert any(c.H < c.d for c in cs) and any(c.W < c.d for c in cs)                    # whole displacement rows / columns read only padding
    assert any(c.H < c.d and c.d == 4 for c in cs) and any(c.H == 1 and c.W == 2 for c in cs)
    assert {TH - 1, TH, TH + 1, 2 * TH + 3} <= {c.H for c in cs} and {TW - 1, TW, TW + 1, 2 * TW + 3} <= {c.W for c in cs}
    assert any(c.H > 2 * TH and c.W > 2 * TW for c in cs)                               # three tiles each way in one launch
    assert any(c.H > TH and c.d == 4 for c in cs) and any(c.W > TW and c.d == 4 for c in cs)      # a seam under the widest halo
    assert {1, 2, 3, CK - 1, CK, CK + 1, 32, 33, 192} <= {c.C for c in cs}
    assert any(c.C % CK and c.C > CK for c in cs) and any(c.C % CK == 0 and c.C > CK for c in cs) and any(c.C > 2 * CK and c.C % CK == 1 for c in cs)
    sl = [c for c in cs if c.slope != 1.0]
    assert {c.slope for c in cs} == {1.0, 0.1} and {c.d for c in sl} == {1, 2, 3, 4}
    assert any(c.H > TH and c.W > TW for c in sl) and any(c.C > CK for c in sl)
    for kind in ("nan", "inf", "huge"):
        assert {c.slope for c in cs if c.kind == kind} == {1.0, 0.1}
    assert any(c.kind == "exact" and c.H > TH and c.W > TW and c.d == 4 for c in cs)


def test_exact_case_is_exact_in_the_restatement():
    for c in (c for c in cc.CASES if c.kind == "exact"):
        d = cc.inputs(c)
        out, _ = cc.fwd_truth(c)
        x2z = np.pad(d["x2"].astype(np.float64), ((0, 0), (0, 0), (c.d, c.d), (c.d, c.d)))
        assert len(np.unique(d["x2"])) == d["x2"].size and d["x2"].max() < 2 ** 24 and c.C == 1 and c.slope == 1.0
        for i in range(c.D):
            for j in range(c.D):
                assert np.array_equal(out[:, i * c.D + j], x2z[:, 0, i:i + c.H, j:j + c.W])
        assert np.array_equal(out.astype(np.float32).astype(np.float64), out)


def test_non_finite_cases_do_what_they_promise():
    for c in (c for c in cc.CASES if c.kind in ("nan", "inf", "huge")):
        d = cc.inputs(c)
        out, mass = cc.fwd_truth(c)
        dx1, m1, dx2, m2 = cc.bwd_truth(c)
        B, C, H, W, dd, D = c.B, c.C, c.H, c.W, c.d, c.D
        if c.kind == "nan":
            (b0, c0, y0, x0), = np.argwhere(np.isnan(d["x2"]))
            want = np.zeros(out.shape, dtype=bool)                    # exactly the (i, j, y, x) whose tap is that pixel
            for i in range(D):
                for j in range(D):
                    y, x = y0 - i + dd, x0 - j + dd
                    if 0 <= y < H and 0 <= x < W:
                        want[b0, i * D + j, y, x] = True
            assert np.array_equal(np.isnan(out), want) and want.sum() > 10
            assert np.array_equal(np.isnan(dx1), np.broadcast_to(want.any(1)[:, None], dx1.shape) & (np.arange(C) == c0)[None, :, None, None])
            assert np.isfinite(dx2).all()
        elif c.kind == "inf":
            (b0, c0, y0, x0), = np.argwhere(np.isinf(d["x1"]))
            assert (y0, x0) in ((0, 0), (H - 1, W - 1))
            here = out[b0, :, y0, x0].reshape(D, D)
            outside = np.array([[not (0 <= y0 + i - dd < H and 0 <= x0 + j - dd < W) for j in range(D)] for i in range(D)])
            assert np.array_equal(np.isnan(here), outside) and outside.sum() > D and np.isinf(here[~outside]).all()
            rest = np.ones(out.shape, dtype=bool)
            rest[b0, :, y0, x0] = False
            assert np.isfinite(out[rest]).all() and np.isfinite(dx1).all()
            assert np.isinf(dx2[b0, c0]).sum() > 3 and np.isfinite(np.delete(dx2[b0], c0, axis=0)).all()
        else:
            big = np.isinf(out)
            assert big.sum() > 20 and not np.isnan(out).any() and (out[big] > 0).any() and (out[big] < 0).any()
            near = np.isfinite(out) & (np.abs(out) > 1e37)
            assert near.sum() > 20 and np.abs(out[np.isfinite(out)]).max() < 3.1e38 / C + 1
            for g in (dx1, dx2):                                       # the gradients stay inside float32's range, with room
                assert np.isfinite(g).all() and 1e35 < np.abs(g).max() < 1e38
            assert np.isfinite(m1).all() and m1.max() < 3e38 and m2.max() < 3e38


# ------------------------------------------------------------------------------------------------------------ host surface
def test_correlation_constructor_surface():
    m = rcf_amd.Correlation(4, 1, 2, kernel_size=1, stride1=1, stride2=1, corr_multiply=1)
    assert (m.max_displacement, m.output_dim, m.pad_size, m.slope) == (4, 9, 4, 1.0)
    m = rcf_amd.Correlation(max_displacement=2, pad_size=2, slope=0.1)
    assert (m.max_displacement, m.output_dim, m.pad_size, m.slope) == (2, 5, 2, 0.1)
    assert rcf_amd.Correlation().max_displacement == 4 and isinstance(m, torch.nn.Module) and not list(m.parameters())
    for bad in (0, 5, -1, 20):
        with pytest.raises(NotImplementedError):
            rcf_amd.Correlation(bad)
    x = torch.zeros(1, 2, 3, 4)
    with pytest.raises(_lib.RcfHipError):
        rcf_amd.Correlation()(x, x)
    with pytest.raises(_lib.RcfHipError):
        rcf_amd.ops.correlation_bwd(x, x, torch.zeros(1, 81, 3, 4))


def test_entries_refuse_before_touching_a_device():
    """sizes and ranges first (with every pointer NULL the status is the same), then pointers: nothing is launched -- there is no
    device here -- and the host buffer keeps its fill"""
    lib = _lib.load()
    buf = (ctypes.c_float * 64)(*([7.0] * 64))
    p = ctypes.cast(buf, ctypes.c_void_p)
    fwd, bwd = lib.rcf_correlation_fwd_f32, lib.rcf_correlation_bwd_f32
    bad_dims = [(0, 1, 2, 2, 4), (1, 0, 2, 2, 4), (1, 1, 0, 2, 4), (1, 1, 2, 0, 4), (-1, 1, 2, 2, 4), (1, 1, 2, 2, 0), (1, 1, 2, 2, 5),
                (1, 1, 2, 2, -4),
                (1, 1, 32768, 65536, 1),              # x1 itself has 2^31 elements
                (1, 1 << 20, 2048, 1, 1),             # x1: 2^20 channels of 2^11 pixels
                (1, 1, 5155, 5155, 4),                # x1 fits, the 81-plane tensor does not
                (2147483647, 2147483647, 2147483647, 2147483647, 4)]
    for B, C, H, W, d in bad_dims:
        for ptr in (p, None):
            assert fwd(ptr, ptr, ptr, B, C, H, W, d, 1.0, None) == -1, (B, C, H, W, d)
            assert bwd(ptr, ptr, ptr, ptr, ptr, ptr, B, C, H, W, d, 1.0, None) == -1, (B, C, H, W, d)
    for k in range(3):
        a = [p, p, p]
        a[k] = None
        assert fwd(*a, 1, 1, 2, 2, 4, 1.0, None) == -1
        assert bwd(*a, p, p, p, 1, 1, 2, 2, 4, 1.0, None) == -1
    assert bwd(p, p, p, p, None, None, 1, 1, 2, 2, 4, 1.0, None) == -1                   # both gradients NULL
    assert bwd(p, p, p, None, p, p, 1, 1, 2, 2, 4, 0.1, None) == -1                      # slope != 1 without out
    assert list(buf) == [7.0] * 64
