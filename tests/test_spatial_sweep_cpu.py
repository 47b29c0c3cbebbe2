"""Conditioning of the spatial sweep (tests/spatial_cases.py): the tables reach the dispatch branches, vector widths, row
geometries and grid-stride trips they name; the restatement agrees with torch's float64 F.interpolate / F.max_pool2d and their
autograd; and the restatement's own float32 run sits within a quarter of every resize bound.  Then a kernel that misses a bound
in tests/test_spatial_sweep_gpu.py is wrong, not unlucky.  A case that cannot meet this gets other inputs, never a looser limit."""
import pytest
import torch
import torch.nn.functional as F

import spatial_cases as sc


def test_resize_tables_reach_every_branch():
    """fwd_branch / bwd_branch restate the dispatchers of rcf_resize_bilinear_nhwc_{fwd,bwd}_mp (to choose inputs, never as a
    reference for a value)"""
    fwd, bwd = {}, {}
    for c, dt, p, fr in sc.resize_runs():
        fwd[c.name, dt, p, fr] = sc.fwd_branch(c, dt, p, fr)
        for b in c.betas:
            bwd[c.name, dt, p, fr, b] = sc.bwd_branch(c, dt, p, fr, b)
    by = sc.RESIZE_BY_NAME
    for k, v in fwd.items():
        print("resize sweep forward", k, v)
    for k, v in bwd.items():
        print("resize sweep backward", k, v)

    # 1. every dispatch branch
    assert {v[:2] for v in fwd.values()} >= {("2x", "whole"), ("2x", "frame"), ("rows", "whole"), ("rows", "frame"), ("rows", "general"),
                                            ("fallback", "whole"), ("fallback", "frame"), ("fallback", "general")}
    got = {(v[0], v[1], k[4]) for k, v in bwd.items()}
    assert got >= {("2x", "whole", 0), ("2x", "whole", 1), ("2x", "frame", 1), ("rows", "whole", 0), ("rows", "whole", 1),
                   ("rows", "frame", 0), ("rows", "frame", 1), ("rows", "general", 0), ("rows", "general", 1),
                   ("fallback", "whole", 0), ("fallback", "whole", 1), ("fallback", "frame", 0), ("fallback", "frame", 1)}
    assert ("2x", "frame", 0) not in got                                                  # the frame form of the 2x backward only accumulates
    tcs = {v[3] for k, v in bwd.items() if v[0] == "fallback" and v[1] == "frame" and k[4] == 1}
    assert {0, 5, 7} <= tcs                                                               # the input-frame walk, and a frame too thick for it
    assert all(v[3] == 0 for k, v in bwd.items() if k[4] == 0)

    # 2. the fallbacks: N * Ho > 65535 (N * Hi backward); the second trip of the 8192 x 256 loop; an exact 2x sent through by frame = -1
    c = by["fb_up"]
    assert c.N * c.Ho == 65536 and fwd["fb_up", "f32", 0, 0][0] == "fallback" and fwd["fb_up", "bf16", 0, 0] == ("fallback", "whole", 4)
    c = by["fb_up_c20"]
    assert fwd["fb_up_c20", "f32", 0, 0][0] == "fallback" and c.N * c.Ho * c.Wo * (c.C // 4) > sc.TRIP
    c = by["fb_down_c20"]
    assert bwd["fb_down_c20", "f32", 0, 0, 1][0] == "fallback" and c.N * c.Hi * c.Wi * (c.C // 4) > sc.TRIP
    c = by["fb_general_2x"]
    assert fwd["fb_general_2x", "f32", 0, -1] == ("fallback", "general", 4) and c.N % 2 == 0
    assert sc.fwd_branch(c, "f32", 0, 0)[0] == "2x" and sc.fwd_branch(dataclass_half(c), "f32", 0, 0)[0] == "2x"

    # 3. C in {4, 20, 24, 64} on exact cases; bf16 on both vector widths, the narrow one by C % 8 == 4 and by a pitch; fp16 once
    ex = {k: v for k, v in fwd.items() if by[k[0]].exact}
    assert {by[k[0]].C for k in ex if k[1] == "f32"} >= {4, 20, 24, 64}
    assert {by[k[0]].C for k, v in ex.items() if k[1] == "bf16" and v[2] == 8} >= {24, 64}
    assert {by[k[0]].C for k, v in ex.items() if k[1] == "bf16" and v[2] == 4 and by[k[0]].C % 8 == 4} >= {4, 20}
    assert any(k[1] == "bf16" and v[2] == 4 and by[k[0]].C % 8 == 0 and k[2] % 8 == 4 for k, v in ex.items())
    assert any(k[1] == "f16" for k in ex)
    for kernel in ("2x", "rows"):
        assert {v[2] for k, v in ex.items() if v[0] == kernel and k[1] == "bf16"} == {4, 8}

    # 4. the row geometry: threads per row (Wo C / V on the rows kernel, Wi C / V on the 2x kernel) below, at and above 256 with a tail
    for kernel, width in (("rows", lambda c: c.Wo), ("2x", lambda c: c.Wi)):
        per_row = {width(by[k[0]]) * by[k[0]].C // v[2] for k, v in ex.items() if v[0] == kernel and v[1] == "whole"}
        assert any(n < 256 for n in per_row) and 256 in per_row and any(n > 256 and n % 256 for n in per_row), (kernel, per_row)

    # 5. pitched operands: [..., 8:8 + C] of a wider buffer
    assert all(p == 0 or p >= sc.SLICE0 + by[n].C for n, dt, p, fr in fwd)
    assert {(dt, p) for n, dt, p, fr in fwd if p} >= {("f32", 40), ("bf16", 40), ("bf16", 36), ("f16", 40)}

    # 6. axis mixes, degenerate sizes, the backward's fast and general candidate loops, frames
    assert any(c.Ho > c.Hi and c.Wo < c.Wi for c in sc.RESIZE) and any(c.Ho < c.Hi and c.Wo > c.Wi for c in sc.RESIZE)
    assert fwd["row_2x", "f32", 0, 0][:2] == ("rows", "whole") and fwd["col_2x", "f32", 0, 0][:2] == ("rows", "whole")
    assert bwd["row_2x", "f32", 0, 0, 0][:2] == ("rows", "whole") and bwd["col_2x", "f32", 0, 0, 1][:2] == ("rows", "whole")
    assert by["align_one_row"].align and by["align_one_row"].Ho == 1 and by["align_one_col"].align and by["align_one_col"].Wo == 1
    assert any(c.Hi > c.Ho and c.Hi % c.Ho and c.exact for c in sc.RESIZE) and any(c.Hi > c.Ho and c.Hi % c.Ho and not c.exact for c in sc.RESIZE)
    share = {c.name: sc.bwd_fast_share(c) for c in sc.RESIZE}
    print("share of input pixels on the MAXC fast path:", share)
    assert share["shrink_1p5"] == 1.0 and share["fb_down"] == 1.0 and share["down_inexact"] == 1.0      # shrinking: the fast path
    assert share["up4_c64"] == 0.0 and share["up_inexact"] == 0.0                                        # 3x and up: the general loop
    assert 0.0 < share["x2_general"] < 1.0                                                               # plain 2x: fast only at the borders
    c = by["x2_frame"]
    assert set(c.frames) >= {1, 2}
    assert fwd["x2_frame", "f32", 0, 14][:2] == ("2x", "frame") and fwd["x2_frame", "f32", 0, 15][:2] == ("rows", "frame")
    assert bwd["x2_frame", "f32", 0, 7, 1][:2] == ("2x", "frame") and bwd["x2_frame", "f32", 0, 8, 1][:2] == ("rows", "frame")
    assert all(2 * fr < min(c.Ho, c.Wo) for c in sc.RESIZE for fr in c.frames)
    assert by["x2_frame_odd"].Hi % 2 == 1 and by["x2_frame_odd"].Wi % 2 == 1 and bwd["x2_frame_odd", "f32", 0, 5, 1][:2] == ("2x", "frame")

    # the table stays small: no resize run holds more than 50 MB (input + output); the largest is the forward second trip
    worst = max(sc.RESIZE, key=lambda c: c.bytes)
    assert worst.name == "fb_up_c20" and worst.bytes == 4 * 8192 * 20 * (9 + 64) < 50e6


def dataclass_half(c):
    import dataclasses
    return dataclasses.replace(c, N=c.N // 2)


def test_exact_cases_have_exact_positions():
    """the float32 scale and source positions of every exact case equal the rational ones; the inexact cases are really inexact
    somewhere (or they would deserve the tight bound)"""
    for c in sc.RESIZE:
        e = sc.positions_exact(c.Ho, c.Hi, c.align) and sc.positions_exact(c.Wo, c.Wi, c.align)
        assert e == c.exact, c.name
    for name, planes, Hi, Wi, Ho, Wo, align in sc.NCHW:
        assert (sc.positions_exact(Ho, Hi, align) and sc.positions_exact(Wo, Wi, align)) == (name != "davis")
    assert {c.name for c in sc.RESIZE if not c.exact} == {"up_inexact", "down_inexact", "mix_inexact", "big_inexact"}


def test_other_tables_reach_their_limits():
    assert sc.POOL_HW == [(1, 1), (1, 9), (8, 1), (7, 10), (15, 22)]
    N, H, W, C, dt = sc.POOL_BIG_BWD
    assert N * H * W * (C // 4) > sc.TRIP and dt == "f32"
    N, H, W, C, dt = sc.POOL_BIG_FWD
    assert N * sc.pool_out(H) * sc.pool_out(W) * (C // 4) > sc.TRIP and dt == "bf16"
    assert 50e6 < N * H * W * C * 2 < 68e6                                               # the one case over 50 MB: 67.6 MB
    assert {(c, p) for _, c, _, _, p in sc.LAYOUT} == {(1, 4), (3, 4), (3, 8), (5, 8)}
    N, C, H, W, Cpad = sc.LAYOUT_BIG_TO
    assert N * H * W > sc.TRIP and 4 * N * H * W * (C + Cpad) < 50e6
    N, C, H, W, pitch = sc.LAYOUT_BIG_BACK
    assert N * C * H * W > sc.TRIP and pitch > C and 4 * N * H * W * (C + pitch) < 50e6
    assert any(rows == 1 for rows, *_ in sc.COPY_SHAPES) and any(sp > C and dp > C for _, C, sp, dp in sc.COPY_SHAPES)
    rows, C = sc.COPY_BIG
    assert rows * (C // 4) > sc.TRIP and 2 * 2 * rows * C < 50e6
    b = next(b for b in sc.BATCHED if b.name == "cap_4097")
    assert b.n0 * b.n1 == 4097 and 4096 // (b.n0 * b.n1) == 0 and b.rows * (b.C // 4) > 256 and 4 * (b.src_len + b.dst_len) < 50e6
    assert any(b.src[3] < 0 for b in sc.BATCHED) and any(b.dst[3] < 0 for b in sc.BATCHED) and all((b.n0, b.n1) == (2, 3) for b in sc.BATCHED[:4])
    N, H, W, C = sc.SPLIT_SHAPE
    assert N == 2
    touch = lambda r: (r[0] == 0, r[1] == 0, r[0] + r[2] == H, r[1] + r[3] == W)
    assert [any(touch(r)[k] for r in sc.SPLIT_RECTS) for k in range(4)] == [True] * 4
    assert (3, 4, 1, 1) in sc.SPLIT_RECTS and (0, 0, H, W) in sc.SPLIT_RECTS and any(not any(touch(r)) for r in sc.SPLIT_RECTS)
    N, H, W, C, rect = sc.SPLIT_BIG
    assert N * H * W * (C // 4) > sc.TRIP and N == 2 and 2 * 2 * N * H * W * C < 50e6


# ------------------------------------------------------------------------------------------------------------------ resize
def torch_resize(x, Ho, Wo, align):
    """float64 F.interpolate of an NHWC tensor, and its autograd"""
    xt = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    y = F.interpolate(xt, size=(Ho, Wo), mode="bilinear", align_corners=align)
    return xt, y


@pytest.mark.parametrize("c", [pytest.param(c, id=c.name) for c in sc.RESIZE])
def test_resize_restatement_vs_torch_and_its_float32_run(c):
    dt = c.variants[0][0]
    x, dy, old = sc.resize_inputs(c.name, dt)
    ref, mass = sc.resize_fwd_truth(c.name, dt)
    xt, y = torch_resize(x, c.Ho, c.Wo, c.align)
    yt = y.detach().permute(0, 2, 3, 1)
    r32, _ = sc.resize_fwd_ref(x, c.Ho, c.Wo, c.align, torch.float32)
    if c.exact:
        e_t = sc.elem_margin(ref, yt, 1e-12 * mass)
    else:
        e_t = sc.image_margin(ref, yt, 0.25 * sc.FLOOR_F32)
    e_32 = sc.resize_margins(c, "f32", r32, ref, mass)
    print(f"resize sweep {c.name}: forward restatement vs torch float64 {e_t:.3f} of its limit, float32 run {e_32:.3f} of the bound")
    assert e_t <= 1.0 and e_32 <= 0.25
    for frame in c.frames:
        fr = max(frame, 0)
        dx, bmass, terms = sc.resize_bwd_truth(c.name, dt, frame)
        M = sc.frame_mask(c.Ho, c.Wo, fr)
        g = torch.where(M[None, :, :, None], dy, torch.zeros(()).double()).permute(0, 3, 1, 2)
        gx, = torch.autograd.grad(y, xt, g, retain_graph=True)
        gx = gx.permute(0, 2, 3, 1)
        d32, _, _ = sc.resize_bwd_ref(dy, c.Hi, c.Wi, c.align, fr, torch.float32)
        if c.exact:
            e_t = sc.elem_margin(dx, gx, 1e-12 * bmass)
        else:
            e_t = sc.image_margin(dx, gx, 0.25 * sc.FLOOR_F32)
        e_32 = sc.resize_margins(c, "f32", d32, dx, bmass, terms)
        # the mass accounts for every term: it vanishes exactly where no term arrives
        assert bool(((terms != 0)[None, :, :, None] >= (bmass != 0)).all())
        print(f"resize sweep {c.name} frame {frame}: backward restatement vs torch autograd {e_t:.3f} of its limit, float32 run "
              f"{e_32:.3f} of the bound, terms up to {int(terms.max())}")
        assert e_t <= 1.0 and e_32 <= 0.25


@pytest.mark.parametrize("name,planes,Hi,Wi,Ho,Wo,align", sc.NCHW, ids=[n[0] for n in sc.NCHW])
def test_nchw_resize_restatement_vs_torch(name, planes, Hi, Wi, Ho, Wo, align):
    x = sc.nchw_input(name, planes, Hi, Wi).double().reshape(-1, Hi, Wi, 1)
    ref, mass = sc.resize_fwd_ref(x, Ho, Wo, align)
    yt = F.interpolate(x.permute(0, 3, 1, 2), size=(Ho, Wo), mode="bilinear", align_corners=align).permute(0, 2, 3, 1)
    r32, _ = sc.resize_fwd_ref(x, Ho, Wo, align, torch.float32)
    if name != "davis":
        e_t, e_32 = sc.elem_margin(ref, yt, 1e-12 * mass), sc.elem_margin(r32, ref, sc.fwd_bound(mass, ref, "f32"))
    else:
        e_t, e_32 = sc.image_margin(ref, yt, 0.25 * sc.FLOOR_F32), sc.image_margin(r32, ref, sc.FLOOR_F32)
    assert e_t <= 1.0 and e_32 <= 0.25


# ---------------------------------------------------------------------------------------------------------------- max-pool
@pytest.mark.parametrize("kind", sc.POOL_KINDS)
@pytest.mark.parametrize("H,W", sc.POOL_HW)
def test_maxpool_restatement_vs_torch(H, W, kind):
    x = sc.pool_input(H, W, kind, "f32")
    y, code = sc.maxpool_ref(x)
    xt = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    yt, it = F.max_pool2d(xt, 3, 2, 1, return_indices=True)
    assert torch.equal(torch.nan_to_num(y, nan=12345.0), torch.nan_to_num(yt.detach().permute(0, 2, 3, 1), nan=12345.0))
    assert torch.equal(sc.pool_flat_index(code, H, W), it.permute(0, 2, 3, 1))
    if kind == "special":
        assert bool(torch.isnan(y).any()) and bool((y == float("inf")).any()) and bool((y == -float("inf")).any())
        assert bool((code[:, 0, 0, 0] == 4).all())               # an all--inf window keeps its first valid tap: (r, s) = (1, 1) in the corner
    if kind == "relu_ties":
        assert float((y == 0).double().mean()) > 0.002 or H * W == 1
    g = torch.Generator().manual_seed(H + W)
    dy = torch.randn(y.shape, generator=g).double()
    dx, mass, terms = sc.maxpool_bwd_ref(dy, code, H, W)
    gx, = torch.autograd.grad(yt, xt, dy.permute(0, 3, 1, 2))
    assert torch.allclose(dx, gx.permute(0, 2, 3, 1), rtol=0, atol=1e-12)
    assert int(terms.sum()) == dy.numel() and int(terms.max()) <= 4
    # the float32 run: its additions are the very additions the bound counts, so it may use all of it (not a quarter)
    d32, _, _ = sc.maxpool_bwd_ref(dy.float(), code, H, W, torch.float32)
    assert sc.elem_margin(d32, dx, sc.pool_bwd_bound(mass, terms, dx, "f32")) <= 1.0


# ---------------------------------------------------------------------------------------------- layout, copies, rectangle
def test_plain_indexing_references():
    g = torch.Generator().manual_seed(5)
    # the frame-pair gather is unflatten(0, (B, I)).flatten of the frames side by side on channels; the scatter is its inverse
    B, I, H, W, C = 2, 3, 5, 7, 8
    x = torch.randn(B * I, H, W, C, generator=g)
    for b in sc.BATCHED[:4]:
        order = [0, 1, 2] if "reversed" not in b.name else [2, 1, 0]
        pairs = x.reshape(B, I, H, W, C)[:, order].permute(0, 2, 3, 1, 4).reshape(B, H, W, I * C)
        if b.name.startswith("gather"):
            out = sc.batched_ref(x.reshape(-1), torch.zeros(b.dst_len), b, 0, torch.float32)
            assert torch.equal(out.reshape(B, H, W, I * C), pairs)
        else:
            out = sc.batched_ref(pairs.reshape(-1), torch.zeros(b.dst_len), b, 0, torch.float32)
            assert torch.equal(out.reshape(B * I, H, W, C), x)
    x = torch.randn(*sc.SPLIT_SHAPE, generator=g)
    for rect in sc.SPLIT_RECTS:
        ins, outs = sc.split_rect_ref(x, rect)
        assert torch.equal(ins + outs, x) and int((ins != 0).sum()) == x.shape[0] * rect[2] * rect[3] * x.shape[3]
    x = torch.randn(2, 3, 5, 7, generator=g)
    y = sc.nchw_to_nhwc_ref(x, 8)
    assert torch.equal(sc.nhwc_to_nchw_ref(y, 3), x) and not y[..., 3:].any()
    # half an ulp of the storage types
    r = torch.tensor([1.0, 1.5, 2.0, 3.0e-6, 0.0]).double()
    assert sc.half_ulp(r, "bf16")[:3].tolist() == [2.0 ** -8, 2.0 ** -8, 2.0 ** -7]
    assert sc.half_ulp(r, "f16")[:3].tolist() == [2.0 ** -11, 2.0 ** -11, 2.0 ** -10] and float(sc.half_ulp(r, "f16")[3]) == 2.0 ** -25
    assert not sc.half_ulp(r, "f32").any()
