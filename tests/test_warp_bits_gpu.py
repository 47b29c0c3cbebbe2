"""The flow family (csrc/warp.hip, the photometric kernels of csrc/unflow.hip) bit for bit against a recorded build.

tests/test_warp_sweep_gpu.py and tests/test_unflow_gpu.py hold the kernels to float64 within rounding bounds; a change that only
moves code must move NOTHING.  Through the public entry points alone (ops.call / ops.*), outputs allocated as NaN, this module takes

  the SHA-256 of the raw bytes, no tolerance, no skipped case, of
    * rcf_flow_warp_f32 in its default form and with RCF_WARP_PER_PIXEL, for every case of warp_cases.CASES x its pads;
    * the dflow of rcf_flow_warp_bwd_f32, with and without dx, for the same runs;
    * rcf_occu_mask_bidirection_f32 on warp_cases.MASK_CASES;
    * warp_cases.BIG_TILE forward (the second trip of the tile walk);
    * the five stats of rcf_unflow_photo_fwd_f32 and the dflow of rcf_unflow_photo_bwd_f32 for every case of unflow_cases.CASES
      (fixed-order sums: tests/test_unflow_gpu.py already demands that they repeat their bits);

  the VALUES, because fp64 atomics across workgroups arrive in no fixed order, of
    * the two sums of rcf_warp_l1_residual_f32 over CASES x pads x {masked, no mask} x {default, per-pixel} and warp_cases.L1_MANY:
      the mask sum equal, the L1 sum within 1e-12 relative (the tolerance test_fused_l1_vs_float64 puts between the two forms);
    * the float of rcf_photometric_loss_f32 on warp_cases.PHOTO_CASES: the recorded float32 or its neighbour (another order of
      the fp64 additions moves the double by ~1e-16 n, which can carry the float32 rounding across one boundary at most);
      zero_mask: non-finite in both.

Not here, because their bits depend on the arrival order of float32 atomics, which no build fixes (the sweep is their check): dx,
the splat count, the backward occlusion mask.

The fixture is recorded from a build of the commit the values are to be held to:
    python tests/test_warp_bits_gpu.py --record [path]        (default path: tests/golden/warp_bits.json)
which runs every group twice and refuses to write a fixture whose two runs do not match each other by the rules above."""
import hashlib
import json
import math
import os
import sys
from ctypes import c_void_p

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np
import pytest
import torch

import rcf_amd  # noqa: F401  (package alias)
import unflow_cases as uc
import warp_cases as wc
from rcf_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
FIXTURE = os.path.join(HERE, "golden", "warp_bits.json")
PP = _lib.WARP_PER_PIXEL
PAD = {"border": 0, "zeros": 1}
L1_RTOL = 1e-12


def sha(t):
    b = t.detach().contiguous().cpu().reshape(-1)
    return hashlib.sha256(b.view(torch.uint8).numpy().tobytes()).hexdigest()


def P(t):
    return None if t is None else c_void_p(t.data_ptr())


def G(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def warp(x, fl, mode):
    B, C, H, W = x.shape
    out = torch.full_like(x, NAN)
    ops.call("rcf_flow_warp_f32", P(x), P(fl), P(out), B, C, H, W, mode, ops._stream())
    return out


def dflow_of(x, fl, dout, mode, want_dx):
    B, C, H, W = x.shape
    dx = torch.zeros_like(x) if want_dx else None                # the kernel accumulates into it
    dfl = torch.full_like(fl, NAN)
    ops.call("rcf_flow_warp_bwd_f32", P(x), P(fl), P(dout), P(dx), P(dfl), B, C, H, W, mode, ops._stream())
    return dfl


def l1(im1, im2, fl, occ, mode):
    B, C, H, W = im1.shape
    out = torch.full((2,), NAN, dtype=torch.float64, device=DEV)
    ops.call("rcf_warp_l1_residual_f32", P(im1), P(im2), P(fl), P(occ), P(out), B, C, H, W, mode, ops._stream())
    s, so = (float(v) for v in out.cpu())
    return {"l1": s, "mask": so}


# --------------------------------------------------------------------------------------------------------------- groups
def warp_family(c):
    """every run of one case of warp_cases.CASES, operands as in the sweep"""
    d = wc.inputs(c)
    x, y, fl, dout, occ = (G(d[k]) for k in ("x", "y", "f12", "dout", "occ"))
    o = {}
    for pad in c.pads:
        o[f"fwd-{pad}"] = sha(warp(x, fl, PAD[pad]))
        o[f"fwd-{pad}-per_pixel"] = sha(warp(x, fl, PAD[pad] | PP))
        o[f"dflow-{pad}"] = sha(dflow_of(x, fl, dout, PAD[pad], True))
        o[f"dflow-{pad}-no_dx"] = sha(dflow_of(x, fl, dout, PAD[pad], False))
        for m, tag in ((occ, "masked"), (None, "no_mask")):
            o[f"l1-{pad}-{tag}"] = l1(y, x, fl, m, PAD[pad])
            o[f"l1-{pad}-{tag}-per_pixel"] = l1(y, x, fl, m, PAD[pad] | PP)
    if c in wc.MASK_CASES:
        m12, f21 = G(d["m12"]), G(d["f21"])
        occ_out = torch.full((c.B, 1, c.H, c.W), NAN, device=DEV)
        ops.call("rcf_occu_mask_bidirection_f32", P(m12), P(f21), P(occ_out), 0.01, 0.5, c.B, c.H, c.W, ops._stream())
        o["occ_bidirection"] = sha(occ_out)
    return o


def big_tile_family():
    """tests/test_warp_sweep_gpu.py test_second_trip_tile_forward's operands"""
    B, C, H, W = wc.BIG_TILE
    g = torch.Generator().manual_seed(26209)
    x = torch.rand(B, C, H, W, generator=g)
    fl = torch.randn(B, 2, H, W, generator=g) * 2.5
    return {"fwd-border": sha(warp(x.to(DEV), fl.to(DEV), 0))}


def l1_many_family():
    """tests/test_warp_sweep_gpu.py test_second_trip_fused_l1_per_pixel_kernel's operands"""
    B, H, W = wc.L1_MANY
    g = torch.Generator().manual_seed(300)
    o = {}
    for C, pad in ((2, "border"), (3, "zeros")):
        x, y = torch.rand(B, C, H, W, generator=g).numpy(), torch.rand(B, C, H, W, generator=g).numpy()
        fl = (torch.randn(B, 2, H, W, generator=g) * 0.7).numpy()
        occ = (torch.rand(B, 1, H, W, generator=g) > 0.3).float().numpy()
        o[f"l1-c{C}-{pad}"] = l1(G(y), G(x), G(fl), G(occ), PAD[pad])
    return o


def photometric_family():
    o = {}
    for name, B, C, H, W, *_ in wc.PHOTO_CASES:
        im, rec, occ, w1, ws = wc.photo_inputs(name)
        im_d, rec_d, occ_d = G(im), G(rec), G(occ)                # named: a temporary's block would be freed before the launch
        out = torch.full((1,), NAN, device=DEV)
        scratch = torch.full((4,), NAN, dtype=torch.float64, device=DEV)
        ops.call("rcf_photometric_loss_f32", P(im_d), P(rec_d), P(occ_d), w1, ws, P(out), P(scratch), B, C, H, W, ops._stream())
        o[name] = {"f32": float(out[0])}
    return o


def unflow_family(c):
    """the flow read in place as a channel slice of a [B, 4, h, w] tensor, as in tests/test_unflow_gpu.py"""
    d = uc.inputs(c)
    im, other, occ = G(d["im"]), G(d["other"]), G(d["occ"])
    wide = torch.full((c.B, 4, c.h, c.w), NAN, device=DEV)
    wide[:, 2:] = G(d["flow"])
    flow = wide[:, 2:]
    _, stats = ops.unflow_photo(im, other, flow, occ, c.md, *c.weights)
    dflow = torch.full((c.B, 2, c.h, c.w), NAN, device=DEV)
    one = torch.ones(1, device=DEV)
    ops.call("rcf_unflow_photo_bwd_f32", P(im), P(other), P(flow), flow.stride(0), P(occ), occ.shape[2], occ.shape[3], c.md,
             *[float(v) for v in c.weights], P(one), P(stats), P(dflow), c.B, c.h, c.w, ops._stream())
    return {"stats": sha(stats), "dflow": sha(dflow)}


def _groups():
    """id -> (function, args): every group is one test case"""
    G_ = {f"warp/{c.name}": (warp_family, (c,)) for c in wc.CASES}
    G_["warp_big_tile"] = (big_tile_family, ())
    G_["l1_many"] = (l1_many_family, ())
    G_["photometric"] = (photometric_family, ())
    G_.update({f"unflow/{c.name}": (unflow_family, (c,)) for c in uc.CASES})
    return G_


GROUPS = _groups()


def compute(gid):
    fn, args = GROUPS[gid]
    return fn(*args)


# -------------------------------------------------------------------------------------------------------------- the rules
def matches(got, want):
    """a hash: equal.  The fused L1's sums: the mask sum equal, the L1 sum within 1e-12 relative.  The photometric float: the
    recorded float32 or one of its two neighbours; non-finite where the recorded one is"""
    if isinstance(want, str):
        return got == want
    if "l1" in want:
        return got["mask"] == want["mask"] and abs(got["l1"] - want["l1"]) <= L1_RTOL * abs(want["l1"])
    g, w = np.float32(got["f32"]), np.float32(want["f32"])
    if not math.isfinite(w) or not math.isfinite(g):
        return not math.isfinite(w) and not math.isfinite(g)
    return g in (w, np.nextafter(w, np.float32(np.inf)), np.nextafter(w, np.float32(-np.inf)))


def differing(got, want):
    return [k for k in want if not matches(got[k], want[k])]


_fixture = []


def fixture():
    if not _fixture:
        with open(FIXTURE) as f:
            _fixture.append(json.load(f))
    return _fixture[0]


@pytest.mark.parametrize("gid", list(GROUPS))
def test_warp_bits_match_recorded_build(gid):
    want = fixture()["groups"][gid]
    got = compute(gid)
    for k in sorted(got):
        if not isinstance(got[k], str):
            print(f"{gid} {k}: {got[k]} recorded {want.get(k)}")
    assert sorted(got) == sorted(want), "the outputs of this group are not the recorded ones"
    differ = differing(got, want)
    assert not differ, f"{gid}: outputs that differ from the recorded build: {differ}"


def test_warp_bits_fixture_covers_every_run():
    groups = fixture()["groups"]
    assert sorted(groups) == sorted(GROUPS)
    for c in wc.CASES:
        runs = groups[f"warp/{c.name}"]
        for pad in c.pads:
            for k in ("fwd-{}", "fwd-{}-per_pixel", "dflow-{}", "dflow-{}-no_dx", "l1-{}-masked", "l1-{}-masked-per_pixel", "l1-{}-no_mask",
                      "l1-{}-no_mask-per_pixel"):
                assert k.format(pad) in runs, (c.name, k.format(pad))
        assert ("occ_bidirection" in runs) == (c in wc.MASK_CASES), c.name
    assert sorted(groups["photometric"]) == sorted(p[0] for p in wc.PHOTO_CASES)
    # a recording that did not reach the kernel's inputs shows as constants: where recon differs from im under a mask that is not
    # all zeros the loss is a positive number, and the fused L1 sums of a case are not all alike
    for name, _, _, _, _, kind, same, _, _ in wc.PHOTO_CASES:
        v = groups["photometric"][name]["f32"]
        if kind == "zeros":
            assert not math.isfinite(v), name
        elif not same:
            assert math.isfinite(v) and v > 0, (name, v)
    for c in wc.CASES:
        sums = {e["l1"] for k, e in groups[f"warp/{c.name}"].items() if k.startswith("l1-border-")}
        assert len(sums) > 1 and all(math.isfinite(s) and s > 0 for s in sums), c.name
    assert all(sorted(groups[f"unflow/{c.name}"]) == ["dflow", "stats"] for c in uc.CASES)


def record(path):
    groups = {}
    for gid in GROUPS:
        a, b = compute(gid), compute(gid)
        assert sorted(a) == sorted(b) and not differing(a, b), f"{gid}: two runs of the same build differ: {differing(a, b)}"
        groups[gid] = a
        print(f"{gid}: {len(a)} outputs", flush=True)
    torch.cuda.synchronize()
    with open(path, "w") as f:
        json.dump({"what": "by group: SHA-256 of the raw bytes of an output; the two fp64 sums of the fused L1; the photometric float32 "
                           "(tests/test_warp_bits_gpu.py)", "groups": groups}, f, indent=0, sort_keys=True)
        f.write("\n")
    n = sum(len(v) for v in groups.values())
    h = sum(isinstance(e, str) for v in groups.values() for e in v.values())
    print(f"recorded {h} hashes and {n - h} values of {len(groups)} groups to {path}")


if __name__ == "__main__":
    if "--record" not in sys.argv:
        sys.exit("usage: python tests/test_warp_bits_gpu.py --record [path]")
    rest = sys.argv[sys.argv.index("--record") + 1:]
    record(rest[0] if rest else FIXTURE)
