"""The resize and copy kernels of csrc/spatial.hip bit for bit against a recorded build.

tests/test_spatial_sweep_gpu.py holds the kernels to float64 within a rounding bound or a floor; a change that only moves code must
move NOTHING.  For every resize run of tests/spatial_cases.py (PARAMS_FWD, PARAMS_BWD, NCHW), every copy run of COPY_SHAPES x
COPY_PAIRS, COPY_BIG and the two frame-reversing batched copies (negative strides) this module takes the SHA-256 of the raw bytes
of the output -- of the whole FILL-ed buffer where the operand is a channel slice of one, so with its guard channels; with the NaN
fill a frame forward must leave and the prior values a beta = 1 backward adds to -- and demands equality with
tests/golden/spatial_bits.json: no tolerance, no skipped case.  A run whose storage is 16-bit is taken once per library (bf16 and
IEEE fp16), its inputs cast on the CPU.  The inputs come from spatial_cases' seeded CPU generators and from the seeds the sweep's
copy tests use, the kernels are gathers with a fixed order of terms, so the hashes depend on the kernels alone.

The fixture is recorded from a build of the commit the hashes are to be held to:
    python tests/test_spatial_bits_gpu.py --record [path]        (default path: tests/golden/spatial_bits.json)
which runs every group twice and refuses to write a fixture whose two runs differ."""
import hashlib
import json
import os
import sys
from ctypes import c_void_p

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import pytest
import torch

import rcf_amd  # noqa: F401  (package alias)
import spatial_cases as sc
from rcf_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
FIXTURE = os.path.join(HERE, "golden", "spatial_bits.json")
BF, FP = torch.bfloat16, torch.float16
HALF_TAG = {BF: "bf16lib", FP: "f16lib"}
REVERSED = [b for b in sc.BATCHED if b.name.endswith("_reversed")]           # batch strides below zero


def sha(t):
    """SHA-256 of a tensor's raw bytes (a view: of the elements it shows)"""
    b = t.detach().contiguous().cpu().reshape(-1)
    return hashlib.sha256(b.view(torch.uint8).numpy().tobytes()).hexdigest()


class Bufs:
    """device NHWC operands in the torch type `td`: contiguous, or channel slices [..., 8:8 + C] of FILL-ed buffers `pitch` wide"""

    def __init__(self, pitch, td):
        self.pitch, self.td = pitch, td

    def full(self, shape, fill):
        """(the operand, what to hash: the whole buffer)"""
        if not self.pitch:
            t = torch.full(shape, fill, dtype=self.td, device=DEV)
            return t, t
        big = torch.full(tuple(shape[:3]) + (self.pitch,), sc.FILL, dtype=self.td, device=DEV)
        v = big[..., sc.SLICE0:sc.SLICE0 + shape[3]]
        v.fill_(fill)
        return v, big

    def put(self, t64):
        v, big = self.full(tuple(t64.shape), 0.0)
        v.copy_(t64.to(self.td))
        return v, big


# --------------------------------------------------------------------------------------------------------------- groups
def resize_family(c, dt, pitch, half):
    """every forward (per frame) and backward (per frame and beta) run of one (case, storage, pitch), operands as in the sweep"""
    td = torch.float32 if dt == "f32" else half
    x64, dy64, old64 = sc.resize_inputs(c.name, dt)
    o = {}
    for frame in c.frames:
        B = Bufs(pitch, td)
        xg, _ = B.put(x64)
        out, whole = B.full((c.N, c.Ho, c.Wo, c.C), NAN)
        ops.resize_nhwc_fwd(xg, (c.Ho, c.Wo), c.align, out=out, frame=frame)
        o[f"fwd-frame{frame}"] = sha(whole)
        del xg, out, whole
        dyg, _ = B.put(dy64)
        if frame > 0:
            dyg[:, ~sc.frame_mask(c.Ho, c.Wo, frame).to(DEV)] = NAN          # off the frame the gradient must not be read
        for beta in c.betas:
            dx, whole = B.put(old64) if beta else B.full(tuple(old64.shape), NAN)
            ops.resize_nhwc_bwd(dyg, (c.Hi, c.Wi), c.align, out=dx, beta=beta, frame=frame)
            o[f"bwd-frame{frame}-beta{beta}"] = sha(whole)
    return o


def nchw_family(half):
    o = {}
    for name, planes, Hi, Wi, Ho, Wo, align in sc.NCHW:
        xg = sc.nchw_input(name, planes, Hi, Wi).to(DEV)
        out = torch.full(planes + (Ho, Wo), NAN, device=DEV)
        ops.call("rcf_resize_bilinear_nchw_f32", c_void_p(xg.data_ptr()), c_void_p(out.data_ptr()), xg.numel() // (Hi * Wi), Hi, Wi, Ho, Wo,
                 int(align), ops._stream())
        o[name] = sha(out)
    return o


def copy_family(sk, dk, half):
    """tests/test_spatial_sweep_gpu.py test_copy2d_bit_equal's runs: the same generator, the same order of draws"""
    sdt, ddt = (half if sk == "h16" else torch.float32), (half if dk == "h16" else torch.float32)
    g = torch.Generator().manual_seed(13)
    o = {}
    for rows, C, sp, dp in sc.COPY_SHAPES:
        for beta in (0, 1):
            sg = torch.randn(rows, sp, generator=g).to(sdt).to(DEV)
            dg = torch.randn(rows, dp, generator=g).to(ddt).to(DEV)
            ops.copy2d(sg, sp, dg, dp, rows, C, beta=beta)
            o[f"{rows}x{C}_p{sp}_p{dp}-beta{beta}"] = sha(dg)
    return o


def copy_big_family(half):
    rows, C = sc.COPY_BIG
    g = torch.Generator().manual_seed(14)
    sg, dg = torch.randn(rows, C, generator=g).to(half).to(DEV), torch.randn(rows, C, generator=g).to(half).to(DEV)
    ops.copy2d(sg, C, dg, C, rows, C, beta=1)
    return {"beta1": sha(dg)}


def batched_family(b, sixteen, half):
    td = half if sixteen else torch.float32
    g = torch.Generator().manual_seed(15)
    o = {}
    for beta in (0, 1):
        sg, dg = torch.randn(b.src_len, generator=g).to(td).to(DEV), torch.randn(b.dst_len, generator=g).to(td).to(DEV)
        ops.copy2d_batched(sg[b.src[0]:], b.src[1], b.src[2:], dg[b.dst[0]:], b.dst[1], b.dst[2:], b.rows, b.C, (b.n0, b.n1), beta=beta)
        o[f"beta{beta}"] = sha(dg)
    return o


def _groups():
    """id -> (function, args, the library's 16-bit type): every group is one test case"""
    G = {}

    def add(gid, fn, args, sixteen):
        for half in ((BF, FP) if sixteen else (BF,)):
            G[gid + (f"/{HALF_TAG[half]}" if sixteen else "")] = (fn, args, half)
    for c in sc.RESIZE:
        for dt, pitch in c.variants:
            add(f"resize/{c.name}-{dt}" + (f"_p{pitch}" if pitch else ""), resize_family, (c, dt, pitch), dt != "f32")
    add("resize_nchw", nchw_family, (), False)
    for sk, dk in sc.COPY_PAIRS:
        add(f"copy2d/{sk}-{dk}", copy_family, (sk, dk), "h16" in (sk, dk))
    add("copy2d_big", copy_big_family, (), True)
    for b in REVERSED:
        add(f"copy2d_batched/{b.name}-f32", batched_family, (b, False), False)
        add(f"copy2d_batched/{b.name}-h16", batched_family, (b, True), True)
    return G


GROUPS = _groups()


def compute(gid):
    fn, args, half = GROUPS[gid]
    with ops.half_storage(half):
        return fn(*args, half)


_fixture = []


def fixture():
    if not _fixture:
        with open(FIXTURE) as f:
            _fixture.append(json.load(f))
    return _fixture[0]


@pytest.mark.parametrize("gid", list(GROUPS))
def test_spatial_bits_match_recorded_build(gid):
    want = fixture()["groups"][gid]
    got = compute(gid)
    assert sorted(got) == sorted(want), "the outputs of this group are not the recorded ones"
    differ = [k for k in want if got[k] != want[k]]
    assert not differ, f"{gid}: outputs whose bytes differ from the recorded build: {differ}"


def test_spatial_bits_fixture_covers_every_run():
    assert sorted(fixture()["groups"]) == sorted(GROUPS)
    runs = {k.split("/")[1] + "-" + r for k, v in fixture()["groups"].items() if k.startswith("resize/") for r in v}
    for p in sc.PARAMS_FWD:
        c, dt, pitch, frame = p.values
        assert f"{c.name}-{dt}" + (f"_p{pitch}" if pitch else "") + f"-fwd-frame{frame}" in runs, p.id
    for p in sc.PARAMS_BWD:
        c, dt, pitch, frame, beta = p.values
        assert f"{c.name}-{dt}" + (f"_p{pitch}" if pitch else "") + f"-bwd-frame{frame}-beta{beta}" in runs, p.id


def record(path):
    groups = {}
    for gid in GROUPS:
        a, b = compute(gid), compute(gid)
        assert a == b, f"{gid}: two runs of the same build differ: {[k for k in a if a[k] != b[k]]}"
        groups[gid] = a
        print(f"{gid}: {len(a)} outputs", flush=True)
    torch.cuda.synchronize()
    with open(path, "w") as f:
        json.dump({"what": "SHA-256 of the raw bytes of every output, by group (tests/test_spatial_bits_gpu.py)", "groups": groups}, f,
                  indent=0, sort_keys=True)
        f.write("\n")
    print(f"recorded {sum(len(v) for v in groups.values())} hashes of {len(groups)} groups to {path}")


if __name__ == "__main__":
    if "--record" not in sys.argv:
        sys.exit("usage: python tests/test_spatial_bits_gpu.py --record [path]")
    rest = sys.argv[sys.argv.index("--record") + 1:]
    record(rest[0] if rest else FIXTURE)
