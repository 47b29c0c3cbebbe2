"""GPU: the semantic-constraint refinement -- rcf_affinity_pack_f32 (the thresholded affinity as a bit matrix),
rcf_ncut_refine_packed_f32 (all Adam steps of a batch of frames on it), rcf_mask_merge_u8 (the CRF / NCut-CRF merge),
NCutHead.forward_batch, offline.double_crf_merge_u8 and the driver rcf_amd.semantic.main.

Bars.  Bits, popcounts, merged bytes and counts: exact.  Refined masks against the existing per-frame path (ncut.ncut_refine)
and against the reference's refined mask of tests/golden/vit_small8.npz: 1e-3 per cell, the bar tests/test_vit_gpu.py applies
to the same quantity (Adam's first steps are sign-like, lr 0.45 and the clamp saturate the mask).  The NCut before the first
step against ncut.soft_ncut_value: 1e-5 relative (that path stores its value in fp32).  Batch size, position and repetition:
bit-identical."""
import os
import shutil

import numpy as np
import pytest
import torch

import rcf_amd
from rcf_amd import _lib, crf, maa, ncut, offline, semantic, synth, vit
from rcf_amd.ops import _p, _stream

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAU, EPS = 0.2, 1e-5
KW = dict(steps=10, learning_rate=0.45, weight_decay=1e-6)
TOL = 1e-3


# ---- pack ----------------------------------------------------------------------------------------------------------------
def _unpack(bits):
    """int32 [..., W] -> bool [..., 32 W]: bit j of a row = bit j % 32 of word j / 32"""
    b = np.ascontiguousarray(bits.cpu().numpy())
    return np.unpackbits(b.view(np.uint8), axis=-1, bitorder="little").astype(bool)


@pytest.mark.parametrize("n", [33, 96, 101])
def test_pack_bits_and_popcounts_are_exact(n):
    g = np.random.default_rng(n)
    pitch = n + 7                                                              # a padded pitch, not a multiple of 4
    G = g.uniform(-1, 1, (3, n, pitch)).astype(np.float32)
    G[:, :, n:] = 1.0                                                          # the padding must not be read as columns
    hit = g.random((3, n, n)) < 0.1
    G[:, :, :n][hit] = np.float32(TAU)                                         # exactly tau: NOT above it
    want = G[:, :, :n] > np.float32(TAU)
    assert not np.array_equal(want, want.transpose(0, 2, 1)) and (G[:, :, :n] == np.float32(TAU)).sum() > n
    Gd = torch.from_numpy(G).to(DEV)
    before = Gd.clone()
    bits, deg = ncut.affinity_pack(Gd, n, TAU)
    assert torch.equal(Gd, before)                                             # read only
    W = ncut.pack_words(n)
    assert W == _lib.load().rcf_affinity_pack_words(n) and tuple(bits.shape) == (3, n, W) and W * 32 >= n
    got = _unpack(bits)
    assert np.array_equal(got[..., :n], want)
    assert not got[..., n:].any()                                              # padding bits are zero
    assert np.array_equal(deg.cpu().numpy(), want.sum(-1).astype(np.int32))
    for f in range(3):                                                         # frames = 3 == three frames = 1 calls
        b1, d1 = ncut.affinity_pack(Gd[f], n, TAU)
        assert torch.equal(b1[0], bits[f]) and torch.equal(d1[0], deg[f])


# ---- refine --------------------------------------------------------------------------------------------------------------
def _clustered(seed, hf, wf, dim=384):
    """the recipe of tests/golden/make_golden_vit.py: 3 clusters + noise, a [CLS] row, a 0.1 / 0.9 random mask"""
    g = np.random.Generator(np.random.PCG64(seed))
    n = hf * wf
    centers = g.standard_normal((3, dim))
    lab = (np.arange(n) * 3 // n + (g.random(n) > 0.85)) % 3
    fe = centers[lab] + 1.2 * g.standard_normal((n, dim))
    feats = np.concatenate([g.standard_normal((1, dim)), fe])[None].astype(np.float32)
    mask = (g.random((hf, wf)) > 0.5).astype(np.float32) * 0.8 + 0.1
    return feats, mask


@pytest.fixture(scope="module")
def cases(golden_dir):
    """name -> (feats [3,T,C], masks [3,h,w], per-frame refined masks and values of the EXISTING path), computed once"""
    fx = np.load(os.path.join(golden_dir, "vit_small8.npz"))
    out = {}
    for name, (hf, wf) in (("n96", (8, 12)), ("n101", (101, 1))):
        frames = [_clustered(1000 * hf + s, hf, wf) for s in range(3)]
        if name == "n96":
            frames[0] = (fx["ncut_feats"], fx["mask"])
        feats = torch.from_numpy(np.concatenate([f for f, _ in frames])).to(DEV)
        masks = torch.from_numpy(np.stack([m for _, m in frames])).to(DEV)
        old = torch.stack([ncut.ncut_refine(feats[b:b + 1], masks[b], tau=TAU, eps=EPS, **KW) for b in range(3)])
        val = [float(ncut.soft_ncut_value(feats[b:b + 1], masks[b], TAU, EPS)) for b in range(3)]
        out[name] = (feats, masks, old.cpu().numpy(), val)
    out["golden_refined"] = fx["refined"]
    return out


@pytest.mark.parametrize("name", ["n96", "n101"])
def test_refine_batch_against_the_existing_path(cases, name, report):
    feats, masks, old, val = cases[name]
    before = masks.clone()
    new, values = ncut.ncut_refine_batch(feats, masks, tau=TAU, eps=EPS, return_values=True, **KW)
    assert torch.equal(masks, before) and new.shape == masks.shape and new.dtype == torch.float32
    assert tuple(values.shape) == (3, KW["steps"]) and values.dtype == torch.float64
    new, values = new.cpu().numpy(), values.cpu().numpy()
    d = np.abs(new - old).reshape(3, -1).max(1)
    e = [abs(values[b, 0] - val[b]) / abs(val[b]) for b in range(3)]
    moved = np.abs(old - before.cpu().numpy()).mean()
    print(f"{name}: max |batch - per-frame| per frame {d.tolist()}, value rel {e}, values[0] {values[0].tolist()}, mean |moved| {moved:.3f}")
    report(f"ncut_refine_batch vs ncut_refine, {name}: refined mask max |d| {d.max():.2e}, NCut before step 1 max rel {max(e):.2e}")
    assert moved > 0.01                                                        # the refinement does something on these inputs
    assert d.max() <= TOL
    assert max(e) <= 1e-5
    assert np.isfinite(values).all() and (new >= 0).all() and (new <= 1).all()
    if name == "n96":
        dg = np.abs(new[0] - cases["golden_refined"]).max()
        report(f"ncut_refine_batch frame 0 vs the reference's refined mask: max |d| {dg:.2e}")
        assert dg <= TOL


@pytest.mark.parametrize("name", ["n96", "n101"])
def test_refine_batch_is_batch_independent_and_repeatable(cases, name):
    feats, masks = cases[name][:2]
    bits_of = lambda t: t.cpu().numpy().view(np.int32 if t.dtype == torch.float32 else np.int64)
    x3, v3 = ncut.ncut_refine_batch(feats, masks, tau=TAU, eps=EPS, return_values=True, **KW)
    again = ncut.ncut_refine_batch(feats, masks, tau=TAU, eps=EPS, return_values=True, **KW)
    assert np.array_equal(bits_of(x3), bits_of(again[0])) and np.array_equal(bits_of(v3), bits_of(again[1]))
    for b in range(3):
        x1, v1 = ncut.ncut_refine_batch(feats[b:b + 1], masks[b:b + 1], tau=TAU, eps=EPS, return_values=True, **KW)
        assert np.array_equal(bits_of(x1[0]), bits_of(x3[b])) and np.array_equal(bits_of(v1[0]), bits_of(v3[b])), b
    perm = [2, 0, 1]
    xp = ncut.ncut_refine_batch(feats[perm], masks[perm], tau=TAU, eps=EPS, **KW)
    assert np.array_equal(bits_of(xp), bits_of(x3[perm]))


def test_zero_steps_return_the_input(cases):
    feats, masks = cases["n101"][:2]
    out, values = ncut.ncut_refine_batch(feats, masks, tau=TAU, eps=EPS, steps=0, learning_rate=0.45, weight_decay=1e-6, return_values=True)
    assert torch.equal(out, masks) and out.data_ptr() != masks.data_ptr() and tuple(values.shape) == (3, 0)


def test_largest_supported_n_and_the_error_above_it(report):
    """n = RCF_NCUT_PACKED_MAX_N (the frame's x fills the 64 KB of LDS the row-sum kernel may ask for) against the existing
    path, and n + 1 as an error status (raised by _lib.call) that leaves x untouched"""
    nmax = ncut.MAX_PACKED_N
    g = np.random.Generator(np.random.PCG64(9))
    feats, mask = _clustered(77, 128, 128, dim=16)
    assert mask.size == nmax
    feats, mask = torch.from_numpy(feats).to(DEV), torch.from_numpy(mask).to(DEV)
    new, values = ncut.ncut_refine_batch(feats, mask[None], tau=TAU, eps=EPS, return_values=True, **KW)
    old = ncut.ncut_refine(feats, mask, tau=TAU, eps=EPS, **KW)
    v0 = float(ncut.soft_ncut_value(feats, mask, TAU, EPS))
    d = float((new[0] - old).abs().max())
    e = abs(float(values[0, 0]) - v0) / abs(v0)
    report(f"ncut_refine_batch vs ncut_refine at n = {nmax}: refined mask max |d| {d:.2e}, NCut before step 1 rel {e:.2e}")
    assert d <= TOL and e <= 1e-5
    n = nmax + 1
    x = torch.from_numpy(g.random((1, n)).astype(np.float32)).to(DEV)
    keep = x.clone()
    bits = torch.zeros((1, n, ncut.pack_words(n)), dtype=torch.int32, device=DEV)
    deg = torch.zeros((1, n), dtype=torch.int32, device=DEV)
    assert _lib.load().rcf_ncut_refine_packed_workspace_bytes(1, n) == 0
    ws = torch.empty(n * 16, dtype=torch.uint8, device=DEV)
    rc = _lib.load().rcf_ncut_refine_packed_f32(_p(bits), _p(deg), n, 1, EPS, _p(x), 10, 0.45, 1e-6, None, _p(ws), n * 16, _stream())
    assert rc == -1
    with pytest.raises(_lib.RcfHipError, match="rcf_ncut_refine_packed_f32"):
        ncut.refine_packed(bits, deg, x, EPS, 10, 0.45, 1e-6)
    torch.cuda.synchronize()
    assert torch.equal(x, keep)


# ---- merge ---------------------------------------------------------------------------------------------------------------
def _merge_numpy(a, b, umi_th):
    """semantic_constraints.py:314-336 frame by frame -> (u8, xor counts)"""
    out, counts = [], []
    for x, y in zip(a, b):
        A, B = x > 0.5, y > 0.5
        u = (A | B).sum()
        umi = float("nan") if u == 0 else u - (A & B).sum()
        counts.append(int((A ^ B).sum()))
        r = x if (umi_th is not None and umi > umi_th) else x * y
        out.append((r * 255.).astype(np.uint8))
    return np.stack(out), np.array(counts, dtype=np.int64)


def _merge_hip(a, b, umi_th):
    n, H, W = a.shape
    out = torch.full((n, H, W), 7, dtype=torch.uint8, device=DEV)
    counts = torch.full((n,), -5, dtype=torch.int64, device=DEV)                # the call writes them: no zero fill asked
    _lib.call("rcf_mask_merge_u8", _p(a), _p(b), n, H * W, -1 if umi_th is None else int(umi_th), _p(out), _p(counts), _stream())
    return out.cpu().numpy(), counts.cpu().numpy()


def test_merge_is_bit_exact():
    g = np.random.default_rng(12)
    a, b = g.random((3, 37, 53), dtype=np.float32), g.random((3, 37, 53), dtype=np.float32)
    a[0, :5], b[0, :5] = 0.5, 0.5                                              # exactly 0.5 is not above it
    b[1, 10:] = a[1, 10:]                                                      # frames that disagree on different numbers of pixels
    b[2, 25:] = a[2, 25:]
    ad, bd = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    want, cw = _merge_numpy(a, b, None)
    got, cg = _merge_hip(ad, bd, None)
    assert np.array_equal(got, want) and np.array_equal(cg, cw)
    lo, mid, hi = np.argsort(cw)
    assert cw[lo] < cw[mid] < cw[hi]
    th = int(cw[mid])                                                          # one frame above, one below, one exactly equal
    want, _ = _merge_numpy(a, b, th)
    got, cg = _merge_hip(ad, bd, th)
    assert np.array_equal(got, want) and np.array_equal(cg, cw)
    assert np.array_equal(got[hi], (a[hi] * 255.).astype(np.uint8)) and not np.array_equal(got[hi], (a[hi] * b[hi] * 255.).astype(np.uint8))
    for f in (lo, mid):                                                        # equal is not above: the product
        assert np.array_equal(got[f], (a[f] * b[f] * 255.).astype(np.uint8))
    for t in (0, int(cw[lo]) - 1, int(cw[hi]), 10 ** 12):
        want, _ = _merge_numpy(a, b, t)
        assert np.array_equal(_merge_hip(ad, bd, t)[0], want), t
    # a frame where both masks are <= 0.5 everywhere: the reference's UMI is NaN, NaN > th is false, the product is kept
    a[1] *= 0.5
    b[1] *= 0.5
    ad, bd = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    for t in (None, 0, th):
        want, cw2 = _merge_numpy(a, b, t)
        got, cg = _merge_hip(ad, bd, t)
        assert cw2[1] == 0 and np.array_equal(cg, cw2) and np.array_equal(got, want), t
        assert np.array_equal(got[1], (a[1] * b[1] * 255.).astype(np.uint8))


# ---- head and driver -----------------------------------------------------------------------------------------------------
def _frames(seed, count):
    """f32 [count,480,854,3] in [0,1] flat-region frames and [count,480,854] masks: the object rectangle, shifted"""
    g = np.random.default_rng(seed)
    imgs, masks = [], []
    for t in range(count):
        img, m = synth._maa_frame(g, t % 3, t)
        imgs.append(img.astype(np.float32) / 255.)
        masks.append(np.where(np.roll(m, (40, 60), axis=(0, 1)), 0.9, 0.1).astype(np.float32))
    return torch.from_numpy(np.stack(imgs)).to(DEV), torch.from_numpy(np.stack(masks)).to(DEV)


def _check_head(head, imgs, masks, label, report, must_move):
    per_frame = head(imgs, masks, standardize=True)
    batch = head.forward_batch(imgs, masks, standardize=True)
    assert batch.shape == per_frame.shape == (2, 480, 854) and batch.dtype == torch.float32
    small_imgs, small = head._inputs(imgs, masks, True)
    feats = head.get_feats(small_imgs)
    want = torch.stack([ncut.ncut_refine(feats[b:b + 1], small[b], head.tau, head.eps, head.steps, head.learning_rate, head.weight_decay)
                        for b in range(2)])
    got = head.refine_batch(imgs, masks, standardize=True)
    assert got.shape == (2, 60, 107)
    d_small, d_full = float((got - want).abs().max()), float((batch - per_frame).abs().max())
    moved = float((want - small).abs().mean())
    report(f"NCutHead.forward_batch vs forward, {label}, 2 frames of 480x854: before the resize max |d| {d_small:.2e}, after {d_full:.2e} "
           f"(mean |refined - mask| {moved:.3f})")
    assert d_small <= TOL and d_full <= TOL
    if must_move:
        assert moved > 0.01
    assert torch.equal(batch, head.forward_batch(imgs, masks, standardize=True))


def test_head_forward_batch_against_forward(report):
    imgs, masks = _frames(3, 2)
    m = vit.vit_small(patch_size=8)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.fill_vit_state_dict(shapes, seed=21).items()})
    # seeded weights give nearly identical tokens (affinity all ones): this leg checks the plumbing around the real ViT
    _check_head(ncut.NCutHead(args=None, model=m, **KW).to(DEV).eval(), imgs, masks, "seeded ViT-S/8", report, False)
    # ... and features that tell the regions apart check the refinement itself at n = 6 420
    _check_head(ncut.NCutHead(args=None, model=synth.PatchFeatures(), **KW).to(DEV).eval(), imgs, masks, "PatchFeatures", report, True)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """synth.maa_tree as a stage-2.1 export: 2 sequences x 2 frames, the export directory under its `_ema` name"""
    root = str(tmp_path_factory.mktemp("semantic_tree"))
    pretrain, data_dir = synth.maa_tree(root)
    os.rename(os.path.join(pretrain, maa.EXPORT_DIR_NAME), os.path.join(pretrain, semantic.EXPORT_DIR_NAMES["davis"]))
    images = maa.dataset_layout("davis", data_dir)[0]
    shutil.rmtree(os.path.join(images, "dog"))
    os.remove(os.path.join(images, "blackswan", "00002.jpg"))
    return pretrain, data_dir, [("blackswan", "00000"), ("blackswan", "00001"), ("camel", "00000"), ("camel", "00001")]


def test_main_end_to_end(tree, capsys):
    from PIL import Image
    pretrain, data_dir, frames = tree
    ch = synth.MAA_TREE_OBJECT
    model = synth.PatchFeatures()
    argv = ["--pretrain_dir", pretrain, "--data_dir", data_dir, "--dataset", "davis", "--object-channel", str(ch), "--batch-frames", "3"]
    written = semantic.main(argv, model=model)
    out = capsys.readouterr().out
    export, save_dir = semantic.export_dirs(pretrain, "davis", ch)
    assert save_dir.endswith(os.path.join("saved_eval_export_trainval_ema_torchcrf_ncut_torchcrf", str(ch)))
    assert "Found 2 sequences: ['blackswan', 'camel']" in out and f"Start refinement: {save_dir}" in out
    assert written == [os.path.join(save_dir, f"pred_seg_{s}_{f}_0000000.png") for s, f in frames]
    assert sorted(os.listdir(save_dir)) == [os.path.basename(p) for p in written]
    # the same inputs through the heads directly, in the driver's batches of 3 + 1
    images_dir = maa.dataset_layout("davis", data_dir)[0]
    head = ncut.NCutHead(args=None, model=model, **semantic.NCUT_KW).to(DEV).eval()
    single = crf.CRFHead(args=None, crf_scale=0.7, **semantic.CRF_KW)
    double = crf.CRFHead(args=None, crf_scale=0.5, **semantic.CRF_KW)
    want = []
    for i in (0, 3):
        chunk = frames[i:i + 3]
        imgs = torch.from_numpy(np.stack([maa.load_image(images_dir, s, f) for s, f in chunk])).to(DEV)
        masks = torch.from_numpy(np.stack([maa.load_mask(export, s, f, ch, 0) for s, f in chunk])).to(DEV)
        refined = head.forward_batch(imgs, masks, standardize=True)
        u8, counts = offline.double_crf_merge_u8(single, double, imgs, masks, refined, umi_th=None, return_counts=True)
        assert u8.dtype == torch.uint8 and u8.is_cuda and tuple(u8.shape) == (len(chunk), 480, 854) and counts.dtype == torch.int64
        a, b = single(imgs, masks, unstandardize=False), double(imgs, refined, unstandardize=False)
        assert torch.equal(u8, (offline.double_crf_merge(single, double, imgs, masks, refined) * 255.).to(torch.uint8))
        assert torch.equal(counts, ((a > 0.5) ^ (b > 0.5)).flatten(1).sum(1))
        want.append(u8.cpu().numpy())
    want = np.concatenate(want)
    assert 0 < (want == 255).mean() < 1                                        # masks with an object in them
    for p, u8 in zip(written, want):
        im = Image.open(p)
        assert im.mode == "L" and im.size == (854, 480)
        assert np.array_equal(np.asarray(im), u8), p
    # a second run refuses to overwrite, before it refines anything
    stamps = [os.path.getmtime(p) for p in written]
    with pytest.raises(FileExistsError, match="pred_seg_blackswan_00000_0000000.png"):
        semantic.main(argv, model=model)
    assert [os.path.getmtime(p) for p in written] == stamps


def test_fbms_threshold_reaches_the_merge():
    """Refiner(umi_th) keeps the single-CRF mask of a frame whose two CRF outputs disagree on more pixels than the threshold"""
    imgs, masks = _frames(8, 2)
    r = semantic.Refiner(synth.PatchFeatures(), umi_th=None)
    refined = r.ncut_head.forward_batch(imgs, masks, standardize=True)
    refined[1] = 1.0 - refined[1]                                             # frame 1: the two CRFs see opposite masks
    prod, counts = offline.double_crf_merge_u8(r.crf_head_single, r.crf_head, imgs, masks, refined, None, return_counts=True)
    c = counts.cpu().numpy()
    assert c[1] > c[0]
    th = int(c[0])
    got = offline.double_crf_merge_u8(r.crf_head_single, r.crf_head, imgs, masks, refined, th)
    a = r.crf_head_single(imgs, masks, unstandardize=False)
    assert torch.equal(got[0], prod[0]) and torch.equal(got[1], (a[1] * 255.).to(torch.uint8)) and not torch.equal(got[1], prod[1])
    assert semantic.Refiner(synth.PatchFeatures(), umi_th=semantic.UMI_TH["fbms59"]).umi_th == 10000
