"""GPU: MAA object-channel selection -- ncut.soft_ncut_values (rcf_ncut_values_f32: the NCut terms of all masks in one
pass over the raw Gram matrix), NCutEvalHead.forward_multi and rcf_amd.maa.main against tests/golden/maa.json, which
make_golden_maa.py captured from the reference's maa.py on the CPU.

Bars.  Values: relative error <= max(1e-5, 10 x the reference's own fp32-to-float64 deviation stored for that value); 1e-5
is the bar test_soft_ncut_vs_reference_golden applies to the same quantity.  Against the existing per-mask path: 1e-6 (it
stores its value in fp32).  Anything computed from device-side image preprocessing: 1e-4 (test_vit_gpu.py's TOL)."""
import json
import os

import numpy as np
import pytest
import torch

import rcf_amd
from rcf_amd import maa, ncut, synth, vit

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL_TREE = 1e-4


@pytest.fixture(scope="module")
def fx(golden_dir):
    return json.load(open(os.path.join(golden_dir, "maa.json")))


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return synth.maa_tree(str(tmp_path_factory.mktemp("maa_tree")))


def _inputs(case):
    feats = torch.from_numpy(synth.maa_features(case["feature_seed"], case["hf"], case["wf"], case["noise"])).to(DEV)
    masks = torch.from_numpy(synth.maa_masks(case["mask_seed"], case["hf"], case["wf"], case["M"]))
    if case["zero_masks"]:
        masks = torch.zeros_like(masks)
    return feats, masks[None].to(DEV)


def test_values_against_the_reference(fx, report):
    for case in fx["cases"]:
        feats, masks = _inputs(case)
        terms = ncut.soft_ncut_values(feats, masks, fx["tau"], fx["eps"], return_terms=True)[0].cpu().numpy()
        assert terms.shape == (case["M"], 4) and terms.dtype == np.float64
        errs = []
        for m, gold in enumerate(case["masks"]):
            got, (cut, aA, aB) = terms[m, 0], terms[m, 1:]
            ref = float.fromhex(gold["ref_f32_hex"])
            if np.isnan(ref):
                assert np.isnan(got), (case["name"], m, got)
                assert cut == 0.0 and aA == 0.0 and np.isfinite(aB)
                continue
            bar = max(1e-5, 10 * gold["rel_dev"])
            e = abs(got - ref) / abs(ref)
            errs.append(e)
            print(f"{case['name']} mask {m}: hip {got!r} reference fp32 {ref!r} float64 {gold['f64']!r} rel {e:.2e} bar {bar:.1e}")
            assert e <= bar, (case["name"], m, got, ref, e, bar)
            assert np.isfinite(terms[m]).all() and cut > 0 and aA > 0 and aB > 0
            assert abs(got - (cut / aA + cut / aB)) <= 1e-14 * abs(got)
            if case["gram_entries_near_tau"] == 0:          # no entry can fall on the other side of tau: rounding alone
                for v, k in ((cut, "cut64"), (aA, "assocA64"), (aB, "assocB64")):
                    assert abs(v - gold[k]) <= bar * abs(gold[k]), (case["name"], m, k, v, gold[k])
        report(f"soft_ncut_values vs reference, {case['name']} (n {case['hf'] * case['wf']}, M {case['M']}, "
               f"{case['gram_entries_near_tau']} Gram entries within 1e-5 of tau): max rel {max(errs, default=0.0):.2e}")


def test_against_the_existing_per_mask_path(fx, report):
    worst = 0.0
    for case in fx["cases"]:
        if case["zero_masks"]:
            continue
        feats, masks = _inputs(case)
        new = ncut.soft_ncut_values(feats, masks, fx["tau"], fx["eps"])[0].cpu().numpy()
        for m in range(case["M"]):
            old = float(ncut.soft_ncut_value(feats, masks[0, m], fx["tau"], fx["eps"]))
            e = abs(new[m] - old) / abs(old)
            worst = max(worst, e)
            print(f"{case['name']} mask {m}: one-pass {new[m]!r} per-mask path {old!r} rel {e:.2e}")
            assert e <= 1e-6, (case["name"], m, new[m], old)
    report(f"soft_ncut_values vs ncut.soft_ncut_value on the same features: max rel {worst:.2e}")


def _bits(t):
    return t.cpu().numpy().view(np.int64)


def test_batching_and_determinism(fx):
    tau, eps = fx["tau"], fx["eps"]
    hf, wf = 13, 21                                                           # n = 273: a quad tail, several row chunks
    feats = torch.cat([torch.from_numpy(synth.maa_features(300 + i, hf, wf, 1.2)) for i in range(3)]).to(DEV)
    masks = torch.stack([torch.from_numpy(synth.maa_masks(400 + i, hf, wf, 11)) for i in range(3)]).to(DEV)
    all3 = ncut.soft_ncut_values(feats, masks[:, :4], tau, eps, return_terms=True)
    assert np.array_equal(_bits(all3), _bits(ncut.soft_ncut_values(feats, masks[:, :4], tau, eps, return_terms=True)))   # two calls
    for i in range(3):                                                       # F = 1 against position i of F = 3
        one = ncut.soft_ncut_values(feats[i:i + 1], masks[i:i + 1, :4], tau, eps, return_terms=True)
        assert np.array_equal(_bits(one[0]), _bits(all3[i])), i
    perm = [2, 0, 1]                                                         # any position
    moved = ncut.soft_ncut_values(feats[perm], masks[perm, :4], tau, eps, return_terms=True)
    assert np.array_equal(_bits(moved), _bits(all3[perm]))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        side = ncut.soft_ncut_values(feats, masks[:, :4], tau, eps, return_terms=True)
    s.synchronize()
    assert np.array_equal(_bits(side), _bits(all3))
    full = ncut.soft_ncut_values(feats, masks, tau, eps, return_terms=True)   # M = 11: groups of 8 + 3
    assert full.shape == (3, 11, 4)
    for M in range(1, 12):                                                    # M = 1..8 one call, 9..11 through the grouping
        part = ncut.soft_ncut_values(feats, masks[:, :M], tau, eps, return_terms=True)
        assert np.array_equal(_bits(part), _bits(full[:, :M])), M
    # the big size too: a frame of the n = 6420 case alone and between two others
    case = fx["cases"][0]
    f1, m1 = _inputs(case)
    alone = ncut.soft_ncut_values(f1, m1, tau, eps, return_terms=True)
    f3 = torch.cat([f1.flip(1), f1, f1 * 0.5])
    three = ncut.soft_ncut_values(f3, m1.expand(3, -1, -1, -1).contiguous(), tau, eps, return_terms=True)
    assert np.array_equal(_bits(alone[0]), _bits(three[1]))


def _tree_inputs(tree, fx, frames):
    pretrain_dir, data_dir = tree
    images = maa.dataset_layout("davis", data_dir)[0]
    imgs, masks = [], []
    for name in frames:
        seq, fid = name.split("/")
        imgs.append(maa.load_image(images, seq, fid))
        masks.append(np.stack([maa.load_mask(os.path.join(pretrain_dir, maa.EXPORT_DIR_NAME), seq, fid, c, 0)
                               for c in range(synth.MAA_TREE_CHANNELS)]))
    return torch.from_numpy(np.stack(imgs)).to(DEV), torch.from_numpy(np.stack(masks)).to(DEV)


def test_head_forward_multi_against_the_tree_fixture(fx, tree, report):
    t = fx["tree"]
    head = ncut.NCutEvalHead(args=None, model=synth.PatchFeatures()).to(DEV).eval()
    gold = np.array(t["ncut"])
    got = []
    for i in range(0, len(t["frames"]), 3):                                    # batches of 3, 3, 2 frames
        imgs, masks = _tree_inputs(tree, fx, t["frames"][i:i + 3])
        out = head.forward_multi(imgs, masks, standardize=True)
        assert out.shape == (imgs.shape[0], synth.MAA_TREE_CHANNELS) and out.dtype == np.float64
        got.append(out)
    got = np.concatenate(got)
    e = np.abs(got - gold) / np.abs(gold)
    print("forward_multi", got.tolist(), "fixture", gold.tolist())
    report(f"NCutEvalHead.forward_multi vs reference on the synthetic tree ({len(gold)} frames x {gold.shape[1]} channels): max rel {e.max():.2e}")
    assert e.max() <= TOL_TREE
    imgs, masks = _tree_inputs(tree, fx, t["frames"][:1])                     # forward (one mask) gives the same value
    single = head(imgs, masks[:, 1], standardize=True)
    assert single.shape == (1,) and abs(single[0] - got[0, 1]) <= 1e-6 * abs(got[0, 1])


def _args(tree, *extra):
    return ["--pretrain_dir", tree[0], "--data_dir", tree[1], "--dataset", "davis", "--num-channels", str(synth.MAA_TREE_CHANNELS)] + list(extra)


def test_main_end_to_end(fx, tree, capsys, report):
    t = fx["tree"]
    model = synth.PatchFeatures()
    maas, best = maa.main(_args(tree), model=model)
    out = capsys.readouterr().out
    assert best == t["best_channel"] == synth.MAA_TREE_OBJECT
    e = np.abs(np.array(maas) - np.array(t["frame_maas"])) / np.abs(np.array(t["frame_maas"]))
    report(f"maa.main on the synthetic tree: frame MAAs {[round(float(m), 6) for m in maas]} vs fixture max rel {e.max():.2e}, best channel {best}")
    assert e.max() <= TOL_TREE
    assert "Dataset: davis" in out and f"Found {len(synth.MAA_TREE)} sequences: {sorted(s for s, _, _ in synth.MAA_TREE)}" in out
    for c, m in enumerate(maas):
        assert f"frame MAA with object channel {c}: {m * 100.:.2f}" in out
    assert f"The best object channel among all channels evaluated is channel {best}" in out
    # batching does not change the choice or (within the bar) the values
    maas1, best1 = maa.main(_args(tree, "--batch-frames", "1"), model=model)
    assert best1 == best and np.allclose(maas1, maas, rtol=TOL_TREE, atol=0)
    # --first-frames-only: one frame per sequence
    maas_f, best_f = maa.main(_args(tree, "--first-frames-only"), model=model)
    gold_f = np.array(t["frame_maas_first_frames"])
    assert best_f == int(np.argmax(gold_f)) and (np.abs(np.array(maas_f) - gold_f) / np.abs(gold_f)).max() <= TOL_TREE
    capsys.readouterr()
    # --object-channel k: that channel alone, no best-channel line and no exit code
    maas_k, best_k = maa.main(_args(tree, "--object-channel", "2"), model=model)
    out = capsys.readouterr().out
    assert best_k is None and len(maas_k) == 1 and abs(maas_k[0] - t["frame_maas"][2]) <= TOL_TREE * abs(t["frame_maas"][2])
    assert "frame MAA with object channel 2:" in out and "best object channel" not in out


def test_main_with_the_real_vit(tree, capsys):
    """the real ViT-S/8 with seeded weights: tokens are nearly identical (affinity all ones), so the values are degenerate and
    only the run itself is checked"""
    m = vit.vit_small(patch_size=8)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.fill_vit_state_dict(shapes, seed=21).items()})
    maas, best = maa.main(_args(tree, "--first-frames-only", "--batch-frames", "2"), model=m)
    out = capsys.readouterr().out
    assert len(maas) == synth.MAA_TREE_CHANNELS and np.isfinite(maas).all()
    assert best in range(synth.MAA_TREE_CHANNELS) and f"is channel {best}" in out


def test_tool_exits_with_the_fixture_channel(fx, tree, capsys):
    """tools/maa.py on the synthetic tree: the per-channel lines, and the best channel as the exit code"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("maa_tool", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "maa.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with pytest.raises(SystemExit) as e:
        tool.cli(_args(tree), model=synth.PatchFeatures())
    out = capsys.readouterr().out
    assert e.value.code == fx["tree"]["best_channel"]
    assert all(f"frame MAA with object channel {c}:" in out for c in range(synth.MAA_TREE_CHANNELS))
