"""CPU: the SegTrackv2 / FBMS59 evaluation (rcf_amd.stv2_fbms) with --host -- its printed lines on the synthetic tree
against the reference tool's own (tests/golden/stv2_fbms_eval.json, generator make_golden_stv2_fbms.py), the dataset rules
(missing annotations, file names, thresholds), the Pillow route for masks the kernel does not take, and the flags."""
import json
import os
import shutil

import numpy as np
import pytest

import rcf_amd
from rcf_amd import stv2_fbms, synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stv2_fbms_eval.json")


@pytest.fixture(scope="module")
def gold():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def tree(gold, tmp_path_factory):
    root = str(tmp_path_factory.mktemp("stv2_fbms"))
    data, pred_dirs = synth.stv2_fbms_tree(root, seed=gold["seed"], step=gold["step"])
    return root, data, pred_dirs


def _args(ds, tree, gold, *more):
    _, data, pred_dirs = tree
    return ["--dataset", ds, "--step", str(gold["step"]), "--pred_dir", pred_dirs[ds], "--data_dir", data, "--host", *more]


@pytest.mark.parametrize("ds", ["SegTrackv2", "FBMS59"])
def test_host_lines_equal_the_reference_tools(ds, tree, gold, capsys):
    res = stv2_fbms.main(_args(ds, tree, gold))
    printed = capsys.readouterr().out.splitlines()
    assert printed == gold["lines"][ds]
    assert stv2_fbms.report_lines(res) == printed
    assert res["routes"] == {"device": 0, "pillow": res["n_frames"], "device_calls": 0}
    assert len(res["ious"]) == res["n_frames"] and [n for n, _ in res["sequences"]] == \
        [s[1] for s in synth.STV2_FBMS_TREE if s[0] == ds]
    # the fixture exercises what it claims: a nan frame per dataset, and values strictly between 0 and 1
    assert sum(np.isnan(v) for v in res["ious"]) == 1
    assert all(0 < v < 1 for v in res["ious"] if not np.isnan(v))


def test_tree_covers_both_directions_and_the_threshold(tree, gold):
    """enlargement, reduction, equal sizes, one axis only, an L export; and the exported masks crowd the threshold"""
    from PIL import Image
    kinds = set()
    for ds, seq, T, (h, w), (H, W), pmode, amode in synth.STV2_FBMS_TREE:
        kinds.add("equal" if (h, w) == (H, W) else "one_axis" if h == H or w == W else "up" if H > h and W > w else
                  "down" if H < h and W < w else "mixed")
        img = Image.open(os.path.join(tree[2][ds], f"pred_seg_{seq}_00000_{gold['step']:07}.png"))
        assert img.mode == pmode and img.size == (w, h)
        p = np.array(img)
        assert np.isin(p, (88, 89, 90, 91)).mean() > 0.1
    assert {"equal", "one_axis", "up", "down"} <= kinds
    assert {s[5] for s in synth.STV2_FBMS_TREE} == {"L", "RGB"}


def test_fbms_skips_and_segtrack_asserts(tree, gold, tmp_path):
    root, data, pred_dirs = tree
    res = stv2_fbms.evaluate("FBMS59", pred_dirs["FBMS59"], step=gold["step"], data_dir=data, host=True)
    listed = sum(s[2] for s in synth.STV2_FBMS_TREE if s[0] == "FBMS59")
    assert res["n_frames"] == listed - len(synth.STV2_FBMS_UNANNOTATED) == 8
    # SegTrackv2 with one annotation removed: the reference's assertion and message
    data2 = str(tmp_path / "data")
    shutil.copytree(data, data2)
    victim = os.path.join(data2, "data_SegTrackv2", "Annotations", "frog", "00002.jpg")
    os.remove(victim)
    with pytest.raises(AssertionError, match="does not exist, but skipping ground truth is not allowed") as e:
        stv2_fbms.evaluate("SegTrackv2", pred_dirs["SegTrackv2"], step=gold["step"], data_dir=data2, host=True)
    assert os.path.join("data_SegTrackv2", "Annotations/frog/", "00002.jpg") in str(e.value)
    # a wrong step: the prediction file name carries it
    with pytest.raises(FileNotFoundError, match="pred_seg_birdfall_00000_0000004.png"):
        stv2_fbms.evaluate("SegTrackv2", pred_dirs["SegTrackv2"], step=4, data_dir=data, host=True)


def test_threshold_constants():
    assert stv2_fbms.pred_min_for() == 90 and 89 / 255. <= 0.35 < 90 / 255.
    assert stv2_fbms.pred_min_for(0.0) == 1 and stv2_fbms.pred_min_for(1.0) == 256 and stv2_fbms.pred_min_for(-1) == 0
    assert np.isnan(stv2_fbms.iou_from_counts((0, 0)))
    v = stv2_fbms.iou_from_counts((1, 3))
    assert isinstance(v, np.float64) and v == np.int64(1) / np.int64(3)


def test_annotation_rule_on_other_dtypes(tmp_path):
    """arr / 255. > 0.5 in float64 on whatever Pillow returns: 127 off, 128 on; a 1-bit image is all off (True / 255.);
    16-bit values above 127 on; channel 0 of RGB"""
    from PIL import Image
    a = np.array([[0, 127, 128, 255]], dtype=np.uint8)
    Image.fromarray(a).save(tmp_path / "l.png")
    assert stv2_fbms.read_annotation(str(tmp_path / "l.png")).tolist() == [[0, 0, 1, 1]]
    Image.fromarray(a > 0).save(tmp_path / "b.png")
    assert Image.open(tmp_path / "b.png").mode == "1"
    assert stv2_fbms.read_annotation(str(tmp_path / "b.png")).tolist() == [[0, 0, 0, 0]]
    Image.fromarray(np.array([[0, 127, 128, 65535]], dtype=np.uint16)).save(tmp_path / "w.png")
    assert stv2_fbms.read_annotation(str(tmp_path / "w.png")).tolist() == [[0, 0, 1, 1]]
    Image.fromarray(np.stack([a, 255 - a, a * 0], -1)).save(tmp_path / "rgb.png")
    assert stv2_fbms.read_annotation(str(tmp_path / "rgb.png")).tolist() == [[0, 0, 1, 1]]


def _reference_ious(ds, pred_dir, data, step):
    """eval_tool.py's loop restated with Pillow for whatever mode the files have"""
    from PIL import Image
    sub, list_name, skip, png = stv2_fbms.DATASETS[ds]
    out = []
    for line in open(os.path.join(data, sub, list_name)):
        parts = line.split()
        seq = parts[0].split("/")[-2]
        for i, frame in enumerate(parts[1:]):
            path = os.path.join(data, sub, "Annotations", seq, frame.replace(".jpg", ".png") if png else frame)
            if not os.path.exists(path):
                continue
            ann = np.array(Image.open(path)) / 255.
            ann = (ann[..., 0] if ann.ndim == 3 else ann) > 0.5
            pred = np.array(Image.open(os.path.join(pred_dir, f"pred_seg_{seq}_{i:05}_{step:07}.png"))
                            .resize((ann.shape[1], ann.shape[0]))) / 255.
            pred = (pred[..., 0] if pred.ndim == 3 else pred) > 0.35
            u = (pred | ann).sum()
            out.append(float("nan") if u == 0 else (pred & ann).sum() / u)
    return out


def palette_copy(pred_dir, dst, seq):
    """a copy of a prediction directory with one sequence's masks rewritten as palette / RGBA / 1-bit PNGs"""
    from PIL import Image
    shutil.copytree(pred_dir, dst)
    modes = ["P", "RGBA", "1", "LA"]
    names = sorted(n for n in os.listdir(dst) if n.startswith(f"pred_seg_{seq}_"))
    for i, n in enumerate(names):
        img = Image.open(os.path.join(dst, n))
        img.load()
        mode = modes[i % len(modes)]
        img = img.convert("L").convert(mode) if mode != "1" else img.convert("L").point(lambda v: 255 * (v >= 92), "1")
        img.save(os.path.join(dst, n))
    return [modes[i % len(modes)] for i in range(len(names))]


def test_palette_and_alpha_predictions_take_the_pillow_route(tree, gold, tmp_path):
    root, data, pred_dirs = tree
    dst = str(tmp_path / "pred")
    modes = palette_copy(pred_dirs["SegTrackv2"], dst, "birdfall")
    assert "P" in modes
    res = stv2_fbms.evaluate("SegTrackv2", dst, step=gold["step"], data_dir=data, host=True)
    want = _reference_ious("SegTrackv2", dst, data, gold["step"])
    assert [float(v).hex() for v in res["ious"]] == [float(v).hex() for v in want]
    # and the restated loop is the tool: on the unmodified tree it reproduces the per-frame values of the golden run
    plain = stv2_fbms.evaluate("SegTrackv2", pred_dirs["SegTrackv2"], step=gold["step"], data_dir=data, host=True)
    want = _reference_ious("SegTrackv2", pred_dirs["SegTrackv2"], data, gold["step"])
    assert [float(v).hex() for v in plain["ious"]] == [float(v).hex() for v in want]
    assert res["ious"][:4] != plain["ious"][:4]                               # the other modes do resize differently


def test_flag_parsing():
    a = stv2_fbms.parse_args(["--dataset", "FBMS59", "--pred_dir", "x"])
    assert (a.dataset, a.step, a.pred_dir, a.data_dir, a.batch_frames, a.host) == ("FBMS59", 0, "x", "data", 16, False)
    a = stv2_fbms.parse_args(["--dataset", "SegTrackv2", "--step", "7", "--pred_dir", "p/0", "--data_dir", "d",
                              "--batch-frames", "4", "--host"])
    assert (a.dataset, a.step, a.pred_dir, a.data_dir, a.batch_frames, a.host) == ("SegTrackv2", 7, "p/0", "d", 4, True)
    for bad in (["--dataset", "DAVIS", "--pred_dir", "x"], ["--pred_dir", "x"], ["--dataset", "FBMS59"]):
        with pytest.raises(SystemExit):
            stv2_fbms.parse_args(bad)
