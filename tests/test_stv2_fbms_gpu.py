"""GPU: the SegTrackv2 / FBMS59 evaluation (rcf_amd.stv2_fbms) through the device resize -- the tool's lines on the synthetic
tree against the reference tool's own (tests/golden/stv2_fbms_eval.json), and its per-frame IoUs against the --host run's,
exactly, for --batch-frames 1 and 4."""
import json
import os

import pytest

import rcf_amd
from rcf_amd import stv2_fbms, synth

from test_stv2_fbms_cpu import palette_copy

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stv2_fbms_eval.json")


@pytest.fixture(scope="module")
def gold():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def tree(gold, tmp_path_factory):
    root = str(tmp_path_factory.mktemp("stv2_fbms_gpu"))
    data, pred_dirs = synth.stv2_fbms_tree(root, seed=gold["seed"], step=gold["step"])
    return root, data, pred_dirs


def _hex(vs):
    return [float(v).hex() for v in vs]


@pytest.mark.parametrize("ds", ["SegTrackv2", "FBMS59"])
def test_device_lines_equal_the_reference_tools(ds, tree, gold, capsys, report):
    _, data, pred_dirs = tree
    res = stv2_fbms.main(["--dataset", ds, "--step", str(gold["step"]), "--pred_dir", pred_dirs[ds], "--data_dir", data])
    assert capsys.readouterr().out.splitlines() == gold["lines"][ds]
    assert res["routes"]["pillow"] == 0 and res["routes"]["device"] == res["n_frames"]
    report(f"stv2_fbms {ds}: {res['n_frames']} frames in {res['routes']['device_calls']} device calls, lines equal the "
           f"reference tool's ({gold['lines'][ds][-2]})")


@pytest.mark.parametrize("ds", ["SegTrackv2", "FBMS59"])
@pytest.mark.parametrize("batch", [1, 4])
def test_per_frame_ious_equal_the_host_runs(ds, batch, tree, gold):
    _, data, pred_dirs = tree
    host = stv2_fbms.evaluate(ds, pred_dirs[ds], step=gold["step"], data_dir=data, host=True)
    dev = stv2_fbms.evaluate(ds, pred_dirs[ds], step=gold["step"], data_dir=data, batch_frames=batch)
    assert _hex(dev["ious"]) == _hex(host["ious"]) and len(dev["ious"]) == host["n_frames"]
    assert _hex(v for _, v in dev["sequences"]) == _hex(v for _, v in host["sequences"])
    assert float(dev["miou"]).hex() == float(host["miou"]).hex()
    n = dev["n_frames"]
    if batch == 1:
        assert dev["routes"]["device_calls"] == n
    else:                                   # frames of one geometry share calls: fewer calls than frames, at most 4 frames each
        assert -(-n // 4) <= dev["routes"]["device_calls"] < n


def test_mixed_modes_split_between_the_routes(tree, gold, tmp_path):
    """palette / alpha / 1-bit masks go through Pillow, the rest of the run through the device; same integers as --host"""
    _, data, pred_dirs = tree
    dst = str(tmp_path / "pred")
    modes = palette_copy(pred_dirs["SegTrackv2"], dst, "birdfall")
    host = stv2_fbms.evaluate("SegTrackv2", dst, step=gold["step"], data_dir=data, host=True)
    dev = stv2_fbms.evaluate("SegTrackv2", dst, step=gold["step"], data_dir=data, batch_frames=4)
    assert dev["routes"]["pillow"] == len(modes) and dev["routes"]["device"] == dev["n_frames"] - len(modes)
    assert _hex(dev["ious"]) == _hex(host["ious"])
