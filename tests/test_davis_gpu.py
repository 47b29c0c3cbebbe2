"""GPU: the DAVIS J & F evaluation (rcf_amd.davis, csrc/davis_eval.hip) -- per-frame J and F against the reference tool's
own numbers (tests/golden/davis.json, generator make_golden_davis.py), the six device counts against a plain numpy
restatement of davis2017/metrics.py written here, batching and stream invariance, and the whole evaluation
(DAVISEvaluation, main) on a synthetic DAVIS tree."""
import json
import os

import numpy as np
import pytest
import torch

import rcf_amd
from rcf_amd import davis, synth

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "davis.json")


@pytest.fixture(scope="module")
def gold():
    with open(GOLDEN) as f:
        return json.load(f)


def _hex(v):
    return float(v).hex()


# ---- numpy restatement (davis2017/metrics.py: _seg2bmap, disk dilation, the four boundary sums) -----------------------

def _bmap(m):
    e, s, se = np.zeros_like(m), np.zeros_like(m), np.zeros_like(m)
    e[:, :-1], s[:-1, :], se[:-1, :-1] = m[:, 1:], m[1:, :], m[1:, 1:]
    b = (m ^ e) | (m ^ s) | (m ^ se)
    b[-1, :] = m[-1, :] ^ e[-1, :]
    b[:, -1] = m[:, -1] ^ s[:, -1]
    b[-1, -1] = False
    return b


def _dilate(b, r):
    H, W = b.shape
    out = np.zeros_like(b)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            if dx * dx + dy * dy > r * r or abs(dy) >= H or abs(dx) >= W:
                continue                                  # outside the disk, or entirely outside the frame
            ys, yd = slice(max(0, dy), H + min(0, dy)), slice(max(0, -dy), H - max(0, dy))
            xs, xd = slice(max(0, dx), W + min(0, dx)), slice(max(0, -dx), W - max(0, dx))
            out[yd, xd] |= b[ys, xs]
    return out


def numpy_counts(pred, gt, void, r):
    nv = np.ones(pred.shape, bool) if void is None else void == 0
    p, g = (pred != 0) & nv, (gt != 0) & nv
    bf, bg = _bmap(p), _bmap(g)
    return np.array([(p & g).sum(), (p | g).sum(), bf.sum(), bg.sum(), (bf & _dilate(bg, r)).sum(),
                     (bg & _dilate(bf, r)).sum()], dtype=np.int64)


# ---- tests ------------------------------------------------------------------------------------------------------------

def test_golden_cases_bit_exact(gold, report):
    """per-frame J (db_eval_iou) and F (f_measure) of every fixture case == the reference's float64 values"""
    for c in gold["cases"]:
        pred, gt, vd = synth.davis_inputs(c["seed"], N=c["N"], H=c["H"], W=c["W"], kind=c["kind"], void=c["void"])
        J = [davis.db_eval_iou(gt[n], pred[n], None if vd is None else vd[n]) for n in range(c["N"])]
        F = [davis.f_measure(pred[n], gt[n], None if vd is None else vd[n], bound_th=c["bound_th"]) for n in range(c["N"])]
        assert [_hex(v) for v in J] == c["J"], c["name"]
        assert [_hex(v) for v in F] == c["F"], c["name"]
        # the batched forms: one device call for all frames of the case
        Fb = davis.db_eval_boundary(gt, pred, vd, bound_th=c["bound_th"])
        Jb = davis.db_eval_iou(gt, pred, vd)
        assert [_hex(v) for v in Fb] == c["F"] and [_hex(v) for v in Jb] == c["J"], c["name"]
    report(f"davis goldens: {len(gold['cases'])} cases, per-frame J and F bit-identical to the reference tool")


def test_counts_match_numpy_restatement(report):
    """~50 seeded odd shapes, radii 0..64, with and without void pixels: the six integers are exact"""
    g = np.random.Generator(np.random.PCG64(2016))
    n_cases = 0
    for i in range(50):
        H, W = int(g.integers(1, 200)), int(g.integers(1, 300))
        kind = synth.DAVIS_KINDS[int(g.integers(0, len(synth.DAVIS_KINDS)))] if i % 3 else "blobs"
        r = int(g.integers(0, 13)) if i % 7 else int(g.integers(13, 65))
        pred, gt, vd = synth.davis_inputs(100 + i, N=2, H=H, W=W, kind=kind, void=bool(i % 2))
        got = davis.boundary_counts(pred, gt, vd, bound_th=r if r >= 1 else 0)
        for n in range(2):
            want = numpy_counts(pred[n], gt[n], None if vd is None else vd[n], r)
            assert got[n].tolist() == want.tolist(), (i, H, W, kind, r)
        n_cases += 1
    # torch bool inputs on the device, and a [H,W] frame
    p, q, _ = synth.davis_inputs(7, N=1, H=97, W=131)
    got = davis.boundary_counts(torch.from_numpy(p[0] != 0).cuda(), torch.from_numpy(q[0] != 0).cuda())
    assert got.shape == (1, 6) and got[0].tolist() == numpy_counts(p[0], q[0], None, 2).tolist()
    report(f"davis counts: {n_cases} odd-shape cases equal the numpy restatement")


def test_all_ones_frame_has_no_boundary():
    ones = np.ones((3, 40, 90), np.uint8)
    c = davis.boundary_counts(ones, ones)
    assert c.tolist() == [[3600, 3600, 0, 0, 0, 0]] * 3
    assert davis.f_measure(ones[0], ones[0]) == 1.0 and davis.db_eval_iou(ones[0], ones[0]) == 1.0


def test_batch_of_100_frames_equals_per_frame_calls():
    pred, gt, vd = synth.davis_inputs(77, N=100, H=480, W=854, kind="blobs", void=True)
    batch = davis.boundary_counts(pred, gt, vd)
    single = np.concatenate([davis.boundary_counts(pred[n], gt[n], vd[n]) for n in range(100)])
    assert batch.shape == (100, 6) and (batch == single).all()
    assert (batch[:, 2] > 0).all()


def test_non_default_stream_equals_default():
    pred, gt, vd = synth.davis_inputs(78, N=4, H=480, W=854, kind="blobs", void=True)
    ref = davis.boundary_counts(pred, gt, vd)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        pt, gtt, vt = (torch.from_numpy(a).cuda() for a in (pred, gt, vd))
        got = davis.boundary_counts(pt, gtt, vt)
    torch.cuda.synchronize()
    assert (got == ref).all()


def _metrics_hex(m):
    return {k: {"M": [_hex(v) for v in d["M"]], "R": [_hex(v) for v in d["R"]], "D": [_hex(v) for v in d["D"]],
                "M_per_object": {s: _hex(v) for s, v in d["M_per_object"].items()},
                "seq_len": {s: int(v) for s, v in d["seq_len"].items()}} for k, d in m.items()}


def test_davis_evaluation_and_main_on_a_synthetic_tree(gold, tmp_path, capsys, report):
    davis_path, res_path = synth.davis_tree(str(tmp_path))
    for task in ("unsupervised", "semi-supervised"):
        ev = davis.DAVISEvaluation(davis_root=davis_path, task=task, gt_set="val", year="2016", step=0)
        assert _metrics_hex(ev.evaluate(res_path)) == gold["tree"][task], task
    m = davis.main(["--davis_path", davis_path, "--set", "val", "--task", "unsupervised", "--results_path", res_path,
                    "--year", "2016", "--step", "0"])
    assert _metrics_hex(m) == gold["tree"]["unsupervised"]
    for fn in ("global_results-val.csv", "per-sequence_results-val.csv"):
        with open(os.path.join(res_path, fn)) as f:
            assert f.read() == gold["tree"][fn], fn
    out = capsys.readouterr().out
    assert "Global results for val" in out and "J&F-Mean" in out
    report("davis tree: metrics_res of both tasks and both CSV files identical to the reference tool's")


def test_missing_result_frame_raises(tmp_path):
    davis_path, res_path = synth.davis_tree(str(tmp_path))
    os.remove(os.path.join(res_path, "pred_seg_dance_00003_0000000.png"))
    ev = davis.DAVISEvaluation(davis_root=davis_path, task="unsupervised", gt_set="val", year="2016")
    with pytest.raises(FileNotFoundError, match="dance frame 00003 not found"):
        ev.evaluate(res_path)
