#!/usr/bin/env python3
"""Fixture for rcf_amd.AMDModel: the REFERENCE's own AMDModel (models/amd/amd_model.py, unmodified) decides the numbers.

Runs the reference on the CPU under the stand-in modules of make_golden.py (mmcv / mmseg / torchvision / ... replaced by torch's own
arithmetic), with BN for SyncBN, dropout 0, log_interval 10^9 and train_iter 1 (tests/amd_cases.py::model_kwargs, the values of
configs/amd/amd.yaml otherwise), on B = 2 pairs of 96 x 160 frames with M = 5; the flow side runs at the reference's 384 x 640.  The
weights are seeded and regenerable (amd_cases.state_dict: synth.fill_state_dict, pwc_cases.draw_params for the flow network) and are
not stored.  amd.npz holds data only:
  names, shapes                  the reference's state-dict names and shapes (shapes flattened, -1 between them)
  truth_logits, truth_dlogits    the float64 run's decode_head2 output [B I, M, h, w] (training mode) and the loss's gradient there
  truth_loss                     the float64 loss (w_seg * loss_seg)
  gradnorm_keys, truth_gradnorm  per top-level module, the norm of its parameters' float64 gradients
  sampled, truth_grad_<i>        the first 256 elements of the float64 gradient of parameter sampled[i]
  truth_eval_masks0              the float64 evaluation-mode masks of frame 0 [B, M, h, w] (models/amd/amd_model.py:155-192)
  ref32_err_*                    for each of these, the reference's OWN float32 error against the float64 run, relative to range
                                 (masks: absolute): the worst of its default float32 run and of one run at weights moved by one unit
                                 in the last place -- the yardstick of the GPU tests, as in rcf_small.npz
  kink_distance, kink_count      the smallest LeakyReLU pre-activation of the flow network's float64 run relative to its layer's
                                 largest, and how many lie within pwc_cases.MIN_KINK_DISTANCE
The conditioning that make_golden_pwclite.py reaches by redrawing its seed -- the float32 run's loss and logit gradient within 1e-5 of
their range of the float64 run, no LeakyReLU pre-activation of the flow network within MIN_KINK_DISTANCE -- is NOT reachable here: at
384 x 640 the flow network has ten times the activations of that fixture's larger case (where one draw in fifty clears the second
condition).  A scan of twenty seeds (`--scan`, 5101 .. 5120) found 56 - 78 such pre-activations in every run, the float32 loss within
5e-7 in every run, and the float32 logit gradient 3.3e-4 .. 1.6e-3 of its range away from the float64 run (a slope decided differently
moves it by that much).  amd_cases.SEED is the scan's best seed (5119, 3.3e-4); what it has is recorded in ref32_err_* and kink_*, and
the GPU tests' limits follow from those.

Regenerate, where a checkout of the reference exists:  python tests/golden/make_golden_amd.py <reference checkout>
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (HERE, os.path.dirname(HERE), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
import amd_cases as ac  # noqa: E402
import pwc_cases as pc  # noqa: E402

SCAN_FROM, SCAN = 5101, 20


def ref_kwargs():
    kw = ac.model_kwargs()
    return kw


def build(ref_models, args, sd, dtype):
    m = ref_models.AMDModel(args, **ref_kwargs())
    m.load_state_dict(sd)
    return m.to(dtype)


def train_run(ref_models, args, sd, dtype, kinks=None):
    """one training forward + backward of the reference -> dict of float64 results"""
    m = build(ref_models, args, sd, dtype).train()
    seen = {}

    head_forward = m.decode_head2.forward            # the reference calls .forward itself: a forward hook would not fire

    def grab(x):
        out = head_forward(x)
        out.retain_grad()
        seen["logits"] = out
        return out
    m.decode_head2.forward = grab
    if kinks is not None:
        def pre(mod, inp):
            a = inp[0].detach().abs()
            kinks.append((float(a.min() / a.max()), int((a < pc.MIN_KINK_DISTANCE * a.max()).sum())))
        for name, mod in m.decode_head.flownet.named_modules():
            if isinstance(mod, nn.LeakyReLU) and name.rsplit(".", 1)[-1].isdigit():      # the convs' activations
                mod.register_forward_pre_hook(pre)
    loss = m(ac.batch(dtype=dtype))
    loss.backward()
    named = list(m.named_parameters())
    assert all(p.grad is not None for _, p in named)
    return dict(loss=float(loss.detach()), logits=seen["logits"].detach().double().numpy(), dlogits=seen["logits"].grad.double().numpy(),
                gradnorm=ac.grad_norms(named),
                grad={n: dict(named)[n].grad.detach().double().numpy().ravel()[:256].copy() for n in ac.SAMPLED})


def eval_run(ref_models, args, sd, dtype):
    m = build(ref_models, args, sd, dtype).eval()
    with torch.no_grad():
        return m(ac.batch(dtype=dtype)).double().numpy()


def errors(r32, r64, e32, e64):
    keys = sorted(r64["gradnorm"])
    return dict(loss=ac.rel(r32["loss"], r64["loss"]), logits=ac.rel(r32["logits"], r64["logits"]), dlogits=ac.rel(r32["dlogits"], r64["dlogits"]),
                gradnorm=[ac.rel(r32["gradnorm"][k], r64["gradnorm"][k]) for k in keys],
                grad=[ac.rel(r32["grad"][n], r64["grad"][n]) for n in ac.SAMPLED], eval_masks=float(np.abs(e32 - e64).max()))


def main():
    if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "models", "amd", "amd_model.py")):
        sys.exit("usage: make_golden_amd.py <reference checkout>")
    import make_golden as mg
    mg.install_standins()
    sys.path.insert(0, sys.argv[1])
    import models as ref_models                      # noqa: the reference itself
    import rcf_amd                                   # noqa: F401  (registers the package alias for amd_cases)
    torch.set_num_threads(8)
    args = types.SimpleNamespace(checkpoints_dir="/tmp/rcf_golden_amd", object_channel=None, eval_save=False, eval_export=False)
    shapes = {k: tuple(v.shape) for k, v in ref_models.AMDModel(args, **ref_kwargs()).state_dict().items()}
    if "--scan" in sys.argv:                         # the redraw the issue asks for, as a table: SCAN seeds from SCAN_FROM on
        for seed in range(SCAN_FROM, SCAN_FROM + SCAN):
            sd, kinks = ac.state_dict(shapes, seed), []
            r64 = train_run(ref_models, args, sd, torch.float64, kinks)
            e = errors(train_run(ref_models, args, sd, torch.float32), r64, 0, 0)
            print("seed", seed, "float32 run vs float64: loss", f"{e['loss']:.1e}", "logit gradient", f"{e['dlogits']:.1e}",
                  "; pre-activations within MIN_KINK_DISTANCE:", sum(c for _, c in kinks), flush=True)
        return
    seed = ac.SEED
    sd, kinks = ac.state_dict(shapes, seed), []
    r64 = train_run(ref_models, args, sd, torch.float64, kinks)
    kink, count = min(k for k, _ in kinks), sum(c for _, c in kinks)
    r32 = train_run(ref_models, args, sd, torch.float32)
    e = errors(r32, r64, 0, 0)
    print("seed", seed, "float32 run vs float64: loss", e["loss"], "logit gradient", e["dlogits"], "; pre-activations within MIN_KINK_DISTANCE:", count)
    assert np.isfinite(r32["loss"]) and e["loss"] <= 1e-5
    e64, e32 = eval_run(ref_models, args, sd, torch.float64), eval_run(ref_models, args, sd, torch.float32)
    errs = [errors(r32, r64, e32, e64)]
    gp = torch.Generator().manual_seed(1001)         # the conditioning: the reference at weights one unit in the last place away
    sdp = {k: (v * (1 + (torch.randint(0, 2, v.shape, generator=gp).float() * 2 - 1) * 2.0 ** -23)
               if v.dtype == torch.float32 and not k.endswith(("running_mean", "running_var")) else v) for k, v in sd.items()}
    errs.append(errors(train_run(ref_models, args, sdp, torch.float32), r64, eval_run(ref_models, args, sdp, torch.float32), e64))
    worst = lambda k: np.max(np.asarray([x[k] for x in errs], dtype=np.float64), axis=0)
    keys = sorted(r64["gradnorm"])
    h, w = r64["logits"].shape[-2:]
    assert e64.shape == (ac.B, ac.M, h, w) and r64["logits"].shape == (ac.B * ac.I, ac.M, h, w)
    fx = dict(names=np.asarray(list(shapes)), shapes=ac.flat_shapes(shapes.values()), seed=seed, B=ac.B, H=ac.H, W=ac.W, M=ac.M,
              truth_logits=r64["logits"], truth_dlogits=r64["dlogits"], truth_loss=np.float64(r64["loss"]),
              gradnorm_keys=np.asarray(keys), truth_gradnorm=np.asarray([r64["gradnorm"][k] for k in keys]),
              sampled=np.asarray(ac.SAMPLED), truth_eval_masks0=e64,
              ref32_err_loss=worst("loss"), ref32_err_logits=worst("logits"), ref32_err_dlogits=worst("dlogits"),
              ref32_err_gradnorm=worst("gradnorm"), ref32_err_grad=worst("grad"), ref32_err_eval_masks=worst("eval_masks"),
              kink_distance=np.float64(kink), kink_count=np.int64(count),
              **{f"truth_grad_{i}": r64["grad"][n] for i, n in enumerate(ac.SAMPLED)})
    path = os.path.join(HERE, "amd.npz")
    np.savez_compressed(path, **fx)
    print({k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in fx.items() if k.startswith(("ref32", "kink", "truth_loss"))})
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 200 * 1024


if __name__ == "__main__":
    main()
