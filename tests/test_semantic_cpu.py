"""CPU: the host side of the semantic-constraint driver (rcf_amd.semantic, tools/semantic_constraints.py) -- flags, the export
directory and the UMI threshold per dataset, the sequence / frame listing, output paths, the refusal to overwrite, error
messages, and that the refiner's bytes are the PNG's bytes.  A stub stands in for the GPU refiner; no GPU call."""
import importlib.util
import os

import numpy as np
import pytest

import rcf_amd
from rcf_amd import _lib, maa, semantic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = maa.IMG_SIZE


def _tree(root, dataset="davis", channel=1, step=0, export_size=None):
    """two sequences (2 + 1 frames), a dot directory and a stray file; -> (pretrain_dir, data_dir, [(seq, frame)])"""
    from PIL import Image
    g = np.random.default_rng(5)
    images_dir = maa.dataset_layout(dataset, os.path.join(root, "data"))[0]
    export = os.path.join(root, semantic.EXPORT_DIR_NAMES[dataset], str(channel))
    os.makedirs(export)
    frames = [("swan", "00000"), ("swan", "00001"), ("bear", "00007")]
    for seq, f in frames:
        os.makedirs(os.path.join(images_dir, seq), exist_ok=True)
        Image.fromarray(g.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(os.path.join(images_dir, seq, f + ".jpg"))
        m = g.integers(0, 256, export_size or (H, W), dtype=np.uint8)
        Image.fromarray(np.stack([m, m, m], -1)).save(os.path.join(export, f"pred_seg_{seq}_{f}_{step:07}.png"))
    os.makedirs(os.path.join(images_dir, ".hidden"))
    open(os.path.join(images_dir, ".hidden", "00000.jpg"), "wb").close()
    open(os.path.join(images_dir, "swan", "notes.txt"), "wb").close()
    return root, os.path.join(root, "data"), sorted(frames)


def _stub(calls):
    def refiner(images, masks):
        assert images.dtype == np.float32 and images.shape[1:] == (H, W, 3) and masks.dtype == np.float32 and masks.shape[1:] == (H, W)
        assert images.shape[0] == masks.shape[0] and 0.0 <= masks.min() and masks.max() <= 1.0
        g = np.random.default_rng(100 + len(calls))
        out = g.integers(0, 256, masks.shape, dtype=np.uint8)
        calls.append((images, masks, out))
        return out
    return refiner


def test_flags_and_defaults():
    a = semantic.build_parser().parse_args(["--pretrain_dir", "exp", "--first-frames-only", "--num-channels", "5", "--object-channel",
                                            "2", "--dataset", "fbms59", "--step", "7", "--data_dir", "d", "--dino_ckpt", "c.pth",
                                            "--batch-frames", "3"])
    assert (a.pretrain_dir, a.first_frames_only, a.num_channels, a.object_channel, a.dataset) == ("exp", True, 5, 2, "fbms59")
    assert (a.step, a.data_dir, a.dino_ckpt, a.batch_frames) == (7, "d", "c.pth", 3)
    d = semantic.build_parser().parse_args([])
    assert (d.pretrain_dir, d.first_frames_only, d.num_channels, d.object_channel, d.dataset) == (None, False, 4, None, "davis")
    assert (d.step, d.data_dir, d.dino_ckpt, d.batch_frames) == (0, "data", None, 4)
    with pytest.raises(SystemExit):
        semantic.build_parser().parse_args(["--dataset", "youtube"])


def test_export_directory_and_umi_threshold_per_dataset():
    j = os.path.join
    assert semantic.export_dirs("exp", "davis", 2) == (j("exp", "saved_eval_export_trainval_ema"),
                                                       j("exp", "saved_eval_export_trainval_ema_torchcrf_ncut_torchcrf", "2"))
    assert semantic.export_dirs("exp", "stv2", 0) == (j("exp", "saved_eval_export_ema"),
                                                      j("exp", "saved_eval_export_ema_torchcrf_ncut_torchcrf", "0"))
    assert semantic.export_dirs("exp", "fbms59", 3)[0] == j("exp", "saved_eval_export_trainval_ema")
    assert semantic.UMI_TH == {"davis": None, "stv2": None, "fbms59": 10000}
    assert set(semantic.EXPORT_DIR_NAMES) == set(maa.DATASETS)
    assert semantic.save_path(j("out", "1"), "dog", "00003", 40) == j("out", "1", "pred_seg_dog_00003_0000040.png")


def test_the_reference_settings():
    assert semantic.NCUT_KW == dict(steps=10, learning_rate=0.45, weight_decay=1e-6)
    assert semantic.CRF_KW == dict(srgb=5., scomp=5., sxy=60., scomp_smooth=0., sxy_smooth=0., refine_iters=50)
    assert (semantic.CRF_SCALE_SINGLE, semantic.CRF_SCALE) == (0.7, 0.5)
    assert semantic.maa is maa                                                 # the loaders and dataset lists are reused, not copied
    assert not any(hasattr(semantic, n) for n in ("load_mask", "load_image", "load_dino", "DATASETS"))


def test_listing_takes_every_sequence_sorted_and_skips_dot_files(tmp_path):
    _, data_dir, frames = _tree(str(tmp_path))
    images_dir = maa.dataset_layout("davis", data_dir)[0]
    seqs = semantic.list_sequences(images_dir)
    assert seqs == ["bear", "swan"]                                            # neither validation sequences only, nor .hidden
    assert semantic.list_frames(images_dir, seqs) == [("bear", "00007"), ("swan", "00000"), ("swan", "00001")] == frames


@pytest.mark.parametrize("dataset,batch", [("davis", 2), ("stv2", 4), ("fbms59", 1)])
def test_main_writes_the_refiners_bytes_as_mode_L_pngs(tmp_path, capsys, dataset, batch):
    from PIL import Image
    pretrain, data_dir, frames = _tree(str(tmp_path), dataset, channel=2, step=3, export_size=(240, 427))
    calls = []
    written = semantic.main(["--pretrain_dir", pretrain, "--data_dir", data_dir, "--dataset", dataset, "--object-channel", "2",
                             "--step", "3", "--batch-frames", str(batch), "--first-frames-only"], refiner=_stub(calls))
    out = capsys.readouterr().out
    save_dir = os.path.join(pretrain, semantic.EXPORT_DIR_NAMES[dataset] + "_torchcrf_ncut_torchcrf", "2")
    assert f"Dataset: {dataset}" in out and "Found 2 sequences: ['bear', 'swan']" in out and f"Start refinement: {save_dir}" in out
    assert written == [os.path.join(save_dir, f"pred_seg_{s}_{f}_0000003.png") for s, f in frames]     # --first-frames-only: unused
    assert sorted(os.listdir(save_dir)) == sorted(os.path.basename(p) for p in written)
    assert [c[1].shape[0] for c in calls] == [len(frames[i:i + batch]) for i in range(0, len(frames), batch)]
    want = np.concatenate([c[2] for c in calls])
    for p, u8 in zip(written, want):
        im = Image.open(p)
        assert im.mode == "L" and im.size == (W, H)
        assert np.array_equal(np.asarray(im), u8)
    # what the refiner was given: the frame, and the export resized to 480 x 854 through maa.load_mask
    got_masks = np.concatenate([c[1] for c in calls])
    got_images = np.concatenate([c[0] for c in calls])
    images_dir = maa.dataset_layout(dataset, data_dir)[0]
    for k, (s, f) in enumerate(frames):
        assert np.array_equal(got_masks[k], maa.load_mask(os.path.join(pretrain, semantic.EXPORT_DIR_NAMES[dataset]), s, f, 2, 3))
        assert np.array_equal(got_images[k], maa.load_image(images_dir, s, f))


def test_refuses_to_overwrite(tmp_path):
    pretrain, data_dir, frames = _tree(str(tmp_path))
    argv = ["--pretrain_dir", pretrain, "--data_dir", data_dir, "--object-channel", "1"]
    calls = []
    written = semantic.main(argv, refiner=_stub(calls))
    before = [open(p, "rb").read() for p in written]
    n = len(calls)
    with pytest.raises(FileExistsError, match="pred_seg_bear_00007_0000000.png"):
        semantic.main(argv, refiner=_stub(calls))
    assert len(calls) == n and [open(p, "rb").read() for p in written] == before      # nothing refined, nothing rewritten
    os.remove(written[0])                                                            # one file left: still refused
    with pytest.raises(FileExistsError, match="pred_seg_swan_00000_0000000.png"):
        semantic.main(argv, refiner=_stub(calls))
    assert not os.path.exists(written[0])


def test_missing_object_channel_and_checkpoint_are_clear_errors(tmp_path):
    pretrain, data_dir, _ = _tree(str(tmp_path))
    with pytest.raises(ValueError, match="--object-channel"):
        semantic.main(["--pretrain_dir", pretrain, "--data_dir", data_dir], refiner=_stub([]))
    assert not os.path.exists(os.path.join(pretrain, "saved_eval_export_trainval_ema_torchcrf_ncut_torchcrf"))     # no `None` directory
    with pytest.raises(ValueError, match="--dino_ckpt"):
        semantic.main(["--pretrain_dir", pretrain, "--data_dir", data_dir, "--object-channel", "1"])


def test_missing_export_is_named(tmp_path):
    pretrain, data_dir, _ = _tree(str(tmp_path), channel=1)
    with pytest.raises(FileNotFoundError, match="pred_seg_bear_00007_0000000.png"):
        semantic.main(["--pretrain_dir", pretrain, "--data_dir", data_dir, "--object-channel", "3"], refiner=_stub([]))


def test_tool_wrapper(tmp_path, capsys):
    spec = importlib.util.spec_from_file_location("semantic_tool", os.path.join(ROOT, "tools", "semantic_constraints.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    pretrain, data_dir, frames = _tree(str(tmp_path))
    tool.cli(["--pretrain_dir", pretrain, "--data_dir", data_dir, "--object-channel", "1"], refiner=_stub([]))
    assert f"wrote {len(frames)} masks" in capsys.readouterr().out


def test_new_entry_points_reject_bad_arguments():
    lib = _lib.load()
    assert not _lib.missing_symbols()
    one = 16                                                                   # a non-null, 16-byte aligned stand-in pointer
    assert [lib.rcf_affinity_pack_words(n) for n in (0, 1, 33, 64, 65, 96, 101, 6420)] == [0, 2, 2, 2, 4, 4, 4, 202]
    pack = lambda g, pitch, n, frames, b, d: lib.rcf_affinity_pack_f32(g, pitch, n, frames, 0.2, b, d, None)
    assert pack(None, 8, 8, 1, one, one) == -1 and pack(one, 8, 8, 1, None, one) == -1 and pack(one, 8, 8, 1, one, None) == -1
    assert pack(one, 4, 8, 1, one, one) == -1 and pack(one, 8, 0, 1, one, one) == -1 and pack(one, 8, 8, 0, one, one) == -1
    assert pack(one, 8, 8, 1, 12, one) == -1                                   # bits not 8-byte aligned
    nmax = 16384                                                               # RCF_NCUT_PACKED_MAX_N of include/rcf_hip.h
    assert nmax >= 60 * 107
    wsb = lib.rcf_ncut_refine_packed_workspace_bytes
    assert wsb(1, nmax + 1) == 0 and wsb(0, 96) == 0 and wsb(1, 0) == 0
    assert wsb(1, 6420) == 6420 * 16 and wsb(4, 6420) == 4 * wsb(1, 6420) and wsb(1, nmax) == nmax * 16
    ref = lambda b, d, n, frames, x, steps, ws, nb: lib.rcf_ncut_refine_packed_f32(b, d, n, frames, 1e-5, x, steps, 0.45, 1e-6, None, ws, nb, None)
    big = 1 << 30
    assert ref(None, one, 96, 1, one, 10, one, big) == -1 and ref(one, None, 96, 1, one, 10, one, big) == -1
    assert ref(one, one, 96, 1, None, 10, one, big) == -1 and ref(one, one, 96, 1, one, 10, None, big) == -1
    assert ref(one, one, 96, 1, one, -1, one, big) == -1 and ref(one, one, 96, 0, one, 10, one, big) == -1
    assert ref(one, one, nmax + 1, 1, one, 10, one, big) == -1                 # above the stated maximum: an error, no launch
    assert ref(one, one, 96, 1, one, 10, one, 96 * 16 - 1) == -2               # workspace too small
    merge = lambda a, b, frames, npix, o, c: lib.rcf_mask_merge_u8(a, b, frames, npix, -1, o, c, None)
    assert merge(None, one, 1, 8, one, one) == -1 and merge(one, None, 1, 8, one, one) == -1
    assert merge(one, one, 1, 8, None, one) == -1 and merge(one, one, 1, 8, one, None) == -1
    assert merge(one, one, 0, 8, one, one) == -1 and merge(one, one, 1, 0, one, one) == -1
