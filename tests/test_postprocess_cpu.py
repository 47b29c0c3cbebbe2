"""CPU: the host side of the CRF post-processing (rcf_amd.postprocess, tools/crf_postprocess.py, offline.unary_table) -- the
unary table against a restatement of the reference's steps for every (frame maximum, pixel value) pair, the new entry point's
argument checks, and the driver with a stub in place of the GPU refiner: flags, listing, the save-path rule, skipping, error
messages, that the refiner gets the raw resized export and that its bytes are the PNG's bytes.  No GPU call."""
import importlib.util
import os
import shutil

import numpy as np
import pytest

import rcf_amd
from rcf_amd import _lib, offline, postprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 480, 854
FRAMES = [("bear", "00007"), ("swan", "00000"), ("swan", "00001")]          # sorted, as `--seq *` lists them


# ---------------------------------------------------------------------------------- the table
def reference_prescale(mask):
    """tools/pydenseCRF/crf.py:169"""
    return (mask / 0.8).clip(min=0, max=255).astype(np.uint8)


def reference_unary(mask, gk=0.1):
    """tools/pydenseCRF/crf.py:60-69 -> float32 [2, H*W]"""
    try:
        from scipy.ndimage import gaussian_filter
        U = gaussian_filter(mask, sigma=gk)
    except ImportError:                      # sigma 0.1: scipy's radius is int(4 * 0.1 + 0.5) = 0, a 1-tap kernel
        U = mask
    U = U / (np.amax(U) + 1e-8)
    U = np.clip(U, 1e-6, 1.0 - 1e-6)
    UU = np.zeros((2, mask.shape[0], mask.shape[1]))
    UU[1, :, :] = U
    UU[0, :, :] = 1.0 - U
    UU = -np.log(UU)
    UU = np.float32(UU)
    return UU.reshape((2, -1))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("prescale", [False, True])
def test_table_equals_the_reference_steps_for_every_pair(prescale):
    table = offline.unary_table(prescale)
    assert table.dtype == np.float32 and table.shape == (256, 256, 2) and np.isfinite(table).all()
    values = np.arange(256, dtype=np.uint8)
    # (a) through the reference's function: a frame that holds every value up to its maximum a
    for a in range(256):
        frame = values[None, :a + 1]
        want = reference_unary(reference_prescale(frame) if prescale else frame)
        assert np.array_equal(bits(table[a, :a + 1].T), bits(want)), a
    # (b) every pair, v > a included (never met in a frame: the same expressions with a as the maximum)
    s = reference_prescale(values) if prescale else values
    for a in range(256):
        U = np.clip(s / (s[a] + 1e-8), 1e-6, 1.0 - 1e-6)
        want = np.float32(-np.log(np.stack([1.0 - U, U], -1)))
        assert np.array_equal(bits(table[a]), bits(want)), a
    # and the function the existing route calls
    g = np.random.default_rng(3)
    for top in (255, 203, 17, 0):
        m = g.integers(0, top + 1, (5, 7), dtype=np.uint8)
        m.flat[3] = top
        ms = reference_prescale(m) if prescale else m
        assert np.array_equal(bits(table[top][m.reshape(-1)]), bits(offline._unary_from_u8(ms, 0.1)))


def test_table_landmarks():
    t = offline.unary_table(False)
    assert np.array_equal(t[0, 0], np.float32([1.0000005e-06, 13.815511]))                  # the all-zero frame
    hi = 1.0 - 1e-6                                                                         # 255 / (255 + 1e-8) clips to it
    assert np.array_equal(t[255, 255], np.float32([-np.log(1.0 - hi), -np.log(hi)]))
    p = offline.prescale_u8(np.arange(256, dtype=np.uint8))
    assert p.dtype == np.uint8 and (p[255], p[204], p[4], p[0]) == (255, 255, 5, 0) and (np.diff(p.astype(int)) >= 0).all()
    assert np.array_equal(p, reference_prescale(np.arange(256, dtype=np.uint8)))
    tp = offline.unary_table(True)
    assert np.array_equal(tp[204, 204], t[255, 255]) and np.array_equal(tp[100, 4], t[p[100], 5])


def test_new_entry_point_rejects_bad_arguments():
    lib = _lib.load()
    assert not _lib.missing_symbols()
    one = 16                                                                   # a non-null, 16-byte aligned stand-in pointer
    un = lambda m, frames, npix, t, u, s: lib.rcf_crf_unary_lut_u8(m, frames, npix, t, u, s, None)
    assert un(None, 1, 8, one, one, one) == -1 and un(one, 1, 8, None, one, one) == -1
    assert un(one, 1, 8, one, None, one) == -1 and un(one, 1, 8, one, one, None) == -1
    assert un(one, 0, 8, one, one, one) == -1 and un(one, -1, 8, one, one, one) == -1
    assert un(one, 1, 0, one, one, one) == -1 and un(one, 1, -5, one, one, one) == -1
    assert un(one, 1, 8, one, 12, one) == -1                                   # unary not 8-byte aligned


# ---------------------------------------------------------------------------------- the driver
def _stub(calls):
    def refiner(images, masks):
        assert images.dtype == np.uint8 and images.shape[1:] == (H, W, 3) and masks.dtype == np.uint8 and masks.shape[1:] == (H, W)
        assert images.shape[0] == masks.shape[0]
        out = masks ^ images[..., 1]                                           # any bytes; a function of the frame alone
        calls.append((images, masks, out))
        return out
    return refiner


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """images/{bear,swan}/*.jpg at 854 x 480; export/: the three masks as 427 x 240 RGB PNGs whose channels differ;
    chan/0/: the swan masks only"""
    from PIL import Image
    root = str(tmp_path_factory.mktemp("postprocess"))
    g = np.random.default_rng(11)
    os.makedirs(os.path.join(root, "export"))
    os.makedirs(os.path.join(root, "chan", "0"))
    for seq, f in FRAMES:
        os.makedirs(os.path.join(root, "images", seq), exist_ok=True)
        Image.fromarray(g.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(os.path.join(root, "images", seq, f + ".jpg"))
        name = f"pred_seg_{seq}_{f}_0000040.png"
        Image.fromarray(g.integers(0, 256, (240, 427, 3), dtype=np.uint8)).save(os.path.join(root, "export", name))
        if seq == "swan":
            shutil.copy(os.path.join(root, "export", name), os.path.join(root, "chan", "0", name))
    open(os.path.join(root, "images", "swan", "notes.txt"), "wb").close()
    return root


def _argv(tree, ann="export", *more):
    return ["--input", os.path.join(tree, "images"), "--output", "unused", "--annotation-dir", os.path.join(tree, ann),
            "--step", "40", *more]


def _expected_inputs(tree, ann, seq, f):
    from PIL import Image
    img = np.asarray(Image.open(os.path.join(tree, "images", seq, f + ".jpg")))
    m = np.asarray(Image.open(os.path.join(tree, ann, f"pred_seg_{seq}_{f}_0000040.png")).resize((W, H)))
    assert m.shape == (H, W, 3) and not np.array_equal(m[..., 0], m[..., 1])
    return img, m[..., 0]                                                      # the raw resized export: not divided by 0.8


def test_flags_and_defaults():
    a = postprocess.build_parser().parse_args(["--input", "in", "--output", "out", "--annotation-dir", "ann", "--allow_skip", "--step",
                                               "4320", "--seq", "dog", "--batch-frames", "3", "--workers", "2"])
    assert (a.input, a.output, a.annotation_dir, a.allow_skip, a.step, a.seq) == ("in", "out", "ann", True, 4320, ["dog"])
    assert (a.batch_frames, a.workers) == (3, 2)
    d = postprocess.build_parser().parse_args([])
    assert (d.input, d.output, d.annotation_dir, d.allow_skip, d.step, d.seq, d.batch_frames, d.workers) == \
        (None, None, None, False, 0, ["*"], 8, 8)
    assert postprocess.build_parser().parse_args(["--seq", "dog", "goat"]).seq == ["dog", "goat"]
    assert postprocess.MAX_WORKERS == 16
    assert postprocess.REFINE_KW == dict(gk=0.1, sxy=60.0, srgb=5.0, compat=5.0, iters=50)


def test_save_path_rule():
    j = os.path.join
    assert postprocess.save_dir_of(j("saved", "saved_eval_export")) == j("saved", "saved_eval_export_crf")
    assert postprocess.save_dir_of(j("saved", "saved_eval_export") + os.sep) == j("saved", "saved_eval_export_crf")
    assert postprocess.save_dir_of(j("saved", "export_ema", "2")) == j(os.path.abspath("saved"), "export_ema_crf", "2")
    assert postprocess.save_dir_of(j("saved", "export_ema", "12")) == j("saved", "export_ema", "12_crf")
    assert postprocess.annotation_path("ann", j("in", "dog", "00003.jpg"), 40) == j("ann", "pred_seg_dog_00003_0000040.png")


@pytest.mark.parametrize("seq,batch,frames", [
    (None, 2, FRAMES),
    (["swan"], 8, FRAMES[1:]),
    (["swan", "bear"], 2, FRAMES[1:] + FRAMES[:1]),                            # patterns in the order given, each sorted
    (["s*", "swan", "b*"], 1, FRAMES[1:] + FRAMES[:1]),                        # a frame two patterns match is taken once
])
def test_main_writes_the_refiners_bytes_as_mode_L_pngs(tree, capsys, seq, batch, frames):
    from PIL import Image
    save_dir = os.path.join(tree, "export_crf")
    shutil.rmtree(save_dir, ignore_errors=True)
    calls = []
    argv = _argv(tree, "export", "--batch-frames", str(batch)) + (["--seq"] + seq if seq else [])
    written = postprocess.main(argv, refiner=_stub(calls))
    out = capsys.readouterr().out
    assert f"Annotation dir: {os.path.join(tree, 'export')}" in out and f"len(paths): {len(frames)}" in out
    assert f"seq: {' '.join(seq or ['*'])}\n" in out and "Skipped" not in out
    assert written == [os.path.join(save_dir, f"pred_seg_{s}_{f}_0000040.png") for s, f in frames]
    assert sorted(os.listdir(save_dir)) == sorted(os.path.basename(p) for p in written)
    assert [c[1].shape[0] for c in calls] == [len(frames[i:i + batch]) for i in range(0, len(frames), batch)]
    got_images, got_masks, want = (np.concatenate([c[k] for c in calls]) for k in range(3))
    for k, (p, (s, f)) in enumerate(zip(written, frames)):
        im = Image.open(p)
        assert im.mode == "L" and im.size == (W, H)
        assert np.array_equal(np.asarray(im), want[k])                         # the stub's bytes are the PNG's bytes
        img, raw = _expected_inputs(tree, "export", s, f)
        assert np.array_equal(got_images[k], img) and np.array_equal(got_masks[k], raw)
    before = [open(p, "rb").read() for p in written]                           # existing files are overwritten, as in the reference
    assert postprocess.main(argv, refiner=lambda images, masks: np.full(masks.shape, 255, np.uint8)) == written
    assert all(open(p, "rb").read() != b for p, b in zip(written, before))
    assert all(np.asarray(Image.open(p)).min() == 255 for p in written)


def test_channel_directory_and_skipping(tree, capsys):
    from PIL import Image
    save_dir = os.path.join(tree, "chan_crf", "0")                             # a one-character directory: its parent gets the suffix
    shutil.rmtree(os.path.join(tree, "chan_crf"), ignore_errors=True)
    calls = []
    with pytest.raises(FileNotFoundError, match="pred_seg_bear_00007_0000040.png"):
        postprocess.main(_argv(tree, os.path.join("chan", "0")), refiner=_stub(calls))
    assert not calls and not os.path.exists(os.path.join(tree, "chan_crf")) and not os.path.exists(os.path.join(tree, "chan", "0_crf"))
    written = postprocess.main(_argv(tree, os.path.join("chan", "0"), "--allow_skip"), refiner=_stub(calls))
    out = capsys.readouterr().out
    assert "len(paths): 3" in out
    assert "Skipped 1 frames (this number does not include the ones in training set if val_seq is True)" in out
    assert written == [os.path.join(save_dir, f"pred_seg_swan_{f}_0000040.png") for f in ("00000", "00001")]
    assert len(calls) == 1 and calls[0][1].shape[0] == 2
    for p, u8 in zip(written, calls[0][2]):
        assert np.array_equal(np.asarray(Image.open(p)), u8)
    assert sorted(os.listdir(os.path.join(tree, "chan"))) == ["0"]                # nothing beside the export itself


def test_files_do_not_depend_on_the_workers(tree):
    runs = []
    for workers in ("1", "4", "64"):
        shutil.rmtree(os.path.join(tree, "export_crf"), ignore_errors=True)
        written = postprocess.main(_argv(tree, "export", "--batch-frames", "2", "--workers", workers), refiner=_stub([]))
        runs.append([(p, open(p, "rb").read()) for p in written])
    assert len(runs[0]) == 3 and runs[0] == runs[1] == runs[2]


def test_errors_name_the_file(tmp_path):
    from PIL import Image
    root = str(tmp_path)
    os.makedirs(os.path.join(root, "images", "dog"))
    os.makedirs(os.path.join(root, "export"))
    Image.fromarray(np.zeros((80, 100, 3), np.uint8)).save(os.path.join(root, "images", "dog", "00000.jpg"))
    Image.fromarray(np.zeros((40, 50), np.uint8)).save(os.path.join(root, "export", "pred_seg_dog_00000_0000000.png"))
    argv = ["--input", os.path.join(root, "images"), "--annotation-dir", os.path.join(root, "export")]
    with pytest.raises(ValueError, match=r"dog.00000\.jpg.*854 x 480.*\(80, 100, 3\)"):
        postprocess.main(argv, refiner=_stub([]))
    Image.fromarray(np.zeros((H, W), np.uint8)).save(os.path.join(root, "images", "dog", "00000.jpg"))     # the size, one channel
    with pytest.raises(ValueError, match=r"dog.00000\.jpg.*3-channel"):
        postprocess.main(argv, refiner=_stub([]))
    with pytest.raises(ValueError, match="--annotation-dir"):
        postprocess.main(["--input", os.path.join(root, "images")], refiner=_stub([]))
    with pytest.raises(FileNotFoundError, match="no_such_dir"):
        postprocess.main(["--input", os.path.join(root, "images"), "--annotation-dir", os.path.join(root, "no_such_dir")], refiner=_stub([]))


def test_tool_wrapper(tree, capsys):
    spec = importlib.util.spec_from_file_location("crf_postprocess_tool", os.path.join(ROOT, "tools", "crf_postprocess.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    tool.cli(_argv(tree, "export", "--seq", "swan"), refiner=_stub([]))
    assert "wrote 2 masks" in capsys.readouterr().out
