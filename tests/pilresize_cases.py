"""Shapes, data and the Pillow reference shared by test_pilresize_cpu.py and test_pilresize_gpu.py (rcf_amd.pilresize).

A case is (h, w, H, W): source and target size.  The reference of a case is Pillow itself, computed once per
(case, filter, kind) and cached."""
import functools

import numpy as np

FILTERS = ("bicubic", "bilinear", "box")
KINDS = ("bytes", "mask", "cluster")        # random bytes, 0 / 255 masks, values clustered at 88...91 (around the tool's threshold)

FIXED = [(1, 1, 5, 7), (33, 17, 1, 1), (2, 3, 70, 130), (97, 65, 33, 201), (300, 500, 13, 17), (5, 900, 4, 1),
         (40, 60, 40, 91), (40, 60, 23, 60), (31, 47, 31, 47), (1, 9, 1, 30), (9, 1, 30, 1), (64, 64, 65, 63)]


def _seeded(n, seed=20):
    g = np.random.Generator(np.random.PCG64(seed))
    out = []
    for _ in range(n):
        h, w = (int(v) for v in g.integers(1, 120, size=2))
        H, W = (int(v) for v in g.integers(1, 160, size=2))
        out.append((h, w, H, W))
    return out


CASES = FIXED + _seeded(28)                 # 40 cases


def pil_filter(name):
    from PIL import Image
    return {"bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR, "box": Image.BOX}[name]


def frames(h, w, kind, seed, N=2):
    """u8 [N,h,w,3]: the three channels differ, so reading another one than channel 0 shows"""
    g = np.random.Generator(np.random.PCG64(1000 * seed + KINDS.index(kind)))
    if kind == "bytes":
        return g.integers(0, 256, size=(N, h, w, 3), dtype=np.uint8)
    if kind == "mask":
        return (g.integers(0, 2, size=(N, h, w, 3), dtype=np.uint8) * 255).astype(np.uint8)
    return g.integers(88, 92, size=(N, h, w, 3), dtype=np.uint8)


def pillow_resize(a, size, filter="bicubic"):
    """a u8 [N,h,w] (mode L) or [N,h,w,3] (mode RGB) -> Pillow's resize of every frame, stacked"""
    from PIL import Image
    H, W = size
    return np.stack([np.array(Image.fromarray(f).resize((W, H), pil_filter(filter))) for f in a])


@functools.lru_cache(maxsize=None)
def case_data(i, kind, N=2):
    a = frames(*CASES[i][:2], kind, seed=i, N=N)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def case_ref(i, filter, kind, N=2):
    """Pillow on the RGB frames of case i: u8 [N,H,W,3], read-only"""
    r = pillow_resize(case_data(i, kind, N), CASES[i][2:], filter)
    r.setflags(write=False)
    return r


def bicubic_taps(in_size, out_size):
    """Pillow's ksize for the bicubic filter: ceil(2 max(scale, 1)) * 2 + 1"""
    scale = max(in_size / out_size, 1.0)
    return int(np.ceil(2.0 * scale)) * 2 + 1


def refused_calls(fake):
    """argument lists rcf_pil_resample_u8 must refuse before any launch; `fake` stands for any non-null pointer"""
    #        src   N  h  w  ps kx    bx    ksx ky    by    ksy H  W  dst   gt    pm  counts
    good = [fake, 1, 8, 8, 1, fake, fake, 5, fake, fake, 5, 6, 6, fake, fake, 90, fake]
    bad = []

    def with_(**kw):
        names = ["src", "N", "h", "w", "ps", "kx", "bx", "ksx", "ky", "by", "ksy", "H", "W", "dst", "gt", "pm", "counts"]
        a = list(good)
        for n, v in kw.items():
            a[names.index(n)] = v
        bad.append((kw, a + [None]))
    with_(src=None)
    for n in ("N", "h", "w", "H", "W"):
        with_(**{n: 0})
        with_(**{n: -3})
    for ps in (0, 2, 4, -1):
        with_(ps=ps)
    with_(dst=None, counts=None)
    with_(gt=None)                              # counts without a mask
    with_(pm=-1)
    with_(pm=257)
    with_(bx=None)
    with_(by=None)
    with_(ksx=0)
    with_(ksy=0)
    with_(ksy=257)                              # RCF_PIL_MAX_TAPS + 1
    with_(kx=None)                              # no horizontal table, but W != w
    with_(ky=None)                              # no vertical table, but H != h
    return good + [None], bad
