"""CPU: the profiling family of a conv launch (bench.py FAMILIES_F32 / FAMILIES_BF16) is what the library's own plan says will
run (rcf_conv_plan_of), mapped to a name by ops.conv_family.  tests/golden/conv_families.json holds, for every shape of
test_conv_plan_cpu.cases(), the family the Python rules that ops.py carried before (its own copy of the C tile rules, plus the
rcf_conv_kernel_of relabel) gave to each (direction, kind, region) -- tests/golden/README.md says how it was recorded.  On the
`model ...` rows, the ones bench.py reports, conv_family must reproduce it exactly.

    python tests/test_conv_family_cpu.py --record        # rewrites the table from the library built in this tree
"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import rcf_amd  # noqa: E402,F401
from rcf_amd import _lib, ops  # noqa: E402
from test_conv_plan_cpu import cases  # noqa: E402

TABLE = os.path.join(ROOT, "tests", "golden", "conv_families.json")

# the kinds the wrappers of ops.py pass per direction
KINDS = {"fwd": ("f32", "planes", "h16"), "dgrad": ("f32", "planes", "h16"), "wgrad": ("f32", "h2", "planes", "h16")}
COLUMNS = [(d, k, r) for d in ("fwd", "dgrad", "wgrad") for k in KINDS[d] for r in range(3)]

_DUMMY = ctypes.create_string_buffer(256)                     # never read: the queries launch nothing


def shape_of(f, size, direction, kind):
    """the rcf_conv_shape a wrapper of that kind builds in a training step: operand ranges and prepared weights on the fp32
    forward / data gradient, ranges alone on the "h2" weight gradient, none on the plain fp32 weight gradient and the 16-bit path"""
    ptr = (ctypes.addressof(_DUMMY) + 15) & ~15
    flags = 0
    if kind == "planes":
        flags = {"fwd": _lib.CONV_X_PLANES, "dgrad": _lib.CONV_DY_PLANES, "wgrad": _lib.CONV_X_PLANES | _lib.CONV_DY_PLANES}[direction]
    if kind == "h16" or (direction == "wgrad" and kind == "f32"):
        p = [None] * 8
    elif direction == "wgrad":
        p = [ptr, None, ptr] + [None] * 5                      # amax_x, amax_dy
    else:
        p = [ptr] * 7 + [None]
    return _lib.ConvShape(*f, *p, flags, ctypes.sizeof(_lib.ConvShape) if size is None else size)


def regions_of(f, drawn, direction):
    """[None, a rectangle, a frame] in the coordinates of the direction's GEMM rows (test_conv_plan_cpu.plan_row's regions)"""
    H, W = (f[1], f[2]) if direction == "dgrad" else (f[4], f[5])
    if H < 4 or W < 4:
        return [None, None, None]
    rect = tuple(drawn) if (drawn is not None and direction != "dgrad") else (1, 1, H - 2, W - 2, 0)
    return [None, rect, (0, 0, H, W, 1)]


def families(family_of):
    """{label: [family_of(shape, direction, kind, region) per COLUMNS entry; None where the library refuses the launch]}"""
    out = {}
    for label, f, size, drawn in cases():
        row = []
        for d, k, r in COLUMNS:
            region = regions_of(f, drawn, d)[r]
            if r and region is None:
                row.append(None)
                continue
            try:
                row.append(family_of(shape_of(f, size, d, k), d, k, region))
            except _lib.RcfHipError:
                row.append(None)
        out[label] = row
    return out


# (model row, column) pairs the library refuses -- 4 stem channels or 4 classes on the 16-bit path, pair planes on channel counts
# their kernels do not take, a region on the stem's weight gradient: launches the model never issues.  Pinned, so that a planner
# that starts refusing a launch of the model cannot hide behind "no bracket is filed".
REFUSED_MODEL = 138


def test_conv_families_match_the_recorded_table():
    """Every row -- `model`, `fuzz` and `abi` alike: when the table was recorded, the old Python rules named the kernel the launch
    ladders of that commit took on each of them, so no row needs an exception."""
    want = json.load(open(TABLE))
    got = families(ops.conv_family)
    assert sorted(got) == sorted(want), "the set of shapes changed: record the table again (module docstring) and say why"
    moved = [f"{label} {COLUMNS[i]}: {old} -> {new}" for label, row in want.items()
             for i, (old, new) in enumerate(zip(row, got[label])) if new is not None and new != old]   # None: refused, no bracket is ever filed
    assert not moved, f"{len(moved)} families moved, e.g. " + "; ".join(moved[:5])
    model = [new for label, row in got.items() if label.startswith("model") for new in row]
    assert model.count(None) == REFUSED_MODEL
    # the table discriminates: every family of both steps occurs on the model rows
    assert set(model) - {None} == set(ops.CONV_FAMILIES), sorted(set(ops.CONV_FAMILIES) ^ (set(model) - {None}))


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], __doc__
    with open(TABLE, "w") as fh:
        fh.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in families(ops.conv_family).items()) + "\n}\n")
    print("wrote", TABLE)
