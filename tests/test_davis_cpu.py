"""CPU: the host side of the DAVIS J & F evaluation (rcf_amd.davis) against the reference tool's own numbers
(tests/golden/davis.json, generator make_golden_davis.py): db_statistics, the boundary radius rule, the CSV writer, and
the argument checks of rcf_davis_counts_u8 (no GPU work)."""
import ctypes
import json
import os

import numpy as np
import pytest

import rcf_amd
from rcf_amd import _lib, davis

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "davis.json")


@pytest.fixture(scope="module")
def gold():
    with open(GOLDEN) as f:
        return json.load(f)


def stats_values(seed, n, nan_frac):
    """tests/golden/make_golden_davis.py stats_values"""
    g = np.random.Generator(np.random.PCG64(seed))
    v = g.integers(0, 1001, size=n) / 1000.0
    v[g.random(n) < nan_frac] = np.nan
    return v


def test_db_statistics_bit_exact(gold):
    assert len(gold["stats"]) >= 5
    for s in gold["stats"]:
        M, R, D = davis.db_statistics(stats_values(s["seed"], s["n"], s["nan_frac"]))
        assert [float(M).hex(), float(R).hex(), float(D).hex()] == s["MRD"], s["name"]


def test_db_statistics_bins_wrap_past_255_frames():
    """the reference casts the bin edges to uint8: on 300 frames the last bin [224, 299] becomes [224, 43], an empty
    slice, so the decay is nan -- kept on purpose"""
    v = np.arange(300, dtype=np.float64) / 300
    M, R, D = davis.db_statistics(v)
    assert M == np.nanmean(v) and R == np.nanmean(v > 0.5)
    assert np.isnan(D)
    M, R, D = davis.db_statistics(v[:255])                  # below the wrap: a plain decay
    assert D == np.mean(v[0:65]) - np.mean(v[191:255])


def test_radius_rule(gold):
    assert davis.radius_for(480, 854, 0.008) == 8
    assert davis.radius_for(481, 855, 0.008) == 8
    assert davis.radius_for(480, 854, 0.004) == 4
    assert davis.radius_for(480, 854, 0.05) == 49
    assert davis.radius_for(480, 854, 0) == 0
    assert davis.radius_for(480, 854, 3) == 3
    assert davis.radius_for(1, 1, 0.008) == 1
    assert davis.radius_for(100, 300, 64) == 64
    for c in gold["cases"]:                    # the reference's expression, in float64
        th = c["bound_th"]
        want = th if th >= 1 else np.ceil(th * np.linalg.norm((c["H"], c["W"])))
        assert davis.radius_for(c["H"], c["W"], th) == want
    with pytest.raises(ValueError):
        davis.radius_for(480, 854, 2.5)        # the reference's disk(2.5) is even-sized; not reproduced
    with pytest.raises(ValueError):
        davis.radius_for(480, 854, 65)
    with pytest.raises(ValueError):
        davis.radius_for(6000, 6000, 0.008)   # 68 px


def test_csv_writer_matches_pandas_text(gold):
    """the tables of evaluation_method.py from the reference's metrics_res, as pandas' to_csv wrote them"""
    m = {k: {"M": [float.fromhex(x) for x in d["M"]], "R": [float.fromhex(x) for x in d["R"]],
             "D": [float.fromhex(x) for x in d["D"]],
             "M_per_object": {s: float.fromhex(x) for s, x in d["M_per_object"].items()}, "seq_len": d["seq_len"]}
         for k, d in gold["tree"]["unsupervised"].items()}
    g_rows, seq_rows = davis.summary_tables(m)
    assert davis.csv_text(davis.G_MEASURES, g_rows) == gold["tree"]["global_results-val.csv"]
    assert davis.csv_text(davis.SEQ_MEASURES, seq_rows) == gold["tree"]["per-sequence_results-val.csv"]


def test_csv_writer_quoting_and_nan():
    assert davis.csv_text(["a", "b"], [("x,y", float("nan")), ("z", -0.0001)]) == 'a,b\n"x,y",\nz,-0.000\n'


def test_counts_kernel_rejects_bad_arguments():
    lib = _lib.load()
    fake = ctypes.c_void_p(64)                 # never dereferenced: every call below is refused before any launch
    f = lib.rcf_davis_counts_u8
    assert f(fake, fake, None, 1, 8, 8, 65, fake, None) == -1
    assert f(fake, fake, None, 1, 8, 8, -1, fake, None) == -1
    assert f(fake, fake, None, 0, 8, 8, 8, fake, None) == -1
    assert f(fake, fake, None, 1, 0, 8, 8, fake, None) == -1
    assert f(fake, fake, None, 1, 8, 0, 8, fake, None) == -1
    assert f(None, fake, None, 1, 8, 8, 8, fake, None) == -1
    assert f(fake, None, None, 1, 8, 8, 8, fake, None) == -1
    assert f(fake, fake, None, 1, 8, 8, 8, None, None) == -1
