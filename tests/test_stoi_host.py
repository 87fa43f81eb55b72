"""CPU: the STOI oracle (tests/stoi_ref.py) against the algorithm's anchors, and the host side of sehip.metric.STOI: the header, the
exported symbols, the resampling table and every refusal that comes before a launch.  `from sehip.metric import STOI` and the
sehip_stoi_* symbols do not exist before this feature."""
import os
import re

import numpy as np
import pytest

import stoi_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ("sehip_stoi_out_len", "sehip_stoi_frames", "sehip_stoi_segment_blocks", "sehip_stoi_resample", "sehip_stoi_levels",
         "sehip_stoi_select", "sehip_stoi_bands", "sehip_stoi_segments")


signal = R.am_signal


def test_band_list_and_filter_anchors():
    assert R.thirdoct(10000, 512, 15, 150) == R.BANDS
    assert R.BANDS[0] == (7, 9) and R.BANDS[-1] == (174, 219)
    assert all(a[1] == b[0] for a, b in zip(R.BANDS[:-1], R.BANDS[1:]))
    anchors = {16000: (5, 8, 290), 48000: (5, 24, 870), 44100: (100, 441, 15973), 8000: (5, 4, 182)}
    for sr, want in anchors.items():
        p, q, L, w = R.resample_filter(sr)
        assert (p, q, L) == want and len(w) == 2 * L + 1 and abs(np.sum(w) - 1) < 1e-12


@pytest.mark.parametrize("sr,n", [(16000, 1003), (48000, 2001), (44100, 1777), (8000, 999)])
def test_resample_is_resample_poly(sr, n):
    signal_module = pytest.importorskip("scipy.signal")
    x = signal(n, sr, seed=sr)
    p, q, _, w = R.resample_filter(sr)
    want = signal_module.resample_poly(x, p, q, window=w)
    got = R.resample(x, sr)
    assert got.shape == want.shape == (R.out_len(n, sr),)
    assert np.abs(got - want).max() < 1e-12


@pytest.mark.parametrize("extended", [False, True])
def test_identical_signals_give_one(extended):
    x = signal(8000, 16000, seed=1)
    assert abs(R.stoi(x, x, 16000, extended) - 1) < 1e-9
    both = np.stack([x, signal(8000, 16000, seed=6)]).reshape(2, 1, 8000)
    assert abs(R.STOI(both, both, 16000, extended) - 1) < 1e-9


def test_frame_count_threshold():
    x = signal(4095, 10000, seed=2)
    st = R.stoi_steps(x, x, 10000)
    assert st["T"] == 29 and st["d"] == 1e-5
    x = signal(4223, 10000, seed=2)
    st = R.stoi_steps(x, x, 10000)
    assert st["T"] == 30 and R.segments(st["x_tob"]).shape == (1, 15, 30)
    assert abs(st["d"] - 1) < 1e-9


def test_zero_row_keeps_every_frame_and_gives_zero():
    z = np.zeros(5000)
    st = R.stoi_steps(z, signal(5000, 10000, seed=3), 10000)
    assert st["mask"].all() and len(st["src"]) == R.frame_count(5000)
    assert st["d"] == 0.0
    assert R.stoi(z, z, 10000, extended=True) == 0.0


def test_float32_restatement_is_close():
    x = signal(8000, 16000, seed=4)
    y = x + 0.05 * np.random.RandomState(5).randn(8000)
    for ext in (False, True):
        assert abs(R.stoi(x, y, 16000, ext, np.float32) - R.stoi(x, y, 16000, ext)) < 1e-5


def test_header_declares_every_entry_point():
    text = open(os.path.join(ROOT, "include", "sehip.h")).read()
    names = set(re.findall(r"\b(sehip_stoi_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert names == set(ENTRY)


def test_library_and_package_export_the_metric():
    import sehip
    from sehip import _lib
    from sehip.metric import STOI, stoi_rows  # noqa: F401
    assert sehip.STOI is STOI
    lib = _lib.lib()
    for name in ENTRY:
        assert hasattr(lib, name), name
        assert name in _lib._PROTOS


def test_host_helpers():
    from sehip import _lib
    lib = _lib.lib()
    for sr, n in [(16000, 1003), (48000, 2001), (44100, 1777), (8000, 999), (10000, 300)]:
        assert lib.sehip_stoi_out_len(n, sr) == R.out_len(n, sr)
    assert lib.sehip_stoi_out_len(-1, 16000) == -1 and lib.sehip_stoi_out_len(100, 0) == -1
    assert [lib.sehip_stoi_frames(n) for n in (255, 256, 383, 384, 4095, 4223)] == [0, 1, 1, 2, 30, 31]
    assert lib.sehip_stoi_segment_blocks(10, 0) == 1 and lib.sehip_stoi_segment_blocks(47, 0) == 2
    assert lib.sehip_stoi_segment_blocks(47, 1) == 3


def test_errors_are_reported_not_thrown():
    from sehip import _lib
    lib = _lib.lib()
    one = 1  # (a non-null pointer value that is never dereferenced: validation comes before any HIP call)
    assert lib.sehip_stoi_resample(None, None, 0, 100, None, 5, 8, 290, None, None) != 0
    assert b"rows=0" in lib.sehip_last_error()
    assert lib.sehip_stoi_resample(None, None, 1, 100, None, 129, 8, 290, None, None) != 0
    assert b"outside p <= 128" in lib.sehip_last_error()
    assert lib.sehip_stoi_resample(None, None, 1, 100, None, 5, 1025, 290, None, None) != 0
    assert b"q <= 1024" in lib.sehip_last_error()
    assert lib.sehip_stoi_resample(None, None, 1, 100, None, 10, 16, 290, None, None) != 0
    assert b"not reduced" in lib.sehip_last_error()
    assert lib.sehip_stoi_resample(None, None, 1, 100, None, 5, 8, 290, None, None) != 0
    assert b"null pointer" in lib.sehip_last_error()
    assert lib.sehip_stoi_levels(one, 1, 255, one, None) != 0
    assert b"len=255" in lib.sehip_last_error()
    assert lib.sehip_stoi_levels(None, 1, 256, None, None) != 0
    assert b"null pointer" in lib.sehip_last_error()
    assert lib.sehip_stoi_select(None, 1, 0, None, None, None) != 0
    assert b"F=0" in lib.sehip_last_error()
    assert lib.sehip_stoi_bands(None, None, 40000, 4000, None, None, None, None) != 0
    assert b"rows=40000" in lib.sehip_last_error()
    assert lib.sehip_stoi_segments(one, one, 1, 40, 2, one, one, one, None) != 0
    assert b"extended=2" in lib.sehip_last_error()
    with pytest.raises(_lib.SehipError):
        _lib.call("sehip_stoi_segments", None, None, 1, 40, 0, None, None, None, None)


def test_python_refusals_come_before_any_launch():
    import torch
    from sehip import SehipError
    from sehip import metric
    with pytest.raises(SehipError):
        metric.stoi_ratio(0)
    with pytest.raises(SehipError):
        metric.stoi_ratio(-16000)
    with pytest.raises(SehipError):
        metric.stoi_ratio(16001)                      # 10000 / 16001 does not reduce: p = 10000
    with pytest.raises(SehipError):
        metric.stoi_workspace(1, 255, 10000, "cpu")   # fewer than 256 samples at 10 kHz
    with pytest.raises(SehipError):
        metric.stoi_workspace(1, 408, 16000, "cpu")   # 408 samples at 16 kHz are 255 at 10 kHz
    with pytest.raises(SehipError):
        metric.STOI(torch.zeros(1, 4000), torch.zeros(1, 4000))   # host tensors: no CPU fallback


@pytest.mark.parametrize("sr", [16000, 48000, 44100, 8000])
def test_package_table_is_the_oracles(sr):
    from sehip.metric import stoi_resample_table
    table, p, q, L = stoi_resample_table(sr)
    rp, rq, rL, rtab = R.phase_table(sr)
    assert (p, q, L) == (rp, rq, rL)
    assert np.array_equal(table.numpy(), rtab.astype(np.float32))
