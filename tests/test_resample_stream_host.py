"""CPU: the streaming resampler's float64 restatement (tests/resample_stream_ref.py: a state machine with exactly the device's state)
against the offline formula, the delay / history / flush-length arithmetic, the streamer's refusals (sehip.ResampleStreamer: all before
any launch, so they show without a GPU) and the plumbing of the new entries.

  Restatement: EQUAL to the offline formula up to float64 summation (1e-13 relative to the magnitude sum_k |h_k| |x_k|: both are float64
               matrix products of the same K <= 714 terms, K 2^-53 ~ 8e-14), for 441 -> 160, 160 -> 441, 3 -> 1, 1 -> 3, 2 -> 1,
               1 -> 2 and 7 -> 5, chunks shorter and longer than the delay, ragged feeds, tails of 0, 1 and old - 1 samples, a stream
               flushed before delay_frames frames arrived, and a reset in mid-stream.  The restatement asserts the history bound H and
               that no ring slot is read and written by one call; the ring starts as NaN, so a slot read before it is written shows."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import resample_stream_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("sehip_rss_delay_frames", "sehip_rss_state_bytes", "sehip_rss_feed", "sehip_rss_advance")
RATIOS = ((44100, 16000), (16000, 44100), (48000, 16000), (16000, 48000), (2, 1), (1, 2), (7, 5))
TOL = 1e-13


def _run(ref, x, sizes, r):
    """feeds the whole frames of x [rows, n] in pieces of `sizes` frames, flushes the last r samples -> (feeds, flushed)"""
    old = ref.old
    whole = (x.shape[1] - r) // old
    assert whole * old + r == x.shape[1]
    outs, i = [], 0
    for f in SR.pieces(whole, sizes):
        outs.append(ref.feed(x[:, i:i + f * old]))
        i += f * old
    feeds = np.concatenate(outs, -1) if outs else np.zeros((x.shape[0], 0))
    return feeds, ref.flush(x[:, i:] if r else None)


def _equal(got, want, mag, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert not np.isnan(got).any(), what
    assert bool((np.abs(got - want) <= TOL * np.maximum(mag, 1e-300)).all()), (what, float(np.abs(got - want).max()))


@pytest.mark.parametrize("old_sr,new_sr", RATIOS)
def test_state_machine_is_the_offline_formula(old_sr, new_sr):
    table, width, old, new = SR.tables(old_sr, new_sr)
    dq = SR.delay_frames(old, width)
    chunkings = ((1,), (3,), (7,), (1, 7, 2, 7)) if dq == 1 else ((1,), (5,), (32,), (100,), (1, 32, 2, 32))
    for sizes in chunkings:
        C = max(sizes)
        ring_frames = -(-(dq * old + width + C * old) // old)
        for r in sorted({0, 1, old - 1} & set(range(old))):
            frames = 3 * ring_frames + 2
            x = SR.signal(3, frames * old + r, 7 * old + new + r).astype(np.float64)
            want, mag = SR.offline(x, table, old, new, width)
            ref = SR.ResampleStreamRef(old_sr, new_sr, 3, C)
            feeds, tail = _run(ref, x, sizes, r)
            D = dq * new
            assert feeds.shape[1] == frames * new and not feeds[:, :D].any()               # the zero prefix, exact
            assert tail.shape[1] == want.shape[1] - max(frames - dq, 0) * new              # the flush length
            _equal(np.concatenate((feeds[:, D:], tail), -1), want, mag, (old, new, sizes, r))
            lo, hi = min(a for a, _ in ref.reads), max(b for _, b in ref.reads)
            assert lo == -(dq * old + width) and hi < 0                                    # the history bound H; causality
            # a second utterance on the same object
            x2 = x[:, ::-1][:, :(dq + 2) * old + r].copy()
            want2, mag2 = SR.offline(x2, table, old, new, width)
            feeds2, tail2 = _run(ref, x2, sizes, r)
            _equal(np.concatenate((feeds2[:, D:], tail2), -1), want2, mag2, ("second", old, new, sizes, r))


@pytest.mark.parametrize("old_sr,new_sr", RATIOS)
def test_flush_before_the_delay_has_passed(old_sr, new_sr):
    table, width, old, new = SR.tables(old_sr, new_sr)
    dq = SR.delay_frames(old, width)
    for frames in sorted({0, 1, dq - 1, dq}):
        for r in sorted({0, 1, old - 1} & set(range(old))):
            for C in (1, 5):
                ref = SR.ResampleStreamRef(old_sr, new_sr, 2, C)
                x = SR.signal(2, frames * old + r, 3 + frames + r).astype(np.float64)
                feeds, tail = _run(ref, x, (C,), r)
                assert not feeds.any()                                                     # (frames <= dq: nothing but the delay's zeros)
                want, mag = SR.offline(x, table, old, new, width) if x.shape[1] else (np.zeros((2, 0)), np.zeros((2, 0)))
                _equal(tail, want, mag, (old, new, frames, r, C))                          # the whole offline output from flush alone


def test_reset_in_mid_stream_starts_the_named_rows_afresh():
    old_sr, new_sr, C, cut, frames = 44100, 16000, 3, 6, 14
    table, width, old, new = SR.tables(old_sr, new_sr)
    x = SR.signal(4, frames * old, 11).astype(np.float64)
    ref = SR.ResampleStreamRef(old_sr, new_sr, 4, C)
    first = [ref.feed(x[:, i * old:(i + C) * old]) for i in range(0, cut, C)]
    ref.reset([0, 1])
    rest = [ref.feed(x[:, i * old:min(i + C, frames) * old]) for i in range(cut, frames, C)]
    tail = ref.flush()
    D = ref.dq * new
    whole, wmag = SR.offline(x, table, old, new, width)
    fresh, fmag = SR.offline(x[:, cut * old:], table, old, new, width)
    run_on = np.concatenate(first + rest + [tail], -1)[2:, D:]
    _equal(run_on, whole[2:], wmag[2:], "the rows that ran on")
    after = np.concatenate(rest + [tail], -1)[:2]
    assert not after[:, :D].any()
    _equal(after[:, D:], fresh[:2], fmag[:2], "the rows that were reset")


def test_delay_history_and_state_size_agree():
    from sehip import _lib
    from sehip import resample_stream as RS
    lib = _lib.lib()
    assert lib.sehip_rss_delay_frames.restype is ctypes.c_long and lib.sehip_rss_state_bytes.restype is ctypes.c_long
    want = {(44100, 16000): (1, 160), (16000, 44100): (1, 441), (48000, 16000): (26, 26), (16000, 48000): (26, 78), (22050, 16000): (1, 320),
            (2, 1): (26, 26), (1, 2): (26, 52), (16000, 11025): (1, 441)}
    for (old_sr, new_sr), (dq, D) in want.items():
        table, width, old, new = SR.tables(old_sr, new_sr)
        assert (old, new) == RS.reduced_ratio(old_sr, new_sr)
        assert SR.delay_frames(old, width) == dq == lib.sehip_rss_delay_frames(old, new, width) == RS.delay_frames_of(old, new, width)
        assert dq * new == D
        H = dq * old + width
        # frame q reads input up to q old + width + old - 1: with F frames fed, frame F - 1 - dq is the last computable one
        assert (dq * old >= width) and ((dq - 1) * old < width)
        for rows, C in ((1, 1), (4, 5), (65535, 16)):
            assert lib.sehip_rss_state_bytes(rows, old, new, width, C) == rows * (8 + 4 * (H + C * old)) == RS.state_bytes_of(rows, old, new, width, C)
        for fed in (0, 1, dq - 1, dq, dq + 3):
            for r in sorted({0, 1, old - 1} & set(range(old))):
                run, drop, keep = RS.flush_plan(fed, r, old, new, dq)
                assert (run, drop, keep) == SR.flush_lengths(fed, r, old, new, dq)
                n_out = (fed * old + r) * new // old
                assert keep == n_out - max(fed - dq, 0) * new and drop + keep <= run * new
    table, width, old, new = SR.tables(48000, 16000)
    for bad in ((0, old, new, width, 4), (65536, old, new, width, 4), (4, old, new, width, 0), (4, old, new, width, 4097), (4, 6, 2, width, 4),
                (4, 3, 3, width, 4), (4, 1025, 1, width, 4), (4, old, new, 0, 4), (4, old, new, 2 ** 16 + 1, 4)):
        assert lib.sehip_rss_state_bytes(*bad) == 0, bad
    for bad in ((6, 2, 5), (1, 1, 5), (0, 1, 5), (1025, 1, 5), (3, 1, 0)):
        assert lib.sehip_rss_delay_frames(*bad) == -1, bad


def test_refusals_come_before_any_launch():
    import sehip
    from sehip import SehipError
    from sehip import resample_stream as RS
    from sehip.resample_stream import ResampleStreamer
    cpu, dev = torch.device("cpu"), torch.device("cuda", 0)
    # the constructor: the ratio, the sizes, then the device
    for old_sr, new_sr in ((16000, 16000), (3, 3), (48000, 48000)):
        with pytest.raises(SehipError, match="1 -> 1"):
            ResampleStreamer(old_sr, new_sr)
    for old_sr, new_sr in ((1025, 1), (16000, 16001), (2050, 3)):
        with pytest.raises(SehipError, match="above 1024"):
            ResampleStreamer(old_sr, new_sr)
    for old_sr, new_sr in ((0, 1), (3, -1), (2.5, 1), (True, 2)):
        with pytest.raises(SehipError, match="_sr"):
            ResampleStreamer(old_sr, new_sr)
    for streams in (0, -1, 1.0, True):
        with pytest.raises(SehipError, match="streams"):
            ResampleStreamer(48000, 16000, streams=streams)
    for channels in (0, 2.0):
        with pytest.raises(SehipError, match="channels"):
            ResampleStreamer(48000, 16000, channels=channels)
    for chunk in (0, 4097, 2.5):
        with pytest.raises(SehipError, match="chunk_frames"):
            ResampleStreamer(48000, 16000, chunk_frames=chunk)
    with pytest.raises(SehipError, match="65535 rows"):
        ResampleStreamer(48000, 16000, streams=32768, channels=2)
    with pytest.raises(SehipError, match="no CPU fallback"):
        ResampleStreamer(48000, 16000, device="cpu")
    if not torch.cuda.is_available():
        with pytest.raises(SehipError, match="no GPU is visible"):
            ResampleStreamer(48000, 16000)
    # feed(): the check the streamer runs first (streams 3, channels 2, old 3, chunk_frames 4)
    chk = lambda x, graph=False, device=cpu: RS.check_feed(x, 3, 2, 3, 4, graph, device)
    assert chk(torch.zeros(3, 2, 12), True) == 4 and chk(torch.zeros(3, 2, 3)) == 1
    with pytest.raises(SehipError, match="device"):
        chk(torch.zeros(3, 2, 12), device=dev)                                                    # a CPU tensor
    for bad, what in ((torch.zeros(3, 12), "shape"), (torch.zeros(3, 2, 2, 12), "shape"), (torch.zeros(3, 1, 12), "shape"),
                      (torch.zeros(2, 2, 12), "shape"), (torch.zeros(3, 2, 12, dtype=torch.float64), "dtype"), (torch.zeros(3, 2, 15), "f=5"),
                      (torch.zeros(3, 2, 0), "f=0"), (torch.zeros(3, 2, 10), "whole frames"), ("no tensor", "tensor")):
        with pytest.raises(SehipError, match=what):
            chk(bad)
    with pytest.raises(SehipError, match="graph=True"):
        chk(torch.zeros(3, 2, 9), True)
    # flush(): 0 <= r < old
    tl = lambda t, device=cpu: RS.check_tail(t, 3, 2, 3, device)
    assert tl(None) == 0 and tl(torch.zeros(3, 2, 0)) == 0 and tl(torch.zeros(3, 2, 2)) == 2
    for bad, what in ((torch.zeros(3, 2, 3), "r=3"), (torch.zeros(3, 2, 7), "r=7"), (torch.zeros(3, 2), "shape"), (torch.zeros(3, 1, 2), "shape"),
                      (torch.zeros(3, 2, 2, dtype=torch.float64), "dtype"), ("no tensor", "tensor")):
        with pytest.raises(SehipError, match=what):
            tl(bad)
    with pytest.raises(SehipError, match="device"):
        tl(torch.zeros(3, 2, 2), dev)
    assert sehip.ResampleStreamer is ResampleStreamer


def test_the_c_entries_validate_before_any_hip_call():
    from sehip import SehipError, _lib
    lib = _lib.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    feed = lambda rows=4, f=2, C=2, old=3, new=1, width=77, end=-1, xin=p: lib.sehip_rss_feed(xin, rows, f, C, p, old, new, width, p, p, end, p, None)
    for kw, word in ((dict(rows=0), b"rows=0"), (dict(rows=65536), b"rows=65536"), (dict(f=0), b"frames=0"), (dict(f=3), b"frames=3"),
                     (dict(C=0), b"C=0"), (dict(C=4097, f=1), b"C=4097"), (dict(old=1025), b"term"), (dict(new=0), b"term"),
                     (dict(old=6, new=2), b"not reduced"), (dict(old=3, new=3), b"not reduced"), (dict(width=0), b"width=0"),
                     (dict(width=2 ** 16 + 1), b"width="), (dict(end=7), b"end_len=7"), (dict(xin=None), b"null")):
        assert feed(**kw) != 0 and word in lib.sehip_last_error(), (kw, lib.sehip_last_error())
    assert lib.sehip_rss_feed(None, 4, 2, 2, None, 3, 1, 77, None, None, -1, None, None) != 0 and b"null" in lib.sehip_last_error()
    assert lib.sehip_rss_advance(p, 0, 1, None) != 0 and b"rows=0" in lib.sehip_last_error()
    assert lib.sehip_rss_advance(p, 4, 0, None) != 0 and b"frames=0" in lib.sehip_last_error()
    assert lib.sehip_rss_advance(None, 4, 1, None) != 0 and b"null" in lib.sehip_last_error()
    with pytest.raises(SehipError):
        _lib.call("sehip_rss_advance", None, 4, 1, None)


def test_new_symbols_are_declared_exported_and_bound():
    import sehip
    from sehip import _lib, streamcore
    text = open(os.path.join(ROOT, "include", "sehip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(sehip_[a-z0-9_]+)\s*\(", text))
    lib = _lib.lib()
    for name in ENTRY_POINTS:
        assert name in declared and hasattr(lib, name) and name in _lib.declared_symbols(), name
    assert sehip.ResampleStreamer is sehip.resample_stream.ResampleStreamer
    assert issubclass(sehip.ResampleStreamer, streamcore.StreamCore)
