"""CPU: the chunked hearing-aid stage's float64 restatement (tests/ha_stream_ref.py) against the whole-signal one (tests/ha_ref.py), the
streamer's refusals (sehip.ha.AmplifyStreamer: all before any launch, so they show without a GPU) and the plumbing of the new entries.

  Restatement: FIR and gain within 1e-12 (relative) of ha_ref.chain on the whole signal, with K - 1 <, =, > chunk, W - 1 <, =, > chunk,
               W longer than the whole stream, ragged piece lengths, and a reset in mid-stream.  1e-12: both are float64; the FIR
               differs by the order of K <= 33 products (K 2^-53 ~ 4e-15), a level by the order of W <= 200 squares, and the
               recurrence contracts (ha_ref's own vectorised paths are held to 1e-10 in tests/test_ha_host.py).
  GPU cases:   the inputs of tests/test_gpu_ha_stream.py's compressor cases pass their input checks, and on them the restatement's
               gain rounds to the fp32 value of the sample loop's at every sample."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ha_ref as R
import ha_stream_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("sehip_has_state_bytes", "sehip_has_fir", "sehip_has_compress", "sehip_has_advance")
TOL = 1e-12


def _signal(rows, n, seed, fs=16000):
    rng = np.random.RandomState(seed)
    t = np.arange(n) / fs
    return np.stack([1.2 * rng.standard_normal(n) * (0.5 + 0.5 * np.sin(2 * np.pi * (40 + 9 * r) * t + r)) ** 2 for r in range(rows)])


def _cfg(W):
    cfg = R.compressor_config(16000, **R.CHAIN["compressor"])
    cfg["W"] = W
    return cfg


def _close(got, want, what):
    fir = np.abs(got["fir"] - want["fir"]).max() / np.abs(want["fir"]).max()
    gain = np.abs(got["gain"] / want["gain"] - 1).max()
    assert fir <= TOL and gain <= TOL, (what, fir, gain)
    assert np.array_equal(got["gain32"], want["gain32"]), what


#                                     K   W    chunk  pieces            n
@pytest.mark.parametrize("K,W,C,pieces,n", ((9, 40, 16, (16,), 400),               # K - 1 < chunk, W - 1 > chunk
                                            (17, 17, 16, (16,), 400),              # K - 1 = chunk, W - 1 = chunk
                                            (33, 8, 16, (16, 3, 1, 11), 400),      # K - 1 > chunk, W - 1 < chunk, ragged pieces
                                            (1, 1, 5, (5, 2), 101),                # no history at all
                                            (5, 700, 32, (32, 7), 300),            # W longer than the whole stream
                                            (12, 30, 100, (100, 64, 99), 900)))    # several segments per chunk (seg = 8 below)
def test_chunked_restatement_is_the_whole_signal_chain(K, W, C, pieces, n):
    rng = np.random.RandomState(K + W)
    taps = rng.standard_normal((3, K)) / np.sqrt(K)
    x, cfg = _signal(3, n, 5 + K), _cfg(W)
    want = R.chain(x, taps, cfg, soft_clip=True, direct_level=True)
    m, crossings, share = SR.input_checks(want["level"], cfg["threshold"])
    assert m >= R.MIN_MARGIN and (W > n or (crossings >= 2 and 0.05 < share < 0.95)), (m, crossings, share)
    for seg in (1024, 8):
        got = SR.run(SR.AmplifyStreamRef(taps, cfg, C, seg=seg), x, pieces)
        assert got["fir"].shape == (3, n + K - 1)
        _close(got, want, (K, W, C, seg))


def test_reset_in_mid_stream_starts_one_row_afresh():
    K, W, C, n, cut = 9, 40, 16, 400, 176
    rng = np.random.RandomState(3)
    taps = rng.standard_normal((3, K)) / np.sqrt(K)
    x, cfg = _signal(3, n, 8), _cfg(W)
    ref = SR.AmplifyStreamRef(taps, cfg, C)
    first = [ref.feed(x[:, i:i + C]) for i in range(0, cut, C)]
    ref.reset([1])
    rest = [ref.feed(x[:, i:i + C]) for i in range(cut, n, C)]
    got = {k: np.concatenate([p[k] for p in first + rest], -1) for k in ("fir", "gain", "gain32")}
    whole = R.chain(x, taps, cfg, direct_level=True)
    fresh = R.chain(x[:, cut:], taps, cfg, direct_level=True)
    for r in (0, 2):                                              # untouched: the uninterrupted run
        _close({k: got[k][r:r + 1] for k in got}, {k: whole[k][r:r + 1, :n] for k in got}, r)
    _close({k: got[k][1:2, cut:] for k in got}, {k: fresh[k][1:2, :n - cut] for k in got}, "row 1 after its reset")
    _close({k: got[k][1:2, :cut] for k in got}, {k: whole[k][1:2, :cut] for k in got}, "row 1 before its reset")
    # and a window of W exact zeros gives exactly sqrt(1e-8), whatever came before: the sums hold non-negative terms only
    quiet = ref.feed(np.zeros((3, C)))
    for _ in range(-(-(W + K) // C)):
        quiet = ref.feed(np.zeros((3, C)))
    assert np.array_equal(quiet["level"][:, -1], np.full(3, np.sqrt(R.EPS)))


@pytest.mark.parametrize("W,n,C", SR.COMP_CASES + (SR.LONG_CASE,))
def test_gpu_compressor_cases_pass_their_input_checks(W, n, C):
    z, cfg = SR.comp_signal(W, n).numpy(), SR.comp_cfg(W)
    want = R.compress(z, cfg, soft_clip=False, loop=True, direct_level=True)
    m, crossings, share = SR.input_checks(want["level"], cfg["threshold"])
    print(f"[ha stream case W={W} n={n} C={C}] margin {m:.3e}, {crossings} crossings, {share:.1%} above")
    assert m >= R.MIN_MARGIN and crossings >= 2 and 0.05 < share < 0.95
    ref = SR.AmplifyStreamRef(np.ones((4, 1)), cfg, C, soft_clip=False)
    got = {k: np.concatenate([ref.feed(z[:, i:i + C])[k] for i in range(0, n, C)], -1) for k in ("gain32",)}
    assert np.array_equal(got["gain32"], want["gain32"])


def test_refusals_come_before_any_launch():
    import sehip
    from sehip import SehipError
    from sehip.ha import AmplifyStreamer, CompressorTorch, NALRTorch
    from sehip.ha import stream as S
    amp, comp = NALRTorch(32, 16000), CompressorTorch(fs=16000, **R.CHAIN["compressor"])
    gram = R.CHAIN["audiogram"]
    dev = torch.device("cuda", 0)
    # feed(): the check the streamer runs first
    assert S.check_feed(torch.zeros(3, 2, 64), 3, 64, True, torch.device("cpu")) == 64
    with pytest.raises(SehipError, match="device"):
        S.check_feed(torch.zeros(3, 2, 64), 3, 64, False, dev)                                     # a CPU tensor
    for bad, what in ((torch.zeros(3, 64), "shape"), (torch.zeros(3, 2, 2, 64), "shape"), (torch.zeros(3, 1, 64), "shape"),
                      (torch.zeros(3, 3, 64), "shape"), (torch.zeros(2, 2, 64), "shape"), (torch.zeros(3, 2, 64, dtype=torch.float64), "dtype"),
                      (torch.zeros(3, 2, 65), "n=65"), (torch.zeros(3, 2, 0), "n=0"), ("no tensor", "tensor")):
        with pytest.raises(SehipError, match=what):
            S.check_feed(bad, 3, 64, False, torch.device("cpu"))
    with pytest.raises(SehipError, match="graph=True"):
        S.check_feed(torch.zeros(3, 2, 63), 3, 64, True, torch.device("cpu"))
    assert S.check_feed(torch.zeros(3, 2, 63), 3, 64, False, torch.device("cpu")) == 63
    # the constructors
    for streams in (0, -1, 1.0, True, 40000):
        with pytest.raises(SehipError, match="streams"):
            AmplifyStreamer(amp, comp, gram, streams=streams)
    for chunk in (0, 2 ** 16 + 1, 2.5):
        with pytest.raises(SehipError, match="chunk_samples"):
            AmplifyStreamer(amp, comp, gram, chunk_samples=chunk)
    with pytest.raises(SehipError, match="audiograms"):
        AmplifyStreamer(amp, comp, [gram, gram], streams=3)
    with pytest.raises(SehipError, match="audiograms"):
        AmplifyStreamer(amp, comp, "gram", streams=1)
    with pytest.raises(SehipError, match="no CPU fallback"):
        AmplifyStreamer(amp, comp, gram, device="cpu")
    with pytest.raises(SehipError, match="NALRTorch"):
        AmplifyStreamer(None, comp, gram)
    with pytest.raises(SehipError, match="CompressorTorch"):
        AmplifyStreamer(amp, None, gram)
    taps, rs = torch.zeros(2, 33), torch.zeros(6, dtype=torch.int32)
    with pytest.raises(SehipError, match="no CPU fallback"):
        AmplifyStreamer.from_taps(taps, rs, comp, streams=3)                                      # CPU tensors
    for bad in (torch.zeros(5, dtype=torch.int32), torch.zeros(3, 2, dtype=torch.int32), torch.zeros(6, dtype=torch.int64), None):
        with pytest.raises(SehipError, match="row_set"):
            AmplifyStreamer.from_taps(taps, bad, comp, streams=3)
    for bad in (torch.zeros(2, 1026), torch.zeros(2, 0)):
        with pytest.raises(SehipError, match="K="):
            AmplifyStreamer.from_taps(bad, rs, comp, streams=3)
    with pytest.raises(SehipError, match="taps"):
        AmplifyStreamer.from_taps(torch.zeros(33), rs, comp, streams=3)
    wide = CompressorTorch(fs=16000, **R.CHAIN["compressor"])
    for W in (0, 2 ** 20 + 1):
        wide.win_len = W
        with pytest.raises(SehipError, match="W="):
            AmplifyStreamer.from_taps(taps, rs, wide, streams=3)
        with pytest.raises(SehipError, match="W="):
            AmplifyStreamer(amp, wide, gram)
    # a ValueError of the right ear's audiogram surfaces although the filter is not used by default (design comes before the device)
    short = dict(gram, audiogram_levels_r=[10, 20, 30])
    with pytest.raises(ValueError):
        AmplifyStreamer(amp, comp, short)
    assert sehip.AmplifyStreamer is AmplifyStreamer


def test_the_c_entries_validate_before_any_hip_call():
    from sehip import SehipError, _lib
    lib = _lib.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    fir = lambda rows=4, n=8, C=8, F=1, K=3, W=5: lib.sehip_has_fir(p, rows, n, C, p, F, K, W, None, p, p, p, p, None)
    for kw, word in ((dict(K=0), b"K=0"), (dict(K=1026), b"K=1026"), (dict(W=0), b"W=0"), (dict(W=2 ** 20 + 1), b"W="), (dict(n=0), b"n=0"),
                     (dict(n=9), b"n=9"), (dict(C=0), b"C=0"), (dict(C=2 ** 16 + 1, n=1), b"C="), (dict(rows=0), b"rows=0"),
                     (dict(rows=65536), b"rows=65536"), (dict(F=0), b"F=0")):
        assert fir(**kw) != 0 and word in lib.sehip_last_error(), (kw, lib.sehip_last_error())
    assert lib.sehip_has_fir(None, 4, 8, 8, p, 1, 3, 5, None, p, p, p, p, None) != 0 and b"null" in lib.sehip_last_error()
    comp = lambda rows=4, n=8, C=8, W=5, thr=0.35, z=p: lib.sehip_has_compress(z, rows, n, C, W, p, p, thr, 0.1, 0.1, 0.1, 1, p, p, p, None)
    for kw, word in ((dict(W=0), b"W=0"), (dict(n=9), b"n=9"), (dict(rows=0), b"rows=0"), (dict(thr=float("nan")), b"NaN"),
                     (dict(z=None), b"null")):
        assert comp(**kw) != 0 and word in lib.sehip_last_error(), kw
    assert lib.sehip_has_advance(p, p, p, 0, 8, None) != 0 and lib.sehip_has_advance(p, p, p, 4, 0, None) != 0
    assert lib.sehip_has_advance(None, p, p, 4, 8, None) != 0 and b"null" in lib.sehip_last_error()
    with pytest.raises(SehipError):
        _lib.call("sehip_has_advance", None, None, None, 4, 8, None)


def test_state_size_helper():
    from sehip import _lib
    from sehip.ha import stream as S
    sb = _lib.lib().sehip_has_state_bytes
    assert sb.restype is ctypes.c_long
    # per row: pos (8), c (8), K - 1 + C input samples, W - 1 + C filtered samples
    assert sb(1, 1, 1, 1) == 8 + 8 + 4 + 4
    assert sb(4, 221, 8820, 64) == 4 * (16 + 4 * (220 + 64) + 4 * (8819 + 64))
    assert S.state_bytes_of(2, 221, 8820, 64) == sb(4, 221, 8820, 64)
    for bad in ((0, 3, 5, 8), (65536, 3, 5, 8), (4, 0, 5, 8), (4, 1026, 5, 8), (4, 3, 0, 8), (4, 3, 2 ** 20 + 1, 8), (4, 3, 5, 0),
                (4, 3, 5, 2 ** 16 + 1)):
        assert sb(*bad) == 0, bad


def test_new_symbols_are_declared_exported_and_bound():
    import sehip
    from sehip import _lib
    text = open(os.path.join(ROOT, "include", "sehip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(sehip_[a-z0-9_]+)\s*\(", text))
    lib = _lib.lib()
    for name in ENTRY_POINTS:
        assert name in declared and hasattr(lib, name) and name in _lib.declared_symbols(), name
    assert sehip.ha.AmplifyStreamer is sehip.AmplifyStreamer is sehip.ha.stream.AmplifyStreamer
    from sehip.model import streamer
    from sehip import streamcore
    assert issubclass(sehip.AmplifyStreamer, streamcore.StreamCore) and issubclass(streamer.ChunkStreamer, streamcore.StreamCore)
    assert not issubclass(sehip.AmplifyStreamer, streamer.ChunkStreamer)
    assert streamer.check_feed_input is streamcore.check_feed_input and streamer.parse_which is streamcore.parse_which
