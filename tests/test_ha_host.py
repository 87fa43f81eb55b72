"""CPU: the host side of the hearing-aid stage (sehip/ha, sehip/audio.py) and its float64 restatement (tests/ha_ref.py) against
vectors recorded from the reference (tests/golden/ha_taps.npz, ha_chain.npz; tools/gen_golden_ha.py).

  NALRTorch.build: float64 design and one fp32 cast, against the reference's taps at 1e-6 (norm-relative; the remainder is the FFT's
                   summation order), the four branches (docstring audiogram, pure delay, t3 > 180, gains clipped to 0), ValueError
                   where interp1d raises.
  ha_ref:          FIR, compressor, amplify_torch output and the input gradient of the chain fixture at ACT_TOL = 5e-5
                   (tests/test_oracle_golden.py's value for fp32 reference vectors); its vectorised paths against its loops.
  Plumbing:        convert_audio_channels, the rejections (no CPU fallback), the exports, the workspace helper.  No GPU call."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ha_ref as R
from util import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ACT_TOL = 5e-5
TAPS_TOL = 1e-6
NEW_ENTRY_POINTS = ("sehip_ha_fir_fwd", "sehip_ha_fir_adj", "sehip_ha_compressor_ws_doubles", "sehip_ha_compressor_fwd",
                    "sehip_ha_compressor_bwd")
_FX = {}


def fixture(name):
    if name not in _FX:
        with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
            _FX[name] = {k: z[k] for k in z.files}
    return _FX[name]


@pytest.mark.parametrize("nfir,fs", R.TAPS_CASES)
@pytest.mark.parametrize("name", sorted(R.AUDIOGRAMS))
def test_build_matches_the_reference_taps(nfir, fs, name):
    from sehip.ha import NALRTorch
    want = fixture("ha_taps")[f"{nfir}_{fs}_{name}"]
    got = NALRTorch(nfir, fs).build(np.array(R.AUDIOGRAMS[name]), np.array(R.CFS))
    assert tuple(got.shape) == (1, 1, nfir + 1) == want.shape and got.dtype == torch.float32 and not got.is_cuda
    err = rel_err(got, want)
    print(f"[ha taps {nfir}/{fs}/{name}] rel {err:.3e}")
    assert err < TAPS_TOL
    ref64 = R.design(nfir, fs, R.AUDIOGRAMS[name], R.CFS)
    assert rel_err(ref64[::-1].copy(), want) < TAPS_TOL           # the restatement too (stored reversed)
    if name == "zeros":                                           # mloss <= 0: exactly the delay
        d = np.zeros(nfir + 1, dtype=np.float32)
        d[nfir // 2] = 1
        assert np.array_equal(got.numpy().reshape(-1), d[::-1])


def test_build_branches_are_the_ones_the_fixtures_name():
    aud = lambda hl: np.interp(R.AUD, R.CFS, hl)  # noqa: E731
    sev, low = aud(R.AUDIOGRAMS["severe"]), aud(R.AUDIOGRAMS["mild_low"])
    assert sev[1] + sev[2] + sev[3] > 180 and aud(R.AUDIOGRAMS["docstring"])[1:4].sum() <= 180
    t3 = low[1] + low[2] + low[3]
    raw = 0.05 * t3 + 0.31 * low + R.BIAS
    assert raw[0] < 0 and raw[1] < 0 and raw[-1] > 0              # the low-frequency gains clip, the high ones do not


def test_build_raises_where_interp1d_would():
    from sehip.ha import NALRTorch
    amp = NALRTorch(32, 16000)
    with pytest.raises(ValueError):
        amp.build([10, 20, 30, 40], [500, 1000, 2000, 4000])     # 250 Hz and 6 kHz lie outside cfs
    with pytest.raises(ValueError):
        amp.build([10, 20, 30], R.CFS)                            # lengths differ
    assert tuple(amp.build([10] * 6).shape) == (1, 1, 33)         # the default cfs reach from 250 Hz to 6 kHz


def test_restatement_matches_the_reference_chain():
    fx, c = fixture("ha_chain"), R.CHAIN
    assert float(fx["margin"]) >= R.MIN_MARGIN
    assert np.array_equal(fx["signal"], R.chain_signal()) and np.array_equal(fx["G"], R.chain_upstream())
    cfg = R.compressor_config(c["fs"], **c["compressor"])
    taps = R.design(c["nfir"], c["fs"], c["audiogram"]["audiogram_levels_l"], c["audiogram"]["audiogram_cfs"])
    assert rel_err(taps[::-1].copy(), fx["taps_left"]) < TAPS_TOL
    taps32 = fx["taps_left"].reshape(-1)[::-1].astype(np.float64)  # the fp32 taps the reference convolved with
    n = c["shape"][-1]
    rows = fx["signal"].reshape(-1, n)
    st = R.chain(rows, taps32, cfg, soft_clip=True, direct_level=True)
    assert R.margin(st["level"], cfg["threshold"]) >= R.MIN_MARGIN
    shape = fx["out"].shape
    errs = dict(fir=rel_err(st["fir"].reshape(shape), fx["fir"]), comp=rel_err(st["prod"].reshape(shape), fx["comp"]),
                out=rel_err(st["out"].reshape(shape), fx["out"]),
                grad=rel_err(R.chain_grad(fx["G"].reshape(-1, shape[-1]), st, taps32, n).reshape(fx["grad"].shape), fx["grad"]))
    print("[ha_ref vs reference]", {k: f"{v:.3e}" for k, v in errs.items()})
    assert all(v < ACT_TOL for v in errs.values()), errs
    # the gain the reference multiplied with, recovered where the signal is not tiny, is the fp32 rounding of the float64 loop
    big = np.abs(fx["fir"]) > 1e-3
    assert np.abs(fx["comp"][big] / fx["fir"][big] - st["gain32"].reshape(shape)[big]).max() < 2e-7
    # the vectorised paths (prefix-sum level, blocked recurrence) agree with the loops
    fast = R.chain(rows, taps32, cfg, soft_clip=True, loop=False, direct_level=False)
    # level: each of the two prefixes carries at most n roundings of 2^-53 of the row's total, the square root halves the relative
    # error: |d lv| / lv <= n 2^-53 total / (W lv^2).  gain: the same float64 recurrence, a block's roundings (<= 4 per sample)
    # accumulate before the contraction a < 1 damps them; 1e-10 is 500 x below the fp32 half-ulp that the gates care about
    total = (st["fir"] ** 2).sum(-1, keepdims=True)
    lv_bound = st["fir"].shape[-1] * 2.0 ** -53 * total / (cfg["W"] * st["level"] ** 2)
    assert bool((np.abs(fast["level"] / st["level"] - 1) <= lv_bound).all())
    assert np.abs(fast["gain"] / st["gain"] - 1).max() < 1e-10


def test_convert_audio_channels():
    from sehip.audio import convert_audio_channels
    g = torch.Generator().manual_seed(0)
    x = torch.randn(3, 2, 4, 50, generator=g)
    assert convert_audio_channels(x, 4) is x                                                       # same count
    assert torch.equal(convert_audio_channels(x, 1), x.mean(dim=-2, keepdim=True))                 # downmix
    mono = x[:, :, :1]
    up = convert_audio_channels(mono, 2)
    assert tuple(up.shape) == (3, 2, 2, 50) and torch.equal(up[:, :, 1], mono[:, :, 0]) and up.data_ptr() == mono.data_ptr()
    cut = convert_audio_channels(x, 2)
    assert torch.equal(cut, x[:, :, :2]) and cut.data_ptr() == x.data_ptr()                        # first channels, a view
    with pytest.raises(ValueError):
        convert_audio_channels(x[:, :, :2], 3)
    assert tuple(convert_audio_channels(torch.zeros(2, 9)).shape) == (2, 9)                        # no batch axes, default channels=2


def test_cpu_wrong_dtype_and_empty_tensors_are_refused():
    import sehip
    from sehip import SehipError
    from sehip.ha import CompressorTorch, NALRTorch, compress_rows, fir_apply
    amp, comp = NALRTorch(32, 16000), CompressorTorch(fs=16000, **R.CHAIN["compressor"])
    taps = amp.build(R.AUDIOGRAMS["docstring"], R.CFS)
    with pytest.raises(SehipError, match="no CPU fallback"):
        amp.apply(taps, torch.zeros(1, 1, 100))
    with pytest.raises(SehipError, match="no CPU fallback"):
        comp.process(torch.zeros(1, 1, 100))
    with pytest.raises(SehipError, match="no CPU fallback"):
        sehip.amplify_torch(torch.zeros(1, 1, 2, 100), amp, comp, R.CHAIN["audiogram"])
    with pytest.raises(SehipError, match="no CPU fallback"):
        fir_apply(torch.zeros(2, 10), torch.zeros(1, 3))
    with pytest.raises(SehipError, match="no CPU fallback"):
        compress_rows(torch.zeros(2, 10), comp)
    # dtype, rank and emptiness are checked before the device, so they show without a GPU
    for bad, what in ((torch.zeros(1, 1, 100, dtype=torch.float64), "dtype"), (torch.zeros(1, 1, 100, dtype=torch.bfloat16), "dtype"),
                      (torch.zeros(1, 1, 0), "empty"), (torch.zeros(1, 100), "axes")):
        with pytest.raises(SehipError, match=what):
            comp.process(bad)
        with pytest.raises(SehipError, match=what):
            amp.apply(taps, bad)
    with pytest.raises(SehipError, match="dtype"):
        sehip.amplify_torch(torch.zeros(1, 1, 2, 100, dtype=torch.float16), amp, comp, R.CHAIN["audiogram"])
    with pytest.raises(SehipError, match="empty"):
        sehip.amplify_torch(torch.zeros(0, 1, 2, 100), amp, comp, R.CHAIN["audiogram"])
    with pytest.raises(SehipError):
        comp.process("not a tensor")


def test_k_and_window_out_of_range():
    from sehip import SehipError, _lib
    from sehip.ha import CompressorTorch, NALRTorch
    with pytest.raises(SehipError, match="1025"):
        NALRTorch(1025, 44100)                                    # K = 1026
    with pytest.raises(SehipError):
        NALRTorch(-1, 44100)
    NALRTorch(1024, 44100)
    with pytest.raises(SehipError, match="W = 0"):
        CompressorTorch(fs=16000, rms_buffer_size=0.00001)
    assert CompressorTorch().win_len == 8820 and CompressorTorch(fs=16000, rms_buffer_size=0.064).win_len == 1024
    # the C ABI validates before any HIP call: safe without a GPU
    lib = _lib.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    for K in (0, 1026):
        assert lib.sehip_ha_fir_fwd(p, 1, 10, p, 1, K, None, p, None) != 0
        assert b"K=" in lib.sehip_last_error()
        assert lib.sehip_ha_fir_adj(p, 1, 10, p, 1, K, None, p, None) != 0
    assert lib.sehip_ha_fir_fwd(p, 0, 10, p, 1, 3, None, p, None) != 0 and b"empty" in lib.sehip_last_error()
    assert lib.sehip_ha_fir_fwd(p, 1, 0, p, 1, 3, None, p, None) != 0
    assert lib.sehip_ha_fir_fwd(p, 1, 10, p, 0, 3, None, p, None) != 0
    assert lib.sehip_ha_fir_fwd(None, 1, 10, p, 1, 3, None, p, None) != 0 and b"null" in lib.sehip_last_error()
    assert lib.sehip_ha_compressor_fwd(p, 1, 10, 0, 0.35, 0.1, 0.1, 0.1, 1, p, p, p, None) != 0
    assert b"W=0" in lib.sehip_last_error()
    assert lib.sehip_ha_compressor_fwd(p, 1, 0, 4, 0.35, 0.1, 0.1, 0.1, 1, p, p, p, None) != 0
    assert lib.sehip_ha_compressor_fwd(p, 1, 10, 4, float("nan"), 0.1, 0.1, 0.1, 1, p, p, p, None) != 0
    assert lib.sehip_ha_compressor_fwd(p, 1, 10, 4, 0.35, 0.1, 0.1, 0.1, 1, None, p, p, None) != 0
    assert lib.sehip_ha_compressor_bwd(p, p, p, 0, 1, p, None) != 0
    with pytest.raises(SehipError):
        _lib.call("sehip_ha_compressor_bwd", None, None, None, 5, 1, None, None)


def test_workspace_helper():
    from sehip import _lib
    ws = _lib.lib().sehip_ha_compressor_ws_doubles
    assert ws(1, 1, 1) == 1 + 5
    assert ws(4, 1024, 64) == 4 * 1024 + 5 * 4 and ws(4, 1025, 64) == 4 * 1025 + 5 * 4 * 2
    assert ws(8, 264820, 2822) == 8 * 264820 + 5 * 8 * 259
    assert ws(3, 5000, 1) == ws(3, 5000, 10 ** 6)                 # the window does not change the workspace
    for bad in ((0, 10, 4), (-1, 10, 4), (65536, 10, 4), (2, 0, 4), (2, -5, 4), (2, 2 ** 30 + 1, 4), (2, 10, 0), (2, 10, -3)):
        assert ws(*bad) == 0, bad


def test_new_symbols_are_declared_exported_and_bound():
    import sehip
    from sehip import _lib
    text = open(os.path.join(ROOT, "include", "sehip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(sehip_[a-z0-9_]+)\s*\(", text))
    lib = _lib.lib()
    for name in NEW_ENTRY_POINTS:
        assert name in declared and hasattr(lib, name) and name in _lib.declared_symbols(), name
    assert lib.sehip_ha_compressor_ws_doubles.restype is ctypes.c_long
    for name in ("NALRTorch", "CompressorTorch", "amplify_torch", "convert_audio_channels"):
        assert hasattr(sehip, name), name
    assert sehip.ha.NALRTorch is sehip.NALRTorch and sehip.audio.amplify_torch is sehip.amplify_torch
