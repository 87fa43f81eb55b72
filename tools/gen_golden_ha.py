#!/usr/bin/env python3
"""tests/golden/ha_taps.npz and tests/golden/ha_chain.npz from the IMPORTED reference (the path of a reference checkout is the first
argument or $SEHIP_REFERENCE).  Data only: nothing of the reference's program text is written.

  ha_taps:  NALRTorch(nfir, fs).build(hl, cfs) for (nfir, fs) in tests/ha_ref.py TAPS_CASES and the four audiograms of AUDIOGRAMS
            (keys '<nfir>_<fs>_<name>', [1, 1, nfir + 1] fp32, reversed as the reference stores them)
  ha_chain: one amplify_torch call (tests/ha_ref.py CHAIN: fs 16000, nfir 32, signal [2, 1, 2, 4000], the compressor settings of
            src/ha/conf/config.yaml): signal, the FIR output, the compressor output, the amplify_torch output (soft_clip=True), a
            fixed upstream G and the gradient of <out, G> with respect to the signal, and `margin`, the smallest relative distance
            of the float64 level from the threshold.  Refused when that margin is below 1e-7: a level that close may fall on
            either side of the threshold in another summation order.

The reference needs scipy.signal.hamming, which current scipy has moved to scipy.signal.windows: it is aliased before the import.
With --time: the reference's wall time of one [4, 1, 2, 264600] call at 44.1 kHz (nfir 220, shipped settings) on this host.
Run:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_ha.py /path/to/reference [--time]"""
import os
import sys
import time

import numpy as np
import torch

sys.dont_write_bytecode = True
ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
REFERENCE = ARGS[0] if ARGS else os.environ.get("SEHIP_REFERENCE")
if not REFERENCE:
    sys.exit("usage: gen_golden_ha.py /path/to/reference [--time]")
sys.path.insert(0, REFERENCE)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLDEN = os.path.join(ROOT, "tests", "golden")

import scipy.signal  # noqa: E402
import scipy.signal.windows  # noqa: E402
import scipy.interpolate  # noqa: E402,F401  (the reference reaches scipy.interpolate through the bare `import scipy`)

if not hasattr(scipy.signal, "hamming"):
    scipy.signal.hamming = scipy.signal.windows.hamming

from src.ha.amplifier import NALRTorch  # noqa: E402
from src.ha.compressor import CompressorTorch  # noqa: E402
from src.audio import amplify_torch  # noqa: E402
import ha_ref as R  # noqa: E402  (the fixture list: one for the generator and the tests)


def taps_fixture():
    out = {}
    for nfir, fs in R.TAPS_CASES:
        for name, hl in R.AUDIOGRAMS.items():
            out[f"{nfir}_{fs}_{name}"] = NALRTorch(nfir=nfir, fs=fs).build(np.array(hl), np.array(R.CFS)).numpy()
    path = os.path.join(GOLDEN, "ha_taps.npz")
    np.savez_compressed(path, **out)
    print(os.path.basename(path), len(out), "entries", os.path.getsize(path), "bytes")


def chain_fixture():
    c = R.CHAIN
    enh = NALRTorch(nfir=c["nfir"], fs=c["fs"])
    comp = CompressorTorch(fs=c["fs"], **c["compressor"])
    cfg = R.compressor_config(c["fs"], **c["compressor"])
    signal = torch.from_numpy(R.chain_signal()).requires_grad_(True)
    G = torch.from_numpy(R.chain_upstream())
    out = amplify_torch(signal, enh, comp, c["audiogram"], soft_clip=True)
    (out * G).sum().backward()
    with torch.no_grad():
        left = enh.build(np.array(c["audiogram"]["audiogram_levels_l"]), np.array(c["audiogram"]["audiogram_cfs"]))
        fir = torch.stack([enh.apply(left, signal[:, :, e]) for e in range(2)], dim=2)          # (the right ear through the LEFT taps)
        cmp_ = torch.stack([comp.process(fir[:, :, e]) for e in range(2)], dim=2)
        assert torch.equal(torch.tanh(cmp_), out.detach())
    lv = np.stack([R.level(r, cfg["W"], direct=True) for r in fir.numpy().reshape(-1, fir.shape[-1])])
    margin = R.margin(lv, cfg["threshold"])
    above = float((lv > cfg["threshold"]).mean())
    crossings = int((np.diff((lv > cfg["threshold"]).astype(np.int8), axis=-1) != 0).sum())
    print(f"chain: level margin {margin:.3e}, {above:.1%} of the samples above the threshold, {crossings} crossings")
    if margin < R.MIN_MARGIN:
        sys.exit(f"refused: the float64 level comes within {margin:.3e} (relative) of the threshold; change CHAIN['seed']")
    path = os.path.join(GOLDEN, "ha_chain.npz")
    np.savez_compressed(path, signal=signal.detach().numpy(), G=G.numpy(), taps_left=left.numpy(), fir=fir.numpy(), comp=cmp_.numpy(),
                        out=out.detach().numpy(), grad=signal.grad.numpy(), margin=np.float64(margin), above=np.float64(above),
                        crossings=np.int64(crossings))
    print(os.path.basename(path), os.path.getsize(path), "bytes")


def time_reference():
    enh = NALRTorch(nfir=220, fs=44100)
    comp = CompressorTorch(fs=44100, **R.CHAIN["compressor"])
    rng = np.random.RandomState(3)
    t = np.arange(264600) / 44100
    x = (0.05 * rng.standard_normal((4, 1, 2, 264600)) * (0.5 + 0.5 * np.sin(2 * np.pi * 3 * t)) ** 2).astype(np.float32)
    t0 = time.perf_counter()
    amplify_torch(torch.from_numpy(x), enh, comp, R.CHAIN["audiogram"], soft_clip=True)
    print(f"reference amplify_torch [4, 1, 2, 264600] at 44.1 kHz on this CPU host: {time.perf_counter() - t0:.2f} s")


if __name__ == "__main__":
    if "--time" in sys.argv:
        time_reference()
    else:
        taps_fixture()
        chain_fixture()
