"""NAL-R amplifier of the hearing-aid stage (the reference's src/ha/amplifier.py:129-215 NALRTorch).

build() designs the linear-phase FIR on the host in float64 numpy (no scipy: np.hamming is the symmetric window scipy.signal.hamming
gave the reference, np.interp stands for interp1d) and returns it as the reference does, REVERSED, [1, 1, nfir + 1] fp32, so that
torch.conv1d(wav, nalr, padding=nfir) is the convolution with the designed filter.  apply() is that convolution on the device
(csrc/hearing_aid.hip), differentiable with respect to the signal.  There is no CPU path: apply() on a CPU tensor raises SehipError.
"""
import numpy as np
import torch

from .. import _lib
from .._lib import SehipError, call, ptr, stream

K_MAX = 1025


def _interp_strict(x_new, x, y, what):
    """Piecewise-linear interpolation that refuses to extrapolate (what interp1d does with its default bounds_error)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if x.ndim != 1 or x.shape != y.shape or x.size < 2:
        raise ValueError("Hearing losses (hl) and center frequencies (cfs) don't match!")
    order = np.argsort(x, kind="stable")
    x, y = x[order], y[order]
    x_new = np.asarray(x_new, dtype=np.float64)
    if x_new.min() < x[0] or x_new.max() > x[-1]:
        raise ValueError(f"{what}: a frequency in [{x_new.min():g}, {x_new.max():g}] Hz lies outside the given range "
                         f"[{x[0]:g}, {x[-1]:g}] Hz")
    return np.interp(x_new, x, y)


def frequency_sampling_fir(order, freq, mag):
    """order + 1 taps of the frequency-sampling design the reference uses (MATLAB's fir2 with its default grid and a Hamming
    window): the magnitude breakpoints are drawn as straight segments on a grid of npt + 1 points over [0, Nyquist], given the
    linear phase of a delay of order / 2 samples, mirrored to a Hermitian spectrum, transformed back and windowed."""
    taps = order + 1
    npt = 512 if taps < 1024 else int(2 ** np.ceil(np.log2(taps)))
    freq = np.array(freq, dtype=np.float64)
    mag = np.asarray(mag, dtype=np.float64)
    freq[0], freq[-1] = 0.0, 1.0
    grid = npt + 1
    resp = np.zeros(grid)
    resp[0] = mag[0]
    lo = 0
    for i in range(len(freq) - 1):
        if freq[i + 1] == freq[i]:                                # a step: blended over npt / 25 grid points
            lap = int(np.fix(npt / 25))
            lo = int(np.ceil(lo - lap / 2))
            hi = lo + lap - 1
        else:
            hi = int(np.fix(freq[i + 1] * grid)) - 1
        idx = np.arange(lo, hi + 1)
        frac = np.zeros(len(idx)) if lo == hi else (idx - lo) / (hi - lo)
        resp[lo:hi + 1] = frac * mag[i + 1] + (1 - frac) * mag[i]
        lo = hi + 1
    phase = np.exp(-0.5j * order * np.pi * np.arange(grid) / (grid - 1))
    half = resp * phase
    spectrum = np.concatenate((half, half[grid - 2:0:-1].conj()))
    impulse = np.fft.ifft(spectrum).real
    return impulse[:taps] * np.hamming(taps)


class NALRTorch:
    AUD = (250, 500, 1000, 2000, 4000, 6000)                      # audiometric frequencies of the prescription
    BIAS = (-17, -8, 1, -1, -2, -2)

    def __init__(self, nfir, fs):
        """nfir: order of the NAL-R filter (nfir + 1 taps, delay nfir // 2); fs: sampling rate in Hz"""
        nfir = int(nfir)
        if not 0 <= nfir <= K_MAX - 1:
            raise SehipError(f"NALRTorch: nfir={nfir}: the device FIR takes K = nfir + 1 taps in [1, {K_MAX}]")
        self.nfir = nfir
        self.fs = fs
        self.fmax = 0.5 * fs
        self.aud = np.array(self.AUD, dtype=np.float32)
        self.delay = np.zeros(nfir + 1)
        self.delay[nfir // 2] = 1.0
        self._device_taps = {}

    def hl_interp(self, hl, cfs):
        return _interp_strict(self.aud, cfs, hl, "NALRTorch.build: audiometric frequencies")

    def design(self, hl, cfs=None):
        """the nfir + 1 designed taps in float64, in filter order (not reversed)"""
        if cfs is None:
            cfs = np.array([250, 500, 1000, 2000, 3000, 6000])
        hl = self.hl_interp(np.array(hl), np.array(cfs))
        if np.max(hl) <= 0:
            return self.delay.copy()
        t3 = hl[1] + hl[2] + hl[3]
        xave = 0.05 * t3 if t3 <= 180 else 9.0 + 0.116 * (t3 - 180)
        gdb = np.clip(xave + 0.31 * hl + np.array(self.BIAS), 0, None)
        fv = np.concatenate(([0.0], self.aud, [self.fmax]))
        gv = np.concatenate(([gdb[0]], gdb, [gdb[-1]]))
        cfreq = np.linspace(0, self.nfir, self.nfir + 1) / self.nfir
        glin = np.power(10, _interp_strict(self.fmax * cfreq, fv, gv, "NALRTorch.build: filter grid") / 20.0)
        return frequency_sampling_fir(self.nfir, cfreq, glin)

    def build(self, hl, cfs=None):
        """hl: hearing thresholds at `cfs` (default [250, 500, 1000, 2000, 3000, 6000] Hz) -> [1, 1, nfir + 1] fp32 CPU tensor, the
        taps reversed as the reference stores them.  ValueError when an audiometric frequency falls outside `cfs`."""
        nalr = self.design(hl, cfs).astype(np.float32)
        return torch.from_numpy(nalr[::-1].copy()).reshape(1, 1, nalr.shape[-1])

    def build_on(self, hl, cfs, device):
        """build() moved to `device`, cached per (hl, cfs, device): a repeated call copies nothing from the host, so a call that
        was made once can be captured into a graph."""
        key = (tuple(float(v) for v in np.asarray(hl).reshape(-1)), None if cfs is None else tuple(float(v) for v in np.asarray(cfs).reshape(-1)),
               str(device))
        if key not in self._device_taps:
            self._device_taps[key] = self.build(hl, cfs).to(device)
        return self._device_taps[key]

    def apply(self, nalr, wav):
        """nalr: what build() returned, on the device; wav [B, S, n] fp32 on the device -> [B, S, n + nfir]: every row convolved
        with the filter (torch.conv1d(wav, nalr, padding=nfir) for S = 1, where the reference stops; here rows are independent)."""
        check_signal(wav, 3, "NALRTorch.apply")
        if not torch.is_tensor(nalr) or nalr.dim() != 3 or nalr.shape[0] != 1 or nalr.shape[1] != 1:
            raise SehipError(f"NALRTorch.apply: taps of shape {tuple(getattr(nalr, 'shape', ()))}; build() returns [1, 1, nfir + 1]")
        taps = stored_to_filter_order(nalr, "NALRTorch.apply")
        b, s, n = wav.shape
        return fir_apply(wav.reshape(b * s, n), taps).reshape(b, s, n + taps.shape[-1] - 1)


def check_signal(t, dim, what):
    if not torch.is_tensor(t):
        raise SehipError(f"{what}: expected a tensor, got {type(t).__name__}")
    if t.dtype != torch.float32:
        raise SehipError(f"{what}: dtype {t.dtype}; the HIP path takes fp32")
    if t.dim() != dim:
        raise SehipError(f"{what}: {t.dim()} axes, expected {dim}")
    if t.numel() == 0:
        raise SehipError(f"{what}: empty tensor of shape {tuple(t.shape)}")
    _lib.require_gpu(t, what)


def stored_to_filter_order(nalr, what):
    """[..., K] taps as build() stores them (reversed) -> [F, K] contiguous fp32 in filter order on their device"""
    _lib.require_gpu(nalr, what + " (taps)")
    if nalr.dtype != torch.float32:
        raise SehipError(f"{what}: taps of dtype {nalr.dtype}; the HIP path takes fp32")
    k = nalr.shape[-1]
    if not 1 <= k <= K_MAX:
        raise SehipError(f"{what}: K={k} taps outside [1, {K_MAX}]")
    return nalr.reshape(-1, k).flip(-1).contiguous()


class _Fir(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, taps, row_set):
        rows, n = x.shape
        f, k = taps.shape
        x = x.contiguous()
        out = torch.empty(rows, n + k - 1, device=x.device, dtype=torch.float32)
        call("sehip_ha_fir_fwd", ptr(x), rows, n, ptr(taps), f, k, ptr(row_set), ptr(out), stream())
        ctx.save_for_backward(taps, row_set)
        ctx.n = n
        return out

    @staticmethod
    def backward(ctx, dout):
        taps, row_set = ctx.saved_tensors
        dout = dout.contiguous()
        rows = dout.shape[0]
        f, k = taps.shape
        dx = torch.empty(rows, ctx.n, device=dout.device, dtype=torch.float32)
        call("sehip_ha_fir_adj", ptr(dout), rows, ctx.n, ptr(taps), f, k, ptr(row_set), ptr(dx), stream())
        return dx, None, None


def fir_apply(x, taps, row_set=None):
    """x [rows, n] fp32, taps [F, K] fp32 in filter order, row_set [rows] int32 (None: set 0) -> [rows, n + K - 1];
    out[r][m] = sum_k taps[row_set[r]][k] x[r][m - k].  Differentiable with respect to x."""
    check_signal(x, 2, "fir_apply")
    check_signal(taps, 2, "fir_apply (taps)")
    if not 1 <= taps.shape[1] <= K_MAX:
        raise SehipError(f"fir_apply: K={taps.shape[1]} taps outside [1, {K_MAX}]")
    if row_set is not None:
        _lib.require_gpu(row_set, "fir_apply (row_set)")
        if row_set.dtype != torch.int32 or tuple(row_set.shape) != (x.shape[0],):
            raise SehipError(f"fir_apply: row_set must be int32 [{x.shape[0]}], got {row_set.dtype} {tuple(row_set.shape)}")
        row_set = row_set.contiguous()
    return _Fir.apply(x, taps.contiguous(), row_set)


def fir_adjoint(dout, taps, n, row_set=None):
    """dout [rows, n + K - 1] -> [rows, n]: dx[r][i] = sum_k taps[row_set[r]][k] dout[r][i + k] (the transpose of fir_apply)"""
    check_signal(dout, 2, "fir_adjoint")
    check_signal(taps, 2, "fir_adjoint (taps)")
    f, k = taps.shape
    if not 1 <= k <= K_MAX:
        raise SehipError(f"fir_adjoint: K={k} taps outside [1, {K_MAX}]")
    if n < 1 or dout.shape[1] != n + k - 1:
        raise SehipError(f"fir_adjoint: dout has {dout.shape[1]} columns, expected n + K - 1 = {n + k - 1}")
    if row_set is not None:
        _lib.require_gpu(row_set, "fir_adjoint (row_set)")
        if row_set.dtype != torch.int32 or tuple(row_set.shape) != (dout.shape[0],):
            raise SehipError(f"fir_adjoint: row_set must be int32 [{dout.shape[0]}]")
        row_set = row_set.contiguous()
    dout, taps = dout.contiguous(), taps.contiguous()
    dx = torch.empty(dout.shape[0], n, device=dout.device, dtype=torch.float32)
    call("sehip_ha_fir_adj", ptr(dout), dout.shape[0], n, ptr(taps), f, k, ptr(row_set), ptr(dx), stream())
    return dx
