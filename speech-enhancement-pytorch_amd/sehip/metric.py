"""On-device validation metrics: SI_SDR and STOI of src/metric.py without the round trip through numpy.

SI_SDR is src/metric.py:92-123.  STOI is src/metric.py:126-144, which calls `pystoi.stoi(clean, estimate, sr, extended=False)` per
utterance: here the published algorithm (Taal et al. 2011; extended: Jensen & Taal 2016) runs as HIP kernels (csrc/stoi.hip).  `pystoi`
is not available to this project, so parity with it is by restatement only: the kernels are pinned by tests/stoi_ref.py, a float64 numpy
restatement of the algorithm as pystoi transcribes it.  PESQ / HASPI / HASQI of src/metric.py wrap third-party CPU libraries (an
iterative, table-driven psychoacoustic model) and are out of scope."""
from math import gcd

import numpy as np
import torch

from ._cache import CaptureAwareCache, canonical_device
from ._lib import SehipError, call, lib, ptr, require_gpu, stream


def SI_SDR(reference, estimation, sr=16000):
    """reference / estimation: device tensors [..., T] of the same shape -> 0-dim device tensor (float32).

    Same arithmetic as the reference (projection on the reference signal, mean of the per-row energy ratios, THEN the
    logarithm; eps = float32 machine epsilon); `sr` is accepted and unused, as in the reference."""
    require_gpu(reference, "SI_SDR")
    require_gpu(estimation, "SI_SDR")
    if reference.shape != estimation.shape:
        raise ValueError(f"SI_SDR: shapes differ: {tuple(reference.shape)} vs {tuple(estimation.shape)}")
    n = reference.shape[-1]
    r = reference.reshape(-1, n).contiguous().float()
    e = estimation.reshape(-1, n).contiguous().float()
    ratios = torch.empty(r.shape[0], device=r.device, dtype=torch.float32)
    out = torch.empty((), device=r.device, dtype=torch.float32)
    call("sehip_sisdr_metric", ptr(r), ptr(e), r.shape[0], n, ptr(ratios), ptr(out), stream())
    return out


# ---- STOI ---------------------------------------------------------------------------------------------------------------------------
STOI_FS, STOI_FRAME, STOI_BANDS = 10000, 256, 15
STOI_MAX_P, STOI_MAX_Q, STOI_MAX_ROWS = 128, 1024, 32767
_stoi_tables = {}        # (p, q, device) -> (table [p][2 L / p + 1], p, q, L)
_stoi_workspaces = CaptureAwareCache()    # (rows, n, sr, device) -> dict of buffers


def stoi_ratio(sr, what="STOI"):
    """(p, q) = 10000 / sr reduced; refuses sr <= 0 and the ratios the resampler does not take"""
    if int(sr) != sr or sr <= 0:
        raise SehipError(f"{what}: the sample rate must be a positive integer, got {sr}")
    g = gcd(STOI_FS, int(sr))
    p, q = STOI_FS // g, int(sr) // g
    if p > STOI_MAX_P or q > STOI_MAX_Q:
        raise SehipError(f"{what}: sample rate {sr} needs the ratio {p} / {q}; the resampler takes p <= {STOI_MAX_P}, q <= {STOI_MAX_Q}")
    return p, q


def stoi_out_len(n, sr):
    """ceil(n p / q): the samples at 10 kHz of n samples at sr"""
    m = lib().sehip_stoi_out_len(int(n), int(sr))
    if m < 0:
        raise SehipError(f"STOI: bad length / sample rate (n={n}, sr={sr})")
    return int(m)


def stoi_resample_table(sr, device="cpu"):
    """-> (table fp32 [p][2 L / p + 1], p, q, L): the resampling filter of the MATLAB / pystoi STOI (`resample_oct`), a Kaiser-windowed
    sinc w of 2 L + 1 taps with fc = 1 / (2 max(p, q)), L = ceil((60 - 8) / (28.714 fc / 10)), beta = 0.1102 (60 - 8.7), normalised to
    unit sum; phase-major with the gain p folded in, table[r][i] = p w[r + i p], zero past the filter.  Built in float64 numpy, rounded
    once, cached per reduced ratio and device."""
    p, q = stoi_ratio(sr)
    if p == q:
        raise SehipError("STOI: 10 kHz input needs no resampling table")
    device = canonical_device(device)
    key = (p, q, str(device))
    hit = _stoi_tables.get(key)
    if hit is not None:
        return hit
    host = _stoi_tables.get((p, q, "cpu"))
    if host is None:
        fc = 1.0 / (2 * max(p, q))
        L = int(np.ceil((60 - 8) / (28.714 * fc / 10)))
        t = np.arange(-L, L + 1)
        h = np.kaiser(2 * L + 1, 0.1102 * (60 - 8.7)) * 2 * p * fc * np.sinc(2 * fc * t)
        w = h / np.sum(h)
        table = np.zeros((p, 2 * L // p + 1))
        for r in range(p):
            taps = w[r::p]
            table[r, :len(taps)] = p * taps
        host = (torch.from_numpy(table.astype(np.float32)).contiguous(), p, q, L)
        _stoi_tables[(p, q, "cpu")] = host
    if device.type != "cpu":
        host = (host[0].to(device), p, q, host[3])
        _stoi_tables[key] = host
    return host


def stoi_buffers(rows, n, sr, device, what="STOI"):
    """Fresh buffers of the forward launches on `rows` pairs of n samples at sr; every refusal names `what` (sehip.loss.stoi_loss keeps
    a set of its own, apart from the metric's cache)."""
    device = canonical_device(device)
    p, q = stoi_ratio(sr, what)
    n10 = n if p == q else stoi_out_len(n, sr)
    if n10 < STOI_FRAME:
        raise SehipError(f"{what}: {n} samples at {sr} Hz are {n10} samples at 10 kHz; one frame needs {STOI_FRAME}")
    if not 1 <= rows <= STOI_MAX_ROWS:
        raise SehipError(f"{what}: {rows} rows outside [1, {STOI_MAX_ROWS}]")
    frames = lib().sehip_stoi_frames(n10)
    if frames <= 0:
        raise SehipError(f"{what}: {n10} samples at 10 kHz are more than the kernels index")
    f32 = dict(device=device, dtype=torch.float32)
    i32 = dict(device=device, dtype=torch.int32)
    return dict(p=p, q=q, n10=n10, frames=frames,
                table=None if p == q else stoi_resample_table(sr, device),
                sig=None if p == q else torch.empty(2 * rows, n10, **f32),
                level=torch.empty(rows, frames, **f32), kept=torch.empty(rows, **i32), src=torch.empty(rows, frames, **i32),
                tob=torch.empty(2, rows, STOI_BANDS, max(frames - 1, 1), **f32),
                partial=[torch.empty(rows, lib().sehip_stoi_segment_blocks(frames, ext), **f32) for ext in (0, 1)])


def stoi_workspace(rows, n, sr, device):
    """The buffers of one STOI call on `rows` pairs of n samples at sr, cached per (rows, n, sr, device): a call allocates nothing but its
    result, so it can be captured into a graph."""
    device = canonical_device(device)
    return _stoi_workspaces.get((rows, n, int(sr), device), stoi_buffers, rows, n, sr, device)


def stoi_forward(r, e, ws, extended, d, out):
    """The forward launches on the contiguous float32 rows r (clean) and e (estimate) [rows, n] with the buffers `ws`: d [rows] and the
    mean `out` are written; kept, src and tob (and, off 10 kHz, the resampled pair in sig) stay in `ws`."""
    rows, n = r.shape
    st, n10, frames = stream(), ws["n10"], ws["frames"]
    if ws["sig"] is None:
        clean, est = ptr(r), ptr(e)
    else:
        table, p, q, L = ws["table"]
        call("sehip_stoi_resample", ptr(r), ptr(e), rows, n, ptr(table), p, q, L, ptr(ws["sig"]), st)
        clean, est = ptr(ws["sig"]), ptr(ws["sig"][rows:])
    call("sehip_stoi_levels", clean, rows, n10, ptr(ws["level"]), st)
    call("sehip_stoi_select", ptr(ws["level"]), rows, frames, ptr(ws["kept"]), ptr(ws["src"]), st)
    call("sehip_stoi_bands", clean, est, rows, n10, ptr(ws["kept"]), ptr(ws["src"]), ptr(ws["tob"]), st)
    call("sehip_stoi_segments", ptr(ws["tob"]), ptr(ws["kept"]), rows, frames, int(bool(extended)),
         ptr(ws["partial"][int(bool(extended))]), ptr(d), ptr(out), st)


def _stoi_launch(reference, estimation, sr, extended, what):
    """-> (d [rows], mean 0-dim, workspace) of a fresh result pair; every check comes before the first launch"""
    if not torch.is_tensor(reference) or not torch.is_tensor(estimation):
        raise SehipError(f"{what}: needs device tensors")
    require_gpu(reference, what)
    require_gpu(estimation, what)
    if reference.shape != estimation.shape:
        raise ValueError(f"{what}: shapes differ: {tuple(reference.shape)} vs {tuple(estimation.shape)}")
    if reference.requires_grad or estimation.requires_grad:
        raise SehipError(f"{what}: the metric is not differentiable; detach the inputs")
    if reference.dim() < 1 or reference.numel() == 0:
        raise SehipError(f"{what}: empty input of shape {tuple(reference.shape)}")
    n = int(reference.shape[-1])
    rows = reference.numel() // n
    ws = stoi_workspace(rows, n, sr, reference.device)
    with torch.no_grad():
        r = reference.reshape(rows, n).contiguous().float()
        e = estimation.reshape(rows, n).contiguous().float()
        d = torch.empty(rows, device=r.device, dtype=torch.float32)
        out = torch.empty((), device=r.device, dtype=torch.float32)
        stoi_forward(r, e, ws, extended, d, out)
    return d, out, ws


def stoi_rows(reference, estimation, sr=16000, extended=False):
    """The value per row: device tensors [..., T] of equal shape -> [rows] float32 on the device (rows = every axis but the last)."""
    return _stoi_launch(reference, estimation, sr, extended, "stoi_rows")[0]


def STOI(reference, estimation, sr=16000, extended=False):
    """reference (clean) / estimation: device tensors [..., T] of equal shape -> 0-dim device tensor (float32): the mean over all rows of
    stoi(clean, estimate, sr, extended), as src/metric.py:126-144 means over batch and channel.

    Both signals are resampled to 10 kHz, the frames more than 40 dB below the clean signal's loudest frame leave both (so a
    zero-padded tail needs no lengths argument), and the one-third-octave envelopes of 30-frame segments are correlated; a row with
    fewer than 30 frames left gives 1e-5.  Nothing is read back and nothing but the result is allocated: the call can be captured
    into a graph on one stream.  Not differentiable: inputs that require grad are refused."""
    return _stoi_launch(reference, estimation, sr, extended, "STOI")[1]
