"""Thin tensor-level wrappers over the C ABI (one function per exported op).

These do shape bookkeeping and output allocation only; all arithmetic happens in libsehip.
"""
import numpy as np
import torch

from . import _lib
from ._cache import CaptureAwareCache, canonical_device
from ._lib import call, ptr, stream, require_gpu

BF16 = torch.bfloat16


def hann_periodic(n):
    """scipy.signal.get_window('hann', n, fftbins=True) (src/model/dccrn.py:653)."""
    k = np.arange(n, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * k / n)).astype(np.float32)


def window_of(win_type, n):
    """The window of init_kernels (src/model/dccrn.py:650-653): ones for None / 'None', else
    scipy.signal.get_window(win_type, n, fftbins=True).  'hann' / 'hamming' in closed form, anything else through scipy."""
    if win_type is None or win_type == "None":
        return np.ones(n, dtype=np.float32)
    if win_type == "hann":
        return hann_periodic(n)
    k = np.arange(n, dtype=np.float64)
    if win_type == "hamming":
        return (0.54 - 0.46 * np.cos(2.0 * np.pi * k / n)).astype(np.float32)
    try:
        from scipy.signal import get_window
        return np.asarray(get_window(win_type, n, fftbins=True), dtype=np.float64).astype(np.float32)
    except Exception as e:      # an unknown name, or scipy absent
        raise _lib.SehipError(f"sehip DCCRN: win_type={win_type!r}: {e}")


def inv_window_energy(win, hop, frames, length, win_type="hann"):
    """1 / (overlap-added window^2 + 1e-8), trimmed like src/model/dccrn.py:733-745."""
    w2 = window_of(win_type, win).astype(np.float64) ** 2
    total = (frames - 1) * hop + win
    e = np.zeros(total, dtype=np.float64)
    for t in range(frames):
        e[t * hop:t * hop + win] += w2
    e = e.astype(np.float32) + np.float32(1e-8)
    pad = win - hop
    return (np.float32(1.0) / e[pad:pad + length]).astype(np.float32)


def stft_frames(n, win, hop):
    return (n + 2 * (win - hop) - win) // hop + 1


def stft_fwd(wav, window, win, hop, fft=512):
    """wav [B,N] fp32 -> (spec [B,T,257,2] fp32, enc_in [B,T,256,2] bf16)."""
    require_gpu(wav, "stft_fwd")
    b, n = wav.shape
    t = stft_frames(n, win, hop)
    spec = torch.empty(b, t, 257, 2, device=wav.device, dtype=torch.float32)
    enc = torch.empty(b, t, 256, 2, device=wav.device, dtype=BF16)
    call("sehip_stft_fwd", ptr(wav), ptr(window), b, n, win, hop, fft, ptr(spec), ptr(enc), stream())
    return spec, enc


def istft_fwd(spec, mask, window, inv_coff, win, hop, length, mode=0, fft=512):
    """spec [B,T,257,2], mask [B,T,256,2] fp32 -> wav [B,length] (clamped to [-1,1])."""
    require_gpu(spec, "istft_fwd")
    b, t = spec.shape[:2]
    frames = torch.empty(b, t, win, device=spec.device, dtype=torch.float32)
    wav = torch.empty(b, length, device=spec.device, dtype=torch.float32)
    call("sehip_istft_fwd", ptr(spec), ptr(mask), ptr(window), ptr(inv_coff), b, t, win, hop, fft, length, mode,
         ptr(frames), ptr(wav), stream())
    return wav


def istft_bwd(dwav, wav, spec, mask, window, inv_coff, win, hop, length, mode=0, fft=512):
    """-> d mask [B,T,256,2] bf16."""
    b, t = spec.shape[:2]
    dmask = torch.empty(b, t, 256, 2, device=spec.device, dtype=BF16)
    call("sehip_istft_bwd", ptr(dwav), ptr(wav), ptr(spec), ptr(mask), ptr(window), ptr(inv_coff), b, t, win, hop, fft,
         length, mode, ptr(dmask), stream())
    return dmask


def sisnr_fwd(est, ref):
    """est/ref [R,N] fp32 -> (loss scalar tensor = -mean si_snr, rowstat [R,4])."""
    require_gpu(est, "sisnr_fwd")
    r, n = est.shape
    rowstat = torch.empty(r, 4, device=est.device, dtype=torch.float32)
    loss = torch.empty(1, device=est.device, dtype=torch.float32)
    call("sehip_sisnr_fwd", ptr(est), ptr(ref), r, n, ptr(rowstat), ptr(loss), stream())
    return loss, rowstat


def sisnr_bwd(est, ref, rowstat, upstream=None):
    r, n = est.shape
    dest = torch.empty_like(est)
    call("sehip_sisnr_bwd", ptr(est), ptr(ref), ptr(rowstat), ptr(upstream), r, n, ptr(dest), stream())
    return dest


def sisnr_pit_fwd(est, ref):
    """est/ref [B,S,C,N] fp32 contiguous -> (loss [1], rowstat [S*S,B*C,4], pairloss [S*S], perm [S] int32): the
    permutation-invariant SI-SNR of src/loss.py:58-100 (batch-level permutation, first minimum in itertools order)."""
    require_gpu(est, "sisnr_pit_fwd")
    b, s, c, n = est.shape
    rowstat = torch.empty(s * s, b * c, 4, device=est.device, dtype=torch.float32)
    pairloss = torch.empty(s * s, device=est.device, dtype=torch.float32)
    perm = torch.empty(s, device=est.device, dtype=torch.int32)
    loss = torch.empty(1, device=est.device, dtype=torch.float32)
    call("sehip_sisnr_pit_fwd", ptr(est), ptr(ref), b, s, c, n, ptr(rowstat), ptr(pairloss), ptr(perm), ptr(loss), stream())
    return loss, rowstat, pairloss, perm


def sisnr_pit_bwd(est, ref, rowstat, perm, upstream=None):
    b, s, c, n = est.shape
    dest = torch.empty_like(est)
    call("sehip_sisnr_pit_bwd", ptr(est), ptr(ref), ptr(rowstat), ptr(perm), ptr(upstream), b, s, c, n, ptr(dest), stream())
    return dest


def pit_pointwise_blocks(b, s, c, n):
    """Records of the pair-matrix workspace for est / ref [B,S,C,N]: partials is [blocks, S*S] fp32."""
    blocks = _lib.lib().sehip_pit_pointwise_blocks(b, s, c, n)
    if blocks <= 0:
        raise _lib.SehipError(f"pit_pointwise: bad shape (B={b} S={s} C={c} n={n}; 1 <= S <= 6, positive sizes)")
    return blocks


def pit_pointwise_fwd(est, ref, mode, partials=None):
    """est/ref [B,S,C,N] fp32 contiguous, mode 0 = l1 / 1 = mse -> (loss [1], pairloss [S*S], perm [S] int32): the
    permutation-invariant l1 / mse of src/loss.py:58-100 in one pass over the data.  partials [pit_pointwise_blocks(...), S*S]
    fp32 is workspace (allocated here when None; pass a cached one to keep the call free of allocations)."""
    require_gpu(est, "pit_pointwise_fwd")
    b, s, c, n = est.shape
    if partials is None:
        partials = torch.empty(pit_pointwise_blocks(b, s, c, n), s * s, device=est.device, dtype=torch.float32)
    pairloss = torch.empty(s * s, device=est.device, dtype=torch.float32)
    perm = torch.empty(s, device=est.device, dtype=torch.int32)
    loss = torch.empty(1, device=est.device, dtype=torch.float32)
    call("sehip_pit_pointwise_fwd", ptr(est), ptr(ref), b, s, c, n, mode, ptr(partials), ptr(pairloss), ptr(perm), ptr(loss), stream())
    return loss, pairloss, perm


def pit_pointwise_bwd(est, ref, perm, mode, upstream=None):
    b, s, c, n = est.shape
    dest = torch.empty_like(est)
    call("sehip_pit_pointwise_bwd", ptr(est), ptr(ref), ptr(perm), ptr(upstream), b, s, c, n, mode, ptr(dest), stream())
    return dest


# ---- julius.resample_frac (julius 0.2.7 ResampleFrac with its defaults), csrc/resample.hip -------------------------------------
RESAMPLE_ZEROS, RESAMPLE_ROLLOFF = 24, 0.945
_resample_tables = {}      # (reduced old, reduced new, device) -> (table, width, old, new)


def resample_out_len(n, old_sr, new_sr):
    """floor(n * new_sr / old_sr): the length julius.resample_frac returns for n samples."""
    m = _lib.lib().sehip_resample_out_len(int(n), int(old_sr), int(new_sr))
    if m < 0:
        raise _lib.SehipError(f"resample: bad length / ratio (n={n}, {old_sr} -> {new_sr})")
    return int(m)


def resample_kernels(old_sr, new_sr, device="cpu"):
    """-> (table fp32 [new][2 * width + old], width, old, new) with old / new the reduced ratio: the windowed-sinc interpolation
    kernels of julius's ResampleFrac (zeros=24, rolloff=0.945, squared-cosine window, each phase normalised to unit sum), built on
    the host in float32 torch arithmetic and cached per reduced ratio and device."""
    old_sr, new_sr = int(old_sr), int(new_sr)
    if old_sr <= 0 or new_sr <= 0:
        raise _lib.SehipError(f"resample_kernels: sample rates must be positive, got {old_sr} -> {new_sr}")
    g = int(np.gcd(old_sr, new_sr))
    old, new = old_sr // g, new_sr // g
    device = torch.device(device)
    key = (old, new, str(device))
    hit = _resample_tables.get(key)
    if hit is not None:
        return hit
    host = _resample_tables.get((old, new, "cpu"))
    if host is None:
        sr = min(new, old) * RESAMPLE_ROLLOFF
        width = int(np.ceil(RESAMPLE_ZEROS * old / sr))
        idx = torch.arange(-width, width + old, dtype=torch.float32)
        rows = []
        for i in range(new):
            t = (-i / new + idx / old) * sr
            t = t.clamp(-RESAMPLE_ZEROS, RESAMPLE_ZEROS) * np.pi
            window = torch.cos(t / RESAMPLE_ZEROS / 2) ** 2
            one = torch.ones_like(t)
            k = torch.where(t == 0, one, torch.sin(t) / torch.where(t == 0, one, t)) * window
            rows.append(k / k.sum())
        host = (torch.stack(rows).contiguous(), width, old, new)
        _resample_tables[(old, new, "cpu")] = host
    if device.type != "cpu":
        host = (host[0].to(device), host[1], old, new)
        _resample_tables[key] = host
    return host


def resample_rows(raw, row_off, rows, old_sr, new_sr, out, out_off):
    """The flat-buffer call: `rows` rows raw[row_off[r] .. row_off[r + 1]) (device fp32 / int64) are written to
    out[out_off[r] .. out_off[r + 1]), floor(len * new / old) samples each; the caller sizes out / out_off (resample_out_len)."""
    require_gpu(raw, "resample_rows")
    table, width, old, new = resample_kernels(old_sr, new_sr, raw.device)
    call("sehip_resample_frac", ptr(raw), ptr(row_off), int(rows), ptr(table), old, new, width, ptr(out), ptr(out_off), stream())
    return out


def resample_frac(x, old_sr, new_sr):
    """julius.resample_frac(x, old_sr, new_sr) (output_length=None, full=False: what src/dataset.py uses) for a CUDA fp32 tensor
    [..., T] -> [..., floor(T * new / old)]."""
    if int(old_sr) == int(new_sr):
        return x
    if not torch.is_tensor(x) or not x.is_cuda:
        raise _lib.SehipError(f"resample_frac: needs a CUDA tensor (got {getattr(x, 'device', type(x))}); there is no CPU fallback")
    if x.dtype != torch.float32:
        raise _lib.SehipError(f"resample_frac: fp32 only, got {x.dtype}")
    if x.dim() < 1 or x.shape[-1] == 0:
        raise _lib.SehipError(f"resample_frac: needs at least one sample along the last axis, got shape {tuple(x.shape)}")
    T = int(x.shape[-1])
    rows = x.numel() // T
    m = resample_out_len(T, old_sr, new_sr)
    out = torch.empty(*x.shape[:-1], m, dtype=torch.float32, device=x.device)
    if rows == 0 or m == 0:
        return out
    xc = x.contiguous()
    row_off = torch.arange(rows + 1, dtype=torch.int64, device=x.device) * T
    out_off = torch.arange(rows + 1, dtype=torch.int64, device=x.device) * m
    table, width, old, new = resample_kernels(old_sr, new_sr, x.device)
    call("sehip_resample_frac", ptr(xc), ptr(row_off), rows, ptr(table), old, new, width, ptr(out), ptr(out_off), stream())
    return out


_mrl_windows = CaptureAwareCache()     # (n_fft, win_length, device) -> the periodic hann of win_length centred in n_fft zeros, fp32 [n_fft]


def _mrl_window_make(n_fft, win_length, device):
    host = torch.zeros(n_fft, dtype=torch.float32)
    lp = (n_fft - win_length) // 2
    host[lp:lp + win_length] = torch.hann_window(win_length, periodic=True, dtype=torch.float64).float()
    return host.to(device)


def mrl_window(n_fft, win_length, device):
    """torch.stft's window for (n_fft, win_length): hann_window(win_length) (periodic, rounded once from float64) behind
    (n_fft - win_length) // 2 zeros, as a cached device table the kernels of csrc/mrstft_loss.hip read."""
    n_fft, win_length, device = int(n_fft), int(win_length), canonical_device(device)
    return _mrl_windows.get((n_fft, win_length, device), _mrl_window_make, n_fft, win_length, device)


def mrl_check(resolutions, rows, n, what="mrstft"):
    """The refusals of csrc/mrstft_loss.hip for `resolutions` ((n_fft, hop, win_length), ...) on rows x n samples, before any launch;
    -> the resolutions as a host int32 tensor [R, 3]."""
    try:
        res = [tuple(int(v) for v in r) for r in resolutions]
    except (TypeError, ValueError):
        raise _lib.SehipError(f"{what}: resolutions must be (n_fft, hop, win_length) triples, got {resolutions!r}")
    if any(len(r) != 3 for r in res):
        raise _lib.SehipError(f"{what}: resolutions must be (n_fft, hop, win_length) triples, got {resolutions!r}")
    host = torch.tensor(res, dtype=torch.int32).reshape(-1, 3)
    status = _lib.lib().sehip_mrl_check(len(res), ptr(host) if res else None, int(rows), int(n))
    if status != 0:
        raise _lib.SehipError(f"{what}: {_lib.lib().sehip_last_error().decode()}")
    return host


def stft_magnitudes(x, n_fft, hop, win_length):
    """M = sqrt(max(|torch.stft(x, n_fft, hop, win_length, hann_window(win_length), center=True, pad_mode='reflect')|^2, 1e-7)) for a
    device tensor x [..., n] -> [rows, n_fft / 2 + 1, 1 + n // hop] fp32 (rows = every axis but the last): the magnitudes the
    multi-resolution STFT loss is taken on, written out."""
    if not torch.is_tensor(x):
        raise _lib.SehipError("stft_magnitudes: needs a device tensor")
    require_gpu(x, "stft_magnitudes")
    if x.dim() < 1 or x.numel() == 0:
        raise _lib.SehipError(f"stft_magnitudes: empty input of shape {tuple(x.shape)}")
    n = int(x.shape[-1])
    rows = x.numel() // n
    mrl_check([(n_fft, hop, win_length)], rows, n, "stft_magnitudes")
    xc = x.reshape(rows, n).contiguous().float()
    out = torch.empty(rows, int(n_fft) // 2 + 1, 1 + n // int(hop), device=x.device, dtype=torch.float32)
    call("sehip_mrl_magnitudes", ptr(xc), rows, n, int(n_fft), int(hop), int(win_length), ptr(mrl_window(n_fft, win_length, x.device)),
         ptr(out), stream())
    return out
