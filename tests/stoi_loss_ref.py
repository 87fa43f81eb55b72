"""tests/stoi_ref.py restated in torch with autograd: the oracle of sehip.loss.stoi_loss (csrc/stoi_loss.hip).

Every step follows tests/stoi_ref.py (which stays the oracle of the VALUE: tests/test_stoi_loss_host.py checks that the two agree to
1e-12); the constants, the resampling table, `levels` and `select` are imported from it.  `dtype=torch.float64` is the oracle;
`dtype=torch.float32` restates the same steps in single precision, one sample of the rounding error an fp32 implementation has.

The conventions that make the gradient total:
  * the kept-frame set is chosen from the clean signal by numpy (`levels` / `select`) and is a constant of the backward pass;
  * `gsqrt`: sqrt with derivative 0 at exactly 0 (a band of an all-zero estimate frame, a zero segment norm);
  * `tmin`: min(a, b) passes the gradient to the branch that was taken, `a` on a tie;
  * a row with fewer than 30 spectra has the value 1e-5 and the gradient exactly zero;
  * the clean signal receives no gradient."""
import numpy as np
import torch

import stoi_ref as R


class _GuardedSqrt(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a):
        s = torch.sqrt(a)
        ctx.save_for_backward(s)
        return s

    @staticmethod
    def backward(ctx, g):
        s, = ctx.saved_tensors
        return torch.where(s > 0, g / (2 * torch.where(s > 0, s, torch.ones_like(s))), torch.zeros_like(g))


def gsqrt(a):
    return _GuardedSqrt.apply(a)


def tmin(a, b):
    return torch.where(a <= b, a, b)


def window(dtype):
    return torch.from_numpy(R.window(np.float64)).to(dtype)


def resample(y, sr, dtype):
    """stoi_ref.resample as a dense gather: out[m] = sum_i tab[r][i] y[k - i] with zeros outside y"""
    if int(sr) == R.FS:
        return y
    p, q, L, tab = R.phase_table(sr)
    n, kt = y.shape[0], tab.shape[1]
    base = np.arange(R.out_len(n, sr), dtype=np.int64) * q + L
    idx = (base // p)[:, None] - np.arange(kt)[None, :]
    ok = torch.from_numpy((idx >= 0) & (idx < n))
    taps = torch.from_numpy(tab[base % p]).to(dtype)
    vals = torch.where(ok, y[torch.from_numpy(np.clip(idx, 0, n - 1))], torch.zeros((), dtype=dtype))
    return (taps * vals).sum(dim=1)


def compact(sig, src, dtype):
    """the kept windowed frames overlap-added at hop 128: (K + 1) * 128 samples"""
    win = window(dtype)
    k = len(src)
    out = torch.zeros((k + 1) * R.HOP, dtype=dtype)
    if k == 0:
        return out
    frames = win * sig[torch.from_numpy(np.asarray(src, dtype=np.int64)[:, None] * R.HOP + np.arange(R.N_FRAME)[None, :])]
    pos = torch.from_numpy((np.arange(k)[:, None] * R.HOP + np.arange(R.N_FRAME)[None, :]).reshape(-1))
    return out.index_add(0, pos, frames.reshape(-1))


def spectra(sig, dtype):
    """[T][257] complex: frames at 0, 128, ... while i < len - 256, windowed again, zero-padded to 512"""
    starts = np.arange(0, len(sig) - R.N_FRAME, R.HOP)
    if len(starts) == 0:
        return torch.zeros(0, R.NFFT // 2 + 1, dtype=torch.complex128 if dtype == torch.float64 else torch.complex64)
    frames = window(dtype) * sig[torch.from_numpy(starts[:, None] + np.arange(R.N_FRAME)[None, :])]
    return torch.fft.rfft(frames, n=R.NFFT, dim=1)


def band_magnitudes(spec):
    """[15][T]: the guarded sqrt of the band's summed |X|^2"""
    pw = spec.real ** 2 + spec.imag ** 2
    return torch.stack([gsqrt(pw[:, a:b].sum(dim=1)) for a, b in R.BANDS])


def segments(tob):
    return tob.unfold(1, R.N, 1).permute(1, 0, 2)                 # [M][15][30]


def _norm(a, dim):
    return gsqrt((a * a).sum(dim=dim, keepdim=True))


def correlate(x_tob, y_tob, extended=False, detail=False):
    """stoi_ref.correlate; with detail=True (plain variant) also the mask of the clipped cells and the relative distance
    |c y - 6.62 x| / (6.62 x) of every cell from the branch point"""
    eps = R.EPS
    xs, ys = segments(x_tob), segments(y_tob)
    m = xs.shape[0]
    if extended:
        def rc(a):
            a = a - a.mean(dim=2, keepdim=True)
            a = a / (_norm(a, 2) + eps)
            a = a - a.mean(dim=1, keepdim=True)
            return a / (_norm(a, 1) + eps)
        return (rc(xs) * rc(ys)).sum() / (R.N * m)
    c = _norm(xs, 2) / (_norm(ys, 2) + eps)
    cy, cx = ys * c, xs * (1 + 10 ** (-R.BETA / 20))
    yp = tmin(cy, cx)
    yp = yp - yp.mean(dim=2, keepdim=True)
    xc = xs - xs.mean(dim=2, keepdim=True)
    d = ((yp / (_norm(yp, 2) + eps)) * (xc / (_norm(xc, 2) + eps))).sum() / (R.NUMBAND * m)
    if detail:
        with torch.no_grad():
            return d, (cy > cx), (cy - cx).abs() / cx.clamp_min(1e-300)
    return d


def kept_frames(x, sr):
    """src of the clean row x (numpy, float64 at sr): the constant of the backward pass"""
    e, _ = R.levels(R.resample(x, sr, np.float64), np.float64)
    return R.select(e)[1]


def stoi_steps(x, y, sr, extended=False, dtype=torch.float64, src=None):
    """the intermediates of one (clean, estimate) pair: x numpy (no gradient), y a torch leaf of `dtype`; 'd' is the value"""
    x = np.asarray(x, dtype=np.float64)
    src = kept_frames(x, sr) if src is None else src
    st = {"src": src, "y10": resample(y, sr, dtype)}
    with torch.no_grad():
        x10 = resample(torch.from_numpy(x).to(dtype), sr, dtype)
        st["x_tob"] = band_magnitudes(spectra(compact(x10, src, dtype), dtype))
    st["yc"] = compact(st["y10"], src, dtype)
    st["y_tob"] = band_magnitudes(spectra(st["yc"], dtype))
    st["T"] = st["x_tob"].shape[1]
    if st["T"] < R.N:
        st["d"] = torch.full((), R.TOO_FEW_FRAMES, dtype=dtype) + 0 * y.sum()      # the value is a constant: gradient exactly zero
    else:
        st["d"] = correlate(st["x_tob"], st["y_tob"], extended)
    return st


def stoi_value_and_grad(x, y, sr, extended=False, dtype=torch.float64):
    """(d, d d / d y) of one pair as (float, numpy float64 array)"""
    yt = torch.from_numpy(np.asarray(y, dtype=np.float64)).to(dtype).requires_grad_(True)
    d = stoi_steps(x, yt, sr, extended, dtype)["d"]
    g, = torch.autograd.grad(d, yt)
    return float(d.detach()), g.double().numpy()


def loss_and_grad(xs, ys, sr, extended=False, dtype=torch.float64):
    """stoi_loss of rows: (-mean d, its gradient [rows][n], the per-row values d)"""
    vals, grads = zip(*(stoi_value_and_grad(x, y, sr, extended, dtype) for x, y in zip(xs, ys)))
    return -float(np.mean(vals)), -np.stack(grads) / len(vals), np.asarray(vals)
