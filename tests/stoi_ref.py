"""STOI / ESTOI (Taal et al. 2011; Jensen & Taal 2016) restated in numpy from the published algorithm, step by step as `pystoi` transcribes the
authors' MATLAB: the oracle of sehip.metric.STOI.  `pystoi` itself is not available to this project's tests, so parity with it is by this
restatement only: if it turns out to differ in a constant, this file and that constant change.

Every step is a function of its own and returns its intermediate.  `dtype=np.float64` is the oracle; `dtype=np.float32` restates the same
steps in single precision (taps, window and products rounded to fp32, complex64 transform through torch.fft), one sample of the rounding
error an fp32 implementation has.  No scipy here (tests/test_stoi_host.py checks `resample` against scipy where scipy exists)."""
from math import gcd

import numpy as np

FS = 10000
N_FRAME = 256
HOP = 128
NFFT = 512
NUMBAND = 15
MINFREQ = 150
N = 30
BETA = -15.0
DYN_RANGE = 40
EPS = np.finfo(float).eps
TOO_FEW_FRAMES = 1e-5
BANDS = [(7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55), (55, 69), (69, 87), (87, 109),
         (109, 138), (138, 174), (174, 219)]


def am_signal(n, sr, seed=0):
    """test signal: a seeded sum of five amplitude-modulated sines plus noise"""
    r = np.random.RandomState(seed)
    t = np.arange(n) / sr
    s = np.zeros(n)
    for _ in range(5):
        f, fm = r.uniform(200, 3500), r.uniform(2, 8)
        s += r.uniform(0.2, 1) * (0.6 + 0.4 * np.sin(2 * np.pi * fm * t + r.uniform(0, 6))) * np.sin(2 * np.pi * f * t + r.uniform(0, 6))
    return 0.1 * s + 0.003 * r.randn(n)


# ---- step 1: resample to 10 kHz -----------------------------------------------------------------------------------------
def ratio(sr):
    g = gcd(FS, int(sr))
    return FS // g, int(sr) // g


def resample_filter(sr):
    """(p, q, L, w): the reduced ratio, the half length and the normalised Kaiser-windowed sinc of 2 L + 1 taps."""
    p, q = ratio(sr)
    fc = 1.0 / (2 * max(p, q))
    L = int(np.ceil((60 - 8) / (28.714 * fc / 10)))
    t = np.arange(-L, L + 1)
    h = np.kaiser(2 * L + 1, 0.1102 * (60 - 8.7)) * 2 * p * fc * np.sinc(2 * fc * t)
    return p, q, L, h / np.sum(h)


def out_len(n, sr):
    p, q = ratio(sr)
    return -((-n * p) // q)


def phase_table(sr):
    """tab[r][i] = p * w[r + i p] (zero past the filter), Kt = 2 L // p + 1 taps per output: out[m] = sum_i tab[r][i] x[k - i] with
    k = (m q + L) // p, r = (m q + L) % p."""
    p, q, L, w = resample_filter(sr)
    kt = 2 * L // p + 1
    tab = np.zeros((p, kt))
    for r in range(p):
        taps = w[r::p]
        tab[r, :len(taps)] = p * taps
    return p, q, L, tab


def resample(x, sr, dtype=np.float64, chunk=4096, absolute=False):
    """out[m] = p sum_k x[k] w[L + m q - k p], m < ceil(n p / q): scipy.signal.resample_poly(x, p, q, window=w).
    absolute=True: p sum_k |x[k]| |w[...]|, the magnitude an fp32 dot-product bound is stated in."""
    x = np.asarray(x, dtype=np.float64)
    if int(sr) == FS:
        return x.astype(dtype)
    p, q, L, tab = phase_table(sr)
    if absolute:
        x, tab = np.abs(x), np.abs(tab)
    n, kt = len(x), tab.shape[1]
    xs, tab = x.astype(dtype), tab.astype(dtype)
    out = np.empty(out_len(n, sr), dtype=dtype)
    for m0 in range(0, len(out), chunk):
        base = np.arange(m0, min(m0 + chunk, len(out)), dtype=np.int64) * q + L
        k = base // p
        idx = k[:, None] - np.arange(kt)[None, :]
        ok = (idx >= 0) & (idx < n)
        prod = tab[base % p] * np.where(ok, xs[np.clip(idx, 0, n - 1)], dtype(0))
        out[m0:m0 + len(base)] = prod.sum(axis=1, dtype=dtype)
    return out


# ---- step 2: silent-frame removal ---------------------------------------------------------------------------------------
def window(dtype=np.float64):
    return np.hanning(N_FRAME + 2)[1:-1].astype(dtype)


def frame_count(n):
    return (n - N_FRAME) // HOP + 1 if n >= N_FRAME else 0


def levels(x, dtype=np.float64):
    """e_f = 20 log10(||win * frame_f|| + EPS) of the frames at 0, 128, ... while i <= len - 256."""
    x = np.asarray(x, dtype=dtype)
    win = window(dtype)
    f = frame_count(len(x))
    frames = np.stack([win * x[i * HOP:i * HOP + N_FRAME] for i in range(f)])
    nrm = np.sqrt(np.sum(frames * frames, axis=1, dtype=dtype))
    return (dtype(20) * np.log10(nrm + dtype(EPS))).astype(dtype), frames


def select(e):
    """(mask, src): the frames within DYN_RANGE dB of the loudest one, and their indices."""
    mask = (np.max(e) - e.dtype.type(DYN_RANGE) - e) < 0
    return mask, np.nonzero(mask)[0]


def threshold_margin(e):
    """distance in dB of every frame's level from the keep / drop threshold (positive: kept)"""
    return e - (np.max(e) - DYN_RANGE)


def compact(sig, src, dtype=np.float64):
    """the kept windowed frames of `sig`, overlap-added at hop 128: (K + 1) * 128 samples"""
    sig = np.asarray(sig, dtype=dtype)
    win = window(dtype)
    out = np.zeros((len(src) + 1) * HOP, dtype=dtype)
    for j, f in enumerate(src):
        out[j * HOP:j * HOP + N_FRAME] += win * sig[f * HOP:f * HOP + N_FRAME]
    return out


# ---- step 3: spectra ------------------------------------------------------------------------------------------------------
def spectra(sig, dtype=np.float64):
    """[T][257] complex: frames at 0, 128, ... while i < len - 256 (exclusive), windowed again, zero-padded to 512"""
    sig = np.asarray(sig, dtype=dtype)
    win = window(dtype)
    starts = range(0, len(sig) - N_FRAME, HOP)
    if len(starts) == 0:
        return np.zeros((0, NFFT // 2 + 1), dtype=np.complex128 if dtype == np.float64 else np.complex64)
    frames = np.stack([win * sig[i:i + N_FRAME] for i in starts])
    if dtype == np.float64:
        return np.fft.rfft(frames, n=NFFT, axis=1)
    import torch
    return torch.fft.rfft(torch.from_numpy(np.ascontiguousarray(frames)), n=NFFT, dim=1).numpy()


# ---- step 4: one-third-octave bands ---------------------------------------------------------------------------------------
def thirdoct(fs=FS, nfft=NFFT, num_bands=NUMBAND, min_freq=MINFREQ):
    """the [lo, hi) bin ranges: the band edges min_freq 2^((2k -+ 1) / 6) snapped to the nearest bin"""
    f = np.linspace(0, fs, nfft + 1)[:nfft // 2 + 1]
    k = np.arange(num_bands, dtype=float)
    lo = min_freq * np.power(2.0, (2 * k - 1) / 6)
    hi = min_freq * np.power(2.0, (2 * k + 1) / 6)
    return [(int(np.argmin(np.square(f - a))), int(np.argmin(np.square(f - b)))) for a, b in zip(lo, hi)]


def band_magnitudes(spec, dtype=np.float64):
    """[15][T]: sqrt of the band's summed |X|^2"""
    pw = (spec.real.astype(dtype) ** 2 + spec.imag.astype(dtype) ** 2)
    return np.stack([np.sqrt(np.sum(pw[:, a:b], axis=1, dtype=dtype)) for a, b in BANDS]).astype(dtype)


# ---- step 6: segments -------------------------------------------------------------------------------------------------------
def segments(tob):
    t = tob.shape[1]
    return np.stack([tob[:, m - N:m] for m in range(N, t + 1)])          # [M][15][30]


def _norm(a, axis, dtype):
    return np.sqrt(np.sum(a * a, axis=axis, keepdims=True, dtype=dtype))


def correlate(x_tob, y_tob, extended=False, dtype=np.float64):
    eps = dtype(EPS)
    xs, ys = segments(x_tob.astype(dtype)), segments(y_tob.astype(dtype))
    m = xs.shape[0]
    if extended:
        def rc(a):
            a = a - np.mean(a, axis=2, keepdims=True, dtype=dtype)
            a = a / (_norm(a, 2, dtype) + eps)
            a = a - np.mean(a, axis=1, keepdims=True, dtype=dtype)
            return a / (_norm(a, 1, dtype) + eps)
        return dtype(np.sum(rc(xs) * rc(ys), dtype=dtype) / dtype(N * m))
    c = _norm(xs, 2, dtype) / (_norm(ys, 2, dtype) + eps)
    yp = np.minimum(ys * c, xs * dtype(1 + 10 ** (-BETA / 20)))
    yp = yp - np.mean(yp, axis=2, keepdims=True, dtype=dtype)
    xs = xs - np.mean(xs, axis=2, keepdims=True, dtype=dtype)
    yp = yp / (_norm(yp, 2, dtype) + eps)
    xs = xs / (_norm(xs, 2, dtype) + eps)
    return dtype(np.sum(yp * xs, dtype=dtype) / dtype(NUMBAND * m))


# ---- the whole metric -------------------------------------------------------------------------------------------------------
def stoi_steps(x, y, sr, extended=False, dtype=np.float64):
    """every intermediate of one (clean, estimate) pair as a dict; 'd' is the value"""
    st = {"x10": resample(x, sr, dtype), "y10": resample(y, sr, dtype)}
    st["levels"], _ = levels(st["x10"], dtype)
    st["mask"], st["src"] = select(st["levels"])
    xc, yc = compact(st["x10"], st["src"], dtype), compact(st["y10"], st["src"], dtype)
    st["x_tob"] = band_magnitudes(spectra(xc, dtype), dtype)
    st["y_tob"] = band_magnitudes(spectra(yc, dtype), dtype)
    st["T"] = st["x_tob"].shape[1]
    st["d"] = dtype(TOO_FEW_FRAMES) if st["T"] < N else correlate(st["x_tob"], st["y_tob"], extended, dtype)
    return st


def stoi(x, y, sr, extended=False, dtype=np.float64):
    return float(stoi_steps(x, y, sr, extended, dtype)["d"])


def STOI(reference, estimation, sr=16000, extended=False, dtype=np.float64):
    """mean over all rows of [..., T] arrays, as src/metric.py:126-144 means over batch and channel"""
    r = np.asarray(reference).reshape(-1, np.shape(reference)[-1])
    e = np.asarray(estimation).reshape(-1, np.shape(estimation)[-1])
    return float(np.mean([stoi(a, b, sr, extended, dtype) for a, b in zip(r, e)]))
