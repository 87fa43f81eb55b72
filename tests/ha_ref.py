"""Float64 numpy restatement of the hearing-aid stage (the reference's src/ha/amplifier.py, src/ha/compressor.py and
src/audio.py:33-61), written for this project: filter design, FIR, level detector, gain recurrence, clip and the gradient with respect
to the signal.  It also holds the fixture list that tools/gen_golden_ha.py and the tests share.

    design(nfir, fs, hl, cfs)          nfir + 1 float64 taps in filter order (the reference stores them reversed)
    fir(x, h) / fir_adjoint(d, h, n)   out[m] = sum_k h[k] x[m - k]  /  dx[i] = sum_k h[k] d[i + k]
    level(z, W)                        sqrt(mean(z^2 over the W samples ending at i) + 1e-8)
    gain_loop(lv, cfg)                 the reference's sample-by-sample recurrence, c_{-1} = 1
    gain_blocks(lv, cfg)               the same recurrence vectorised (cumulative products over blocks); tools/bench_ha.py's CPU path
    chain(signal, taps, cfg, clip)     FIR -> compressor -> tanh for rows [R, n]; returns a dict of every stage
    chain_grad(G, stages, taps, clip)  gradient of <out, G> with the gain held constant, as the reference's autograd sees it
"""
import numpy as np

EPS = 1e-8
AUD = np.array([250, 500, 1000, 2000, 4000, 6000], dtype=np.float64)
BIAS = np.array([-17, -8, 1, -1, -2, -2], dtype=np.float64)

# ---- fixtures ---------------------------------------------------------------------------------------------------------------------
CFS = [250, 500, 1000, 2000, 3000, 4000, 6000, 8000]
AUDIOGRAMS = {
    "docstring": [25, 40, 55, 65, 65, 70, 65, 60],      # the example of src/ha/amplifier.py's docstring (left ear)
    "zeros": [0, 0, 0, 0, 0, 0, 0, 0],                  # no loss: the pure delay
    "severe": [50, 60, 70, 75, 80, 80, 85, 85],         # hl(500) + hl(1000) + hl(2000) = 205 > 180: the second xave formula
    "mild_low": [0, 5, 10, 20, 30, 40, 50, 50],         # the gains at 250 and 500 Hz come out negative and clip to 0
}
TAPS_CASES = ((220, 44100), (32, 16000))
CHAIN = dict(fs=16000, nfir=32, shape=(2, 1, 2, 4000), seed=11,
             compressor=dict(threshold=0.35, attenuation=0.1, attack=50, release=1000, rms_buffer_size=0.064),   # src/ha/conf/config.yaml
             audiogram={"audiogram_cfs": CFS, "audiogram_levels_l": [25, 40, 55, 65, 65, 70, 65, 60],
                        "audiogram_levels_r": [20, 30, 55, 65, 65, 75, 60, 50]})
MIN_MARGIN = 1e-7                                        # a fixture's float64 level stays this far (relative) from the threshold


def chain_signal():
    """[2, 1, 2, 4000] fp32: seeded noise under a slow envelope, loud enough after the NAL-R gain to cross the threshold both ways"""
    b, s, e, n = CHAIN["shape"]
    rng = np.random.RandomState(CHAIN["seed"])
    t = np.arange(n) / CHAIN["fs"]
    x = np.empty(CHAIN["shape"], dtype=np.float32)
    for r in range(b * s * e):
        env = (0.5 + 0.5 * np.sin(2 * np.pi * (5 + r) * t + r)) ** 2
        x.reshape(-1, n)[r] = (0.05 * rng.standard_normal(n) * env).astype(np.float32)
    return x


def chain_upstream():
    b, s, e, n = CHAIN["shape"]
    rng = np.random.RandomState(CHAIN["seed"] + 1)
    return (rng.standard_normal((b, s, e, n + CHAIN["nfir"])) / np.sqrt(b * s * e * n)).astype(np.float32)


def compressor_config(fs, attack, release, threshold, attenuation, rms_buffer_size):
    """per-sample coefficients and the window, as CompressorTorch.__init__ derives them"""
    return dict(attack=1 / (attack / 1000) / fs, release=1 / (release / 1000) / fs, threshold=float(threshold),
                attenuation=float(attenuation), W=int(rms_buffer_size * fs))


# ---- NAL-R design -----------------------------------------------------------------------------------------------------------------
def _interp(x_new, x, y):
    x, y, x_new = np.asarray(x, np.float64), np.asarray(y, np.float64), np.asarray(x_new, np.float64)
    if x.shape != y.shape or x_new.min() < x.min() or x_new.max() > x.max():
        raise ValueError("interpolation outside the given frequencies")
    o = np.argsort(x, kind="stable")
    return np.interp(x_new, x[o], y[o])


def sampled_response_fir(order, freq, mag):
    """frequency-sampling design: straight segments between the breakpoints on 513 (or 2^k + 1) grid points, linear phase of
    order / 2 samples, Hermitian extension, inverse FFT, Hamming window"""
    taps = order + 1
    npt = 512 if taps < 1024 else int(2 ** np.ceil(np.log2(taps)))
    grid = npt + 1
    freq = np.array(freq, np.float64)
    freq[0], freq[-1] = 0.0, 1.0
    resp = np.zeros(grid)
    resp[0] = mag[0]
    start = 0
    for i in range(len(freq) - 1):
        if freq[i + 1] == freq[i]:
            lap = int(np.fix(npt / 25))
            start = int(np.ceil(start - lap / 2))
            stop = start + lap - 1
        else:
            stop = int(np.fix(freq[i + 1] * grid)) - 1
        j = np.arange(start, stop + 1)
        w = np.zeros(len(j)) if start == stop else (j - start) / (stop - start)
        resp[start:stop + 1] = w * mag[i + 1] + (1 - w) * mag[i]
        start = stop + 1
    half = resp * np.exp(-1j * np.pi * 0.5 * order * np.arange(grid) / (grid - 1))
    full = np.concatenate((half, np.conj(half[grid - 2:0:-1])))
    return np.real(np.fft.ifft(full))[:taps] * np.hamming(taps)


def design(nfir, fs, hl, cfs=None):
    cfs = [250, 500, 1000, 2000, 3000, 6000] if cfs is None else cfs
    hl = _interp(AUD, cfs, hl)
    if hl.max() <= 0:
        d = np.zeros(nfir + 1)
        d[nfir // 2] = 1.0
        return d
    t3 = hl[1] + hl[2] + hl[3]
    xave = 0.05 * t3 if t3 <= 180 else 9.0 + 0.116 * (t3 - 180)
    gdb = np.maximum(xave + 0.31 * hl + BIAS, 0.0)
    fmax = 0.5 * fs
    cfreq = np.linspace(0, nfir, nfir + 1) / nfir
    gain_db = _interp(fmax * cfreq, np.concatenate(([0.0], AUD, [fmax])), np.concatenate(([gdb[0]], gdb, [gdb[-1]])))
    return sampled_response_fir(nfir, cfreq, 10.0 ** (gain_db / 20.0))


# ---- signal path ------------------------------------------------------------------------------------------------------------------
def fir(x, h):
    """x [n] -> [n + K - 1]"""
    return np.convolve(np.asarray(x, np.float64), np.asarray(h, np.float64), mode="full")


def fir_adjoint(d, h, n):
    """d [n + K - 1] -> [n]: dx[i] = sum_k h[k] d[i + k]"""
    out = np.correlate(np.asarray(d, np.float64), np.asarray(h, np.float64), mode="valid")
    assert out.shape == (n,)
    return out


def fir_abs(x, h):
    """sum_k |h[k]| |x[m - k]|: the magnitude the fp32 dot-product bound scales with"""
    return np.convolve(np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(h, np.float64)), mode="full")


def level(z, W, direct=False):
    """sqrt(mean(z^2 over the W samples ending at i, zeros before the row) + 1e-8); direct=True sums every window on its own (the
    reference's np.convolve), otherwise a difference of float64 prefix sums"""
    sq = np.asarray(z, np.float64) ** 2
    if direct:
        ss = np.convolve(np.concatenate((np.zeros(W - 1), sq)), np.ones(W), mode="valid")
    else:
        p = np.concatenate(([0.0], np.cumsum(sq)))
        i = np.arange(1, len(sq) + 1)
        ss = np.maximum(p[i] - p[np.maximum(i - W, 0)], 0.0)
    return np.sqrt(ss / W + EPS)


def margin(lv, threshold):
    """smallest relative distance of the level from the threshold"""
    return float(np.min(np.abs(lv - threshold)) / threshold)


def maps(lv, cfg):
    """(a_i, b_i) of c_i = a_i c_{i-1} + b_i"""
    above = lv > cfg["threshold"]
    target = lv * cfg["attenuation"] + (1 - cfg["attenuation"]) * cfg["threshold"]
    a = np.where(above, 1 - cfg["attack"], 1 - cfg["release"])
    b = np.where(above, target * cfg["attack"], cfg["release"])
    return a, b


def gain_loop(lv, cfg):
    a, b = maps(lv, cfg)
    out = np.empty(len(lv))
    c = 1.0
    for i, (ai, bi) in enumerate(zip(a.tolist(), b.tolist())):
        c = c * ai + bi
        out[i] = c
    return out


def gain_blocks(lv, cfg, block=512):
    """c_i = A_i (c_start + sum_{j <= i} b_j / A_j) with A the cumulative product of a over a block short enough that A stays far from
    underflow; the blocks are chained by their last value"""
    a, b = maps(lv, cfg)
    amin = float(a.min())
    if 0 < abs(amin) < 1:
        block = int(max(1, min(block, 200.0 / -np.log(abs(amin)))))
    elif amin == 0 or abs(amin) > 1:
        block = 1
    out = np.empty(len(lv))
    c = 1.0
    for s in range(0, len(lv), block):
        A = np.cumprod(a[s:s + block])
        out[s:s + block] = A * (c + np.cumsum(b[s:s + block] / A))
        c = out[min(s + block, len(lv)) - 1]
    return out


def chain(rows, taps, cfg, soft_clip=True, loop=True, direct_level=False):
    """rows [R, n] (any float dtype), taps [K] or [R, K] float64 in filter order -> dict of float64 stages, all [R, n + K - 1]:
    fir, level, gain (float64), gain32 (its fp32 rounding, as the reference casts it), prod = fir * gain32, out"""
    rows = np.asarray(rows, np.float64)
    taps = np.asarray(taps, np.float64)
    y = np.stack([fir(r, taps if taps.ndim == 1 else taps[i]) for i, r in enumerate(rows)])
    lv = np.stack([level(r, cfg["W"], direct=direct_level) for r in y])
    g = np.stack([(gain_loop if loop else gain_blocks)(r, cfg) for r in lv])
    g32 = g.astype(np.float32).astype(np.float64)
    prod = y * g32
    return dict(fir=y, level=lv, gain=g, gain32=g32, prod=prod, out=np.tanh(prod) if soft_clip else prod)


def compress(rows, cfg, soft_clip=False, loop=True, direct_level=False):
    """the compressor alone on rows [R, n]: the chain with the identity filter"""
    return chain(rows, np.ones(1), cfg, soft_clip=soft_clip, loop=loop, direct_level=direct_level)


def chain_grad(G, stages, taps, n, soft_clip=True):
    """d<out, G>/d(rows) with the gain held constant: FIR^T(G * (1 - out^2) * gain32)"""
    G = np.asarray(G, np.float64)
    taps = np.asarray(taps, np.float64)
    d = G * stages["gain32"] * ((1 - stages["out"] ** 2) if soft_clip else 1.0)
    return np.stack([fir_adjoint(r, taps if taps.ndim == 1 else taps[i], n) for i, r in enumerate(d)])
