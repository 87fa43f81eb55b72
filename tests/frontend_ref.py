"""float64 restatements of the front-end every training step passes through (csrc/stft.hip, csrc/mask.h, csrc/loss.hip), for
tests/test_frontend_ref_host.py (CPU) and tests/test_gpu_frontend_edges.py (GPU).  No GPU is used here.

STFT / iSTFT: the exact cos / -sin basis in float64 times the fp32 window VALUES cast to double, so the reference reads the operands the
kernel read; synthesis = pinv(basis).T * window as oracle/dccrn_oracle.py:stft_bases before its cast to fp32; window energy of
sehip.ops.inv_window_energy (the fp32 table the kernel reads).  Every sum comes with the sum of its absolute addends: the same linear map
applied to the absolute values of the basis and of the operand.
SI-SNR, PIT, psa, l1 / mse: the oracle's own functions on tensors of the requested dtype, float64 for the reference and float32 for the
deviation of the CPU oracle from it, which is what the GPU gates are measured against."""
from itertools import permutations

import numpy as np
import torch
import torch.nn.functional as F

from oracle import dccrn_oracle as O
from oracle import loss_oracle as LO
from oracle import pit_oracle
from sehip import ops

D = torch.float64
FFT = 512
NBIN = FFT // 2 + 1
SDR_EPS = float(np.finfo(np.float32).eps)
_BASES = {}


def bases(win, win_type="hann"):
    """(analysis [514, win], synthesis [514, win], window [win]) in float64; the window is the fp32 one of sehip.ops.window_of"""
    key = (win, str(win_type))
    if key not in _BASES:
        n = np.arange(win, dtype=np.int64)[None, :]
        k = np.arange(NBIN, dtype=np.int64)[:, None]
        m = (k * n) % FFT                                                       # the angle reduced exactly, on the integers
        ang = 2.0 * np.pi * m.astype(np.float64) / FFT
        # cos / sin are exactly 0 at the odd / even multiples of pi / 2: the imaginary parts of DC and Nyquist have NO addends, and a
        # transform of real input leaves exactly 0 there
        basis = np.concatenate([np.where(m % 256 == 128, 0.0, np.cos(ang)), np.where(m % 256 == 0, 0.0, -np.sin(ang))], 0)
        w = ops.window_of(win_type, win).astype(np.float64)
        _BASES[key] = tuple(torch.from_numpy(a) for a in (basis * w[None], np.linalg.pinv(basis).T * w[None], w))
    return _BASES[key]


def window32(win, win_type="hann"):
    return torch.from_numpy(ops.window_of(win_type, win))


def frames_of(n, win, hop):
    return ops.stft_frames(n, win, hop)


def _bins(x):
    """[B, T, 514] (real rows | imaginary rows) -> [B, T, 257, 2]"""
    return torch.stack([x[..., :NBIN], x[..., NBIN:]], -1)


def stft(wav, win, hop, win_type="hann"):
    """wav [B, N] -> (spec [B, T, 257, 2], the absolute addends of every bin, same shape), float64"""
    a, _, _ = bases(win, win_type)
    pad = win - hop
    fr = F.pad(wav.to(D), [pad, pad]).unfold(-1, win, hop)                      # [B, T, win]
    return _bins(fr @ a.t()), _bins(fr.abs() @ a.abs().t())


def apply_mask(spec, mask, mode):
    """spec [B, T, 257, 2], mask [B, T, 256, 2] (bins 1..256; DC is zero padding) -> estimate [B, T, 514]: the tail of
    oracle/dccrn_oracle.py:dccrn_forward, modes 0 'E', 1 'C', 2 'R'"""
    real, imag = spec[..., 0], spec[..., 1]
    m_r, m_i = F.pad(mask[..., 0], [1, 0]), F.pad(mask[..., 1], [1, 0])
    if mode == 0:
        mags = torch.sqrt(real ** 2 + imag ** 2 + 1e-8)
        phase = torch.atan2(imag, real)
        m_mag = (m_r ** 2 + m_i ** 2) ** 0.5
        m_phase = torch.atan2(m_i / (m_mag + 1e-8), m_r / (m_mag + 1e-8))
        est_mag = torch.tanh(m_mag) * mags
        er, ei = est_mag * torch.cos(phase + m_phase), est_mag * torch.sin(phase + m_phase)
    elif mode == 1:
        er, ei = real * m_r - imag * m_i, real * m_i + imag * m_r
    else:
        er, ei = real * m_r, imag * m_i
    return torch.cat([er, ei], -1)


def inv_energy(win, hop, frames, length, win_type="hann"):
    return torch.from_numpy(ops.inv_window_energy(win, hop, frames, length, win_type))


def istft(spec, mask, win, hop, length, mode, win_type="hann"):
    """-> (waveform [B, length] BEFORE the clamp, the absolute addends of every sample): synthesis, overlap-add, the trim of win - hop
    samples, [:length], times the fp32 reciprocal window energy.  Differentiable with respect to mask."""
    _, s, _ = bases(win, win_type)
    est = apply_mask(spec.to(D), mask.to(D), mode)
    inv = inv_energy(win, hop, spec.shape[1], length, win_type).to(D)
    pad = win - hop

    def synth(e, basis):
        return F.conv_transpose1d(e.transpose(1, 2), basis[:, None, :], stride=hop)[:, 0, pad:pad + length] * inv
    return synth(est, s), synth(est.detach().abs(), s.abs())


def clamp(y):
    return torch.clamp(y, -1.0, 1.0)


def istft_dmask(spec, mask, dwav, win, hop, length, mode, win_type="hann", clamped=True):
    """d <clamp(istft), dwav> / d mask [B, T, 256, 2] in float64.  clamped=False is the backward that ignores the clamp (the planted
    fault of the host test).  Mode 0 yields NaN exactly where a mask element pair is (0, 0): the caller replaces those."""
    m = mask.to(D).clone().requires_grad_(True)
    y, _ = istft(spec, m, win, hop, length, mode, win_type)
    ((clamp(y) if clamped else y) * dwav.to(D)).sum().backward()
    return m.grad


def near_limit(y, width=1e-4):
    """samples whose float64 value lies within `width` of +-1: an fp32 sample may fall on the other side of the limit there"""
    return (y.abs() - 1.0).abs() < width


# ----------------------------------------------------------------------------------------------------------------------------------
# losses
# ----------------------------------------------------------------------------------------------------------------------------------
def sisnr(est, ref, upstream=1.0, dtype=D):
    """est / ref [rows, n] -> (loss, per-row SI-SNR in dB [rows], d (upstream * loss) / d est) in `dtype`"""
    e = est.to(dtype).clone().requires_grad_(True)
    r = ref.to(dtype)
    loss = O.loss_sisdr(e, r)
    (upstream * loss).backward()
    rows = torch.stack([O.si_snr(e[i:i + 1].detach(), r[i:i + 1]) for i in range(e.shape[0])])
    return loss.detach(), rows, e.grad


def pit(est, ref, upstream=1.0, dtype=D, force_perm=None):
    """est / ref [B, S, C, n] -> (loss, perm [S] with perm[j] = the estimated speaker matched with target j, the S x S matrix of
    batch-mean pair losses, d (upstream * loss) / d est) in `dtype`; the permutation is pit_oracle's, or the forced one (the planted
    fault of the host test)"""
    e = est.to(dtype).clone().requires_grad_(True)
    t = ref.to(dtype)
    if force_perm is None:
        loss, comb, _ = pit_oracle.pit(e, t, O.loss_sisdr)
    else:
        comb = [(i, j) for j, i in enumerate(force_perm)]
        loss = sum(O.loss_sisdr(e[:, i], t[:, j]) for i, j in comb) / len(comb)
    (upstream * loss).backward()
    s = e.shape[1]
    with torch.no_grad():          # (pit_oracle keeps its matrix in fp32 whatever the input type)
        m = torch.stack([torch.stack([O.loss_sisdr(e[:, i], t[:, j]) for j in range(s)]) for i in range(s)])
    perm = [i for i, _ in sorted(comb, key=lambda p: p[1])]
    return loss.detach(), perm, m, e.grad


def pit_gap(m):
    """the two smallest permutation losses (mean over the matched pairs) of a pair matrix: (gap in dB, best permutation)"""
    s = m.shape[0]
    tot = sorted((float(sum(m[pe[j], j] for j in range(s))) / s, pe) for pe in permutations(range(s)))
    return (tot[1][0] - tot[0][0] if len(tot) > 1 else float("inf")), list(tot[0][1])


def si_sdr_metric(reference, estimation, dtype=np.float64):
    """the formula of tests/test_gpu_evaluate.py:test_si_sdr_metric_on_device in `dtype` (eps = float32 machine epsilon in both)"""
    reference, estimation = np.asarray(reference, dtype=dtype), np.asarray(estimation, dtype=dtype)
    eps = dtype(SDR_EPS)
    energy = np.sum(reference ** 2, axis=-1, keepdims=True)
    scale = np.sum(estimation * reference, axis=-1, keepdims=True) / (energy + eps)
    proj = scale * reference
    noise = estimation - proj
    ratio = np.mean(np.sum(proj ** 2, axis=-1) / (np.sum(noise ** 2, axis=-1) + eps))
    return float(10 * np.log10(ratio + eps))


def pointwise(name, x, y, upstream=1.0, dtype=D):
    """l1 / mse with reduction 'mean' -> (loss, d (upstream * loss) / d x)"""
    xr = x.to(dtype).clone().requires_grad_(True)
    loss = (F.l1_loss if name == "l1" else F.mse_loss)(xr, y.to(dtype))
    (upstream * loss).backward()
    return loss.detach(), xr.grad


def psa(enh, tgt, mix, upstream=1.0, dtype=D):
    """-> (loss, d (upstream * loss) / d enh); NaN where an enhanced element is (0, 0), as in tests/test_psa_loss.py"""
    e = enh.to(dtype).clone().requires_grad_(True)
    loss = LO.psa_loss(e, tgt.to(dtype), mix.to(dtype))
    (upstream * loss).backward()
    return loss.detach(), e.grad


# ----------------------------------------------------------------------------------------------------------------------------------
# gates on fp32 results: the bound is measured, a multiple of the fp32 CPU oracle's own deviation from float64 on the same inputs
# ----------------------------------------------------------------------------------------------------------------------------------
MARGIN = 4.0                  # a different summation order and, for the SI-SNR gradient, the factor up to 2.9 between two fp32 forms
REL_FLOOR = 1e-6              # the tolerance of tests/test_gpu_frontend.py:test_l1_mse_losses


def _f64(v):
    """flat float64 tensor of a tensor or a Python number (which torch.as_tensor alone would round to fp32)"""
    return (v.detach() if torch.is_tensor(v) else torch.as_tensor(v, dtype=D)).double().reshape(-1)


def rel(a, b):
    a, b = _f64(a), _f64(b)
    return float((a - b).norm() / (b.norm() + 1e-300))


def rel_bound(oracle32, want):
    """max(4 x the norm-relative deviation of the fp32 CPU oracle from the float64 `want`, 1e-6)"""
    return max(MARGIN * rel(oracle32, want), REL_FLOOR)


def check_rel(what, got, want, bound):
    """norm-relative error of got against the float64 `want` within `bound` (rel_bound of the TRUE reference)"""
    err = rel(got, want)
    print(f"{what}: {err:.3e} (bound {bound:.3e})")
    assert err <= bound, (what, err, bound)
    return err


def db_bound(oracle32, want, sum_tol):
    """per value in dB: max(4 x the fp32 oracle's deviation, 4.343 * 2 * sum_tol) -- two sums of squares at sum_tol carried through
    10 log10 (d dB = 4.343 d ratio / ratio)"""
    o, w = _f64(oracle32), _f64(want)
    return torch.clamp(MARGIN * (o - w).abs(), min=4.343 * 2 * sum_tol)


def check_db(what, got, want, bound):
    got, want = _f64(got), _f64(want)
    err = (got - want).abs()
    i = int((err / bound).argmax())
    print(f"{what}: largest deviation {float(err.max()):.3e} dB; closest to its bound {float(err[i]):.3e} of {float(bound[i]):.3e} dB")
    assert bool((err <= bound).all()), (what, float(err[i]), float(bound[i]))
    return float(err.max())


# ----------------------------------------------------------------------------------------------------------------------------------
# the inputs of the GPU tests: built here so that the host test can assert their conditions without a GPU
# ----------------------------------------------------------------------------------------------------------------------------------
CLAMP_GEOM = (400, 100)
CLAMP_SHAPE = (2, 4000)
CLAMP_AMPLITUDE = {0: 1.5, 1: 1.0, 2: 1.0}


def clamp_inputs(mode):
    """(wav [2, 4000], mask [2, T, 256, 2], upstream gradient): a waveform and a mask near one, so that a large share of the samples
    clamp.  Mode 0 ('E': tanh(|m|) < 1 shrinks every bin) takes a larger waveform."""
    g = torch.Generator().manual_seed(40 + mode)
    b, n = CLAMP_SHAPE
    t = frames_of(n, *CLAMP_GEOM)
    wav = CLAMP_AMPLITUDE[mode] * torch.randn(b, n, generator=g)
    mask = 0.3 * torch.randn(b, t, 256, 2, generator=g)
    mask[..., 0] += 1.0
    if mode == 2:
        mask[..., 1] += 1.0
    return wav, mask, torch.randn(b, n, generator=g)


SILENT_ROWS = slice(40, 44)


def silence_inputs():
    """(wav [2, 4000] with a zeroed run inside and a zeroed tail in each row, mask [2, 43, 256, 2] with bins 40..43 zero, upstream)"""
    g = torch.Generator().manual_seed(50)
    wav = 0.3 * torch.randn(2, 4000, generator=g)
    wav[0, 900:2300] = 0.0
    wav[0, 3800:] = 0.0
    wav[1, 1500:2600] = 0.0
    wav[1, 3700:] = 0.0
    mask = 0.7 * torch.randn(2, frames_of(4000, 400, 100), 256, 2, generator=g)
    mask[:, :, SILENT_ROWS] = 0.0
    return wav, mask, torch.randn(2, 4000, generator=g)


def silent_frames(wav, win, hop):
    """number of all-zero frames per batch row"""
    pad = win - hop
    return [int(v) for v in (F.pad(wav, [pad, pad]).unfold(-1, win, hop).abs().sum(-1) == 0).sum(-1)]


def noisy_pair(shape, seed, noise=0.3):
    g = torch.Generator().manual_seed(seed)
    ref = torch.randn(shape, generator=g)
    return ref + noise * torch.randn(shape, generator=g), ref


SNR_DB = (0.0, 20.0, 40.0, 60.0)


def snr_batch(n=4001, seed=60):
    """one row per entry of SNR_DB: est = ref + noise at that signal-to-noise ratio"""
    g = torch.Generator().manual_seed(seed)
    ref = torch.randn(len(SNR_DB), n, generator=g)
    noise = torch.randn(len(SNR_DB), n, generator=g)
    scale = torch.tensor([10.0 ** (-s / 20.0) for s in SNR_DB])[:, None] * ref.norm(dim=-1, keepdim=True) / noise.norm(dim=-1, keepdim=True)
    return ref + scale * noise, ref


def silent_row_batch(n=300, seed=61):
    """rows: normal, all-zero target, all-zero estimate, normal, both all-zero"""
    est, ref = noisy_pair((5, n), seed)
    ref[1] = 0.0
    est[2] = 0.0
    est[4] = 0.0
    ref[4] = 0.0
    return est, ref


PIT_SHAPES = [(3, 1, 2, 301), (3, 2, 2, 301), (2, 4, 1, 257), (1, 6, 1, 300), (35, 2, 2, 64)]


def pit_inputs(shape, seed=70):
    """est = the targets cyclically shifted by one speaker + 0.3 randn"""
    g = torch.Generator().manual_seed(seed + shape[1] + shape[0])
    tgt = torch.randn(shape, generator=g)
    return torch.roll(tgt, 1, dims=1) + 0.3 * torch.randn(shape, generator=g), tgt


def pit_tie_inputs():
    g = torch.Generator().manual_seed(71)
    tgt = torch.randn(2, 2, 1, 128, generator=g)
    est = tgt[:, :1] + 0.3 * torch.randn(2, 1, 1, 128, generator=g)
    return est.repeat(1, 2, 1, 1).contiguous(), tgt


def bf16_truncate(x):
    """fp32 -> bf16 by dropping the low 16 bits (the planted fault: a pack that does not round)"""
    bits = x.float().contiguous().view(torch.int32) & -65536
    return bits.view(torch.float32).bfloat16()


def bf16_half_ulp_up(x):
    """a float64 reference moved away from zero by half a bf16 ulp: against it a correctly rounded value sits where a truncated one sits
    against the true reference"""
    x = x.double()
    e = torch.floor(torch.log2(x.abs().clamp(min=1e-300)))
    return x + torch.sign(x) * 2.0 ** (e - 8)


CAP_FLOATS = 4194304          # above it the forward grids of l1 / mse / psa stop at 1024 blocks and the backward grids at 2048
POINTWISE_SIZES = [1, 255, 257, CAP_FLOATS + 4099]
PSA_SIZES = [1, 255, 257, (CAP_FLOATS + 4099) // 2]              # complex elements; the last is 2 099 201


def pointwise_inputs(n, equal_share=0.0, seed=80):
    """x, y [n]; with equal_share that share of the elements exactly equal (l1: gradient 0 there)"""
    g = torch.Generator().manual_seed(seed + n % 1000)
    x, y = torch.randn(n, generator=g), torch.randn(n, generator=g)
    if equal_share:
        same = torch.rand(n, generator=g) < equal_share
        y[same] = x[same]
    return x, y


def psa_inputs(n, seed=90):
    g = torch.Generator().manual_seed(seed + n % 1000)
    return tuple(torch.randn(n, 2, generator=g) for _ in range(3))


def oracle32(wav, mask, dwav, win, hop, length, mode):
    """the fp32 CPU oracle (oracle/dccrn_oracle.py conv_stft / conv_istft, autograd) on the layouts of the C ABI:
    (spec [B, T, 257, 2], clamped waveform [B, length], d <waveform, dwav> / d mask [B, T, 256, 2]); it stands in for the kernel in the
    host test"""
    analysis, synthesis, window = O.stft_bases(win, FFT)
    ref = O.conv_stft(wav[:, None], analysis, win, hop)                         # [B, 514, T]
    spec = torch.stack([ref[:, :NBIN], ref[:, NBIN:]], -1).permute(0, 2, 1, 3).contiguous()
    m = mask.clone().requires_grad_(True)
    est = apply_mask(spec, m, mode)                                             # [B, T, 514]
    out = clamp(O.conv_istft(est.transpose(1, 2), synthesis, window, win, hop, length)[:, 0])
    (out * dwav).sum().backward()
    return spec, out.detach(), m.grad
