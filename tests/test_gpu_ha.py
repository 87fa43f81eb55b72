"""Hearing-aid stage on the device (csrc/hearing_aid.hip, sehip/ha, sehip/audio.py) against tests/ha_ref.py in float64.

FIR, op-local: K in {1, 2, 33, 221, 1025}, rows of n in {1, K - 1, K, K + 1, 3 tiles + 5} (tile from sehip_last_kernel), two tap
    sets with the rows alternating between them; every sample within the fp32 dot-product bound (K + 2) * 2^-24 * sum_k |h_k| |x_k|
    (tests/test_gpu_resample.py's), guard words, run-to-run bits; the adjoint with the same bound and <Ax, y> = <x, A^T y>.
Compressor, op-local: six (W, n) cases of 4 rows each; the test's own float64 level must keep 1e-7 (relative) from the threshold
    (an input check, never a mask); gain within 2^-23 relative of fp32(float64 recurrence), out within |z c| 2^-22; rows that stay
    below / above the threshold; run-to-run bits; deterministic mode on and off.
tanh: |out - tanh64(z64 c64)| <= |z c| 2^-22 + T.  T is an allowance for the device's tanh, not derivable on the host; it started
    at 2^-21.  Measured on an MI355X over the six cases: the device's tanh on its own fp32 product is at most 9.04e-08 (1.52 x 2^-24)
    from float64's, the whole |out - tanh64(z64 c64)| at most 1.07e-07.  T_TANH = 2^-22 = 2.38e-07 is 2.6 x
    the former, inside the 4 x that the gate may keep.
Chain: amplify_torch on the recorded reference call (tests/golden/ha_chain.npz) at 5e-5, the right-ear quirk, the backward pass
    against ha_ref's gradient, and one forward + backward captured into a graph and replayed."""
import os

import numpy as np
import pytest
import torch

import ha_ref as R
from util import rel_err

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64
ACT_TOL = 5e-5
T_TANH = 2.0 ** -22
CHAIN_MARGIN = 1e-5      # chain tests feed the compressor the DEVICE's fp32 FIR output, the reference its float64 one: the levels
#                          differ by up to the FIR's fp32 error (~K 2^-24 ~ 2e-6 relative at K = 33), so the input must keep further away
_cache = {}


def _kernel():
    from sehip import _lib
    return _lib.lib().sehip_last_kernel().decode()


def _field(kernel, name):
    return int(kernel.split(name + "=")[1].split()[0])


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- FIR ------------------------------------------------------------------------------------------------------------------------
FIR_K = (1, 2, 33, 221, 1025)
FIR_ROWS = 4


def _fir_raw(fn, x, taps, row_set, n, out_cols):
    """the C entry on a guarded output buffer -> ([rows, out_cols] on the host, guard intact?)"""
    from sehip._lib import call, ptr, stream
    rows, (F, K) = x.shape[0], taps.shape
    out = torch.full((rows * out_cols + GUARD,), 12345.0, device="cuda")
    call(fn, ptr(x), rows, n, ptr(taps), F, K, ptr(row_set), ptr(out), stream())
    torch.cuda.synchronize()
    return out[:rows * out_cols].reshape(rows, out_cols).cpu(), bool((out[rows * out_cols:] == 12345.0).all())


def _fir_case(K):
    if K not in _cache:
        g = torch.Generator().manual_seed(100 + K)
        taps = torch.randn(2, K, generator=g) / K ** 0.5
        _cache[K] = (taps, g)
    return _cache[K]


@pytest.mark.parametrize("K", FIR_K)
def test_fir_and_adjoint_against_float64(K):
    from sehip.ha import fir_adjoint, fir_apply
    taps, g = _fir_case(K)
    t64 = taps.double().numpy()
    d_taps = taps.cuda()
    row_set = torch.tensor([r % 2 for r in range(FIR_ROWS)], dtype=torch.int32)
    d_set = row_set.cuda()
    # the tile size, from a first tiny call
    _fir_raw("sehip_ha_fir_fwd", torch.zeros(1, 1, device="cuda"), d_taps, None, 1, K)
    tile = _field(_kernel(), "tile")
    lens = sorted({n for n in (1, K - 1, K, K + 1, 3 * tile + 5) if n >= 1})
    worst = 0.0
    for n in lens:
        x = 0.3 * torch.randn(FIR_ROWS, n, generator=g) + 0.05
        y = torch.randn(FIR_ROWS, n + K - 1, generator=g)
        out, guard = _fir_raw("sehip_ha_fir_fwd", x.cuda(), d_taps, d_set, n, n + K - 1)
        kernel = _kernel()
        assert guard, f"wrote past the output (K={K}, n={n})"
        assert kernel.startswith("ha_fir_fwd") and _field(kernel, "K") == K and _field(kernel, "tiles") == -(-(n + K - 1) // tile)
        if n == lens[-1]:
            assert _field(kernel, "tiles") > 3, kernel            # the long row really spans several tiles
        dx, guard = _fir_raw("sehip_ha_fir_adj", y.cuda(), d_taps, d_set, n, n)
        assert guard, f"adjoint wrote past its output (K={K}, n={n})"
        assert _kernel().startswith("ha_fir_adj")
        for r in range(FIR_ROWS):
            h = t64[r % 2]
            for got, want, mag in ((out[r], R.fir(x[r].numpy(), h), R.fir_abs(x[r].numpy(), h)),
                                   (dx[r], R.fir_adjoint(y[r].numpy(), h, n), R.fir_adjoint(np.abs(y[r].numpy()), np.abs(h), n))):
                err = np.abs(got.double().numpy() - want)
                bound = (K + 2) * 2.0 ** -24 * mag
                worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
                assert bool((err <= bound).all()), (K, n, r, int(err.argmax()), float(err.max()), float(bound[err.argmax()]))
        # <A x, y> = <x, A^T y> in float64 on the device's own results
        lhs, rhs = float((out.double() * y.double()).sum()), float((x.double() * dx.double()).sum())
        scale = float((out.double().abs() * y.double().abs()).sum())
        assert abs(lhs - rhs) <= 1e-6 * scale, (K, n, lhs, rhs)
        # two runs, and the tensor interface, give the same bits; a NULL row_set means set 0
        again, _ = _fir_raw("sehip_ha_fir_fwd", x.cuda(), d_taps, d_set, n, n + K - 1)
        assert _bits(out, again)
        assert _bits(fir_apply(x.cuda(), d_taps, d_set).cpu(), out) and _bits(fir_adjoint(y.cuda(), d_taps, n, d_set).cpu(), dx)
        zero_set, _ = _fir_raw("sehip_ha_fir_fwd", x.cuda(), d_taps, None, n, n + K - 1)
        assert _bits(zero_set[0::2], out[0::2])
        # a row's bits do not depend on its neighbours or on the grid: row 2 alone
        alone, _ = _fir_raw("sehip_ha_fir_fwd", x[2:3].cuda(), d_taps, None, n, n + K - 1)
        assert _bits(alone[0], out[2])
    print(f"[ha fir K={K}] n={lens} tile={tile}: worst error / bound = {worst:.4f}")


def test_apply_is_conv1d_with_the_stored_taps():
    """NALRTorch.apply(nalr, wav) with the REVERSED stored taps = torch.conv1d(wav, nalr, padding=nfir) (evaluated on the host in
    float64), for S = 1 and, rows being independent here, for S = 3; differentiable: the gradient is the adjoint"""
    from sehip.ha import NALRTorch
    amp = NALRTorch(32, 16000)
    nalr = amp.build(R.AUDIOGRAMS["docstring"], R.CFS)
    g = torch.Generator().manual_seed(3)
    for S in (1, 3):
        wav = 0.1 * torch.randn(2, S, 700, generator=g)
        w = wav.cuda().requires_grad_(True)
        out = amp.apply(nalr.cuda(), w)
        assert tuple(out.shape) == (2, S, 732)
        want = torch.conv1d(wav.double().reshape(2 * S, 1, 700), nalr.double(), padding=32).reshape(2, S, 732)
        assert rel_err(out.detach().cpu(), want) < ACT_TOL
        G = torch.randn(2, S, 732, generator=g)
        out.backward(G.cuda())
        wd = wav.double().requires_grad_(True)
        (torch.conv1d(wd.reshape(2 * S, 1, 700), nalr.double(), padding=32).reshape(2, S, 732) * G.double()).sum().backward()
        assert rel_err(w.grad.cpu(), wd.grad) < ACT_TOL


# ---- compressor -----------------------------------------------------------------------------------------------------------------
#            W     n      fs
COMP_CASES = ((1024, 4032, 16000), (1024, 20000, 16000), (64, 3000, 16000), (2822, 44320, 44100), (1, 700, 16000), (1024, 300, 16000))
SETTINGS = R.CHAIN["compressor"]                                  # threshold 0.35, attenuation 0.1, attack 50 ms, release 1000 ms


def _compressor(W, fs):
    from sehip.ha import CompressorTorch
    comp = CompressorTorch(fs=fs, **SETTINGS)
    comp.win_len = W
    cfg = R.compressor_config(fs, **SETTINGS)
    cfg["W"] = W
    return comp, cfg


def _comp_case(W, n, fs):
    """4 rows of seeded randn * 1.2 * (0.5 + 0.5 sin(2 pi (3 + r) t + r))^2 and their float64 stages: computed once, shared"""
    key = ("comp", W, n)
    if key not in _cache:
        g = torch.Generator().manual_seed(7000 + W + n)
        t = torch.arange(n, dtype=torch.float64) / fs
        z = torch.stack([(torch.randn(n, generator=g).double() * 1.2 * (0.5 + 0.5 * torch.sin(2 * np.pi * (3 + r) * t + r)) ** 2).float()
                         for r in range(4)])
        _, cfg = _compressor(W, fs)
        plain = R.compress(z.numpy(), cfg, soft_clip=False, loop=True, direct_level=True)
        _cache[key] = (z, cfg, plain)
    return _cache[key]


def _check_gain_and_product(z, gain, out, st, what):
    g64, prod = st["gain"], st["fir"] * st["gain"]                # (st["fir"] is z itself: the identity filter)
    want32 = g64.astype(np.float32).astype(np.float64)
    gerr = np.abs(gain.double().numpy() - want32) / np.abs(want32)
    perr = np.abs(out.double().numpy() - prod)
    print(f"[ha compressor {what}] worst gain error {gerr.max() / 2.0 ** -23:.3f} x 2^-23, worst product error "
          f"{(perr / np.maximum(np.abs(prod) * 2.0 ** -22, 1e-300)).max():.3f} x bound")
    assert bool((gerr <= 2.0 ** -23).all()), (what, int(gerr.argmax()), float(gerr.max()))
    assert bool((perr <= np.abs(prod) * 2.0 ** -22).all()), (what, int(perr.argmax()))


@pytest.mark.parametrize("W,n,fs", COMP_CASES)
def test_compressor_against_float64(W, n, fs):
    from sehip import _lib
    from sehip.ha import compress_rows
    z, cfg, st = _comp_case(W, n, fs)
    comp, _ = _compressor(W, fs)
    m = R.margin(st["level"], cfg["threshold"])
    above = st["level"] > cfg["threshold"]
    crossings = int((np.diff(above.astype(np.int8), axis=-1) != 0).sum())
    print(f"[ha compressor W={W} n={n}] level margin {m:.3e}, {above.mean():.1%} above the threshold, {crossings} crossings")
    assert m >= R.MIN_MARGIN, "the INPUT is at fault (a level too close to the threshold), not the kernel: change the seed"
    assert crossings >= 2 and 0.05 < above.mean() < 0.95
    dz = z.cuda()
    out, gain = compress_rows(dz, comp, soft_clip=False)
    torch.cuda.synchronize()
    kernel = _kernel()
    tile = _field(kernel, "tile")
    assert kernel.startswith("ha_compressor") and _field(kernel, "W") == W and _field(kernel, "tiles") == -(-n // tile), kernel
    if n == 44320:
        assert _field(kernel, "tiles") > 3 and W > tile, kernel   # the row spans several tiles and the window is longer than one
    if n == 300:
        assert n < W                                              # the row is shorter than the window
    _check_gain_and_product(z, gain.cpu(), out.cpu(), st, f"W={W} n={n}")
    # two runs, CompressorTorch.process, and both settings of the deterministic switch give the same bits
    out2, gain2 = compress_rows(dz, comp, soft_clip=False)
    assert _bits(out, out2) and _bits(gain, gain2)
    assert _bits(comp.process(dz.reshape(2, 2, n)).reshape(4, n), out)
    was = _lib.lib().sehip_get_deterministic()
    try:
        for mode in (1, 0):
            _lib.call("sehip_set_deterministic", mode)
            o, g_ = compress_rows(dz, comp, soft_clip=False)
            assert _bits(o, out) and _bits(g_, gain), mode
    finally:
        _lib.call("sehip_set_deterministic", was)
    # tanh: the unclipped bound plus the allowance for the device's tanh
    clipped, gain_c = compress_rows(dz, comp, soft_clip=True)
    assert _bits(gain_c, gain)
    prod = st["fir"] * st["gain"]
    terr = np.abs(clipped.double().cpu().numpy() - np.tanh(prod))
    only = np.abs(clipped.double().cpu().numpy() - np.tanh(out.double().cpu().numpy()))      # the device's tanh on its own fp32 product
    print(f"[ha tanh W={W} n={n}] device tanh alone: worst |tanhf(y) - tanh64(y)| = {only.max():.3e} = {only.max() / 2.0 ** -24:.3f} x 2^-24")
    print(f"[ha tanh W={W} n={n}] worst |out - tanh64| = {terr.max():.3e} = {terr.max() / 2.0 ** -24:.3f} x 2^-24, "
          f"worst excess over the product bound {np.maximum(terr - np.abs(prod) * 2.0 ** -22, 0).max():.3e}")
    assert bool((terr <= np.abs(prod) * 2.0 ** -22 + T_TANH).all()), (int(terr.argmax()), float(terr.max()))


def test_compressor_rows_that_never_cross():
    from sehip.ha import compress_rows
    g = torch.Generator().manual_seed(5)
    # always below: |z| <= 0.05 keeps every level under sqrt(0.0025 + 1e-8) < 0.35; the gain relaxes towards 1 from 1
    comp, cfg = _compressor(1024, 16000)
    quiet = (0.1 * (torch.rand(1, 5000, generator=g) - 0.5)).float()
    out, gain = compress_rows(quiet.cuda(), comp)
    st = R.compress(quiet.numpy(), cfg)
    assert bool((st["level"] < cfg["threshold"]).all())
    assert float((gain.double().cpu() - 1).abs().max()) <= 2.0 ** -23
    _check_gain_and_product(quiet, gain.cpu(), out.cpu(), st, "always below")
    # always above: W = 1 makes the level |z|, and 0.5 <= |z| keeps it over 0.35 from the first sample on
    comp, cfg = _compressor(1, 16000)
    sign = torch.where(torch.rand(1, 5000, generator=g) < 0.5, -1.0, 1.0)
    loud = (sign * (0.5 + torch.rand(1, 5000, generator=g))).float()
    out, gain = compress_rows(loud.cuda(), comp)
    st = R.compress(loud.numpy(), cfg)
    assert bool((st["level"] > cfg["threshold"]).all()) and R.margin(st["level"], cfg["threshold"]) > 0.4
    _check_gain_and_product(loud, gain.cpu(), out.cpu(), st, "always above")
    assert float(gain[0, -1]) < 0.6                                # and the gain has really come down


# ---- chain ------------------------------------------------------------------------------------------------------------------------
def _chain_objects():
    from sehip.ha import CompressorTorch, NALRTorch
    c = R.CHAIN
    return NALRTorch(c["nfir"], c["fs"]), CompressorTorch(fs=c["fs"], **c["compressor"]), c["audiogram"]


def _golden():
    if "chain" not in _cache:
        with np.load(os.path.join(ROOT, "tests", "golden", "ha_chain.npz")) as z:
            _cache["chain"] = {k: z[k] for k in z.files}
    return _cache["chain"]


def test_amplify_torch_matches_the_reference():
    from sehip.audio import amplify_torch
    fx = _golden()
    assert float(fx["margin"]) >= CHAIN_MARGIN
    amp, comp, audiogram = _chain_objects()
    x = torch.from_numpy(fx["signal"]).cuda().requires_grad_(True)
    out = amplify_torch(x, amp, comp, audiogram, soft_clip=True)
    assert tuple(out.shape) == fx["out"].shape == (2, 1, 2, 4032) and out.dtype == torch.float32 and out.is_cuda
    (out * torch.from_numpy(fx["G"]).cuda()).sum().backward()
    e_out, e_grad = rel_err(out.detach().cpu(), fx["out"]), rel_err(x.grad.cpu(), fx["grad"])
    print(f"[ha chain vs reference] out {e_out:.3e} grad {e_grad:.3e}")
    assert e_out < ACT_TOL and e_grad < ACT_TOL
    plain = amplify_torch(x.detach(), amp, comp, audiogram, soft_clip=False)
    assert rel_err(plain.cpu(), fx["comp"]) < ACT_TOL
    assert _bits(amplify_torch(x.detach(), amp, comp, audiogram, soft_clip=True), out.detach())      # the cached taps: same bits


def test_right_ear_goes_through_the_left_filter():
    """the reference's quirk (src/audio.py:49): both ears use the LEFT ear's taps"""
    from sehip.audio import amplify_torch
    fx = _golden()
    amp, comp, audiogram = _chain_objects()
    x = torch.from_numpy(fx["signal"]).cuda()
    left = amp.build(audiogram["audiogram_levels_l"], audiogram["audiogram_cfs"]).cuda()
    right = amp.build(audiogram["audiogram_levels_r"], audiogram["audiogram_cfs"]).cuda()
    assert not torch.equal(left, right)
    out = amplify_torch(x, amp, comp, audiogram, soft_clip=False)
    for ear in (0, 1):
        assert _bits(comp.process(amp.apply(left, x[:, :, ear].contiguous())), out[:, :, ear].contiguous()), ear
    assert not _bits(comp.process(amp.apply(right, x[:, :, 1].contiguous())), out[:, :, 1].contiguous())


def test_backward_matches_the_float64_gradient():
    """[2, 1, 2, 500] through amplify_torch with a 64-sample level window (so that the level crosses the threshold inside 500
    samples): out, and d<out, G>/d(signal) with the gain held constant, against ha_ref.  Per input sample the gradient is a K-term
    dot product of fp32 values d = G * gain * (1 - out^2): the bound is the dot-product bound on |d| plus the filter applied to the
    error of d itself -- four fp32 roundings of the product, 2 |out| times the error allowed for out (|z c| 2^-22 + T) and the
    gain's answer to the FIR's fp32 error: a level moves by at most the largest FIR error of its row (an RMS of errors), the
    target b by attenuation x attack times that, and the recurrence's sum of attack (1 - attack)^j is at most 1."""
    from sehip.audio import amplify_torch
    from sehip.ha import CompressorTorch, NALRTorch
    c = R.CHAIN
    amp = NALRTorch(c["nfir"], c["fs"])
    comp = CompressorTorch(fs=c["fs"], **dict(c["compressor"], rms_buffer_size=0.004))
    cfg = R.compressor_config(c["fs"], **dict(c["compressor"], rms_buffer_size=0.004))
    assert comp.win_len == cfg["W"] == 64
    g = torch.Generator().manual_seed(21)
    t = torch.arange(500, dtype=torch.float64) / 500
    env = torch.stack([(0.5 + 0.5 * torch.sin(2 * np.pi * (2 + r) * t + r)) ** 2 for r in range(4)]).reshape(2, 1, 2, 500)
    sig = (0.08 * torch.randn(2, 1, 2, 500, generator=g).double() * env).float()
    G = torch.randn(2, 1, 2, 532, generator=g)
    taps32 = amp.build(c["audiogram"]["audiogram_levels_l"], c["audiogram"]["audiogram_cfs"]).reshape(-1).flip(0).double().numpy()
    st = R.chain(sig.numpy().reshape(4, 500), taps32, cfg, soft_clip=True, direct_level=True)
    above = st["level"] > cfg["threshold"]
    assert R.margin(st["level"], cfg["threshold"]) >= CHAIN_MARGIN and 0.05 < above.mean() < 0.95
    want = R.chain_grad(G.numpy().reshape(4, 532), st, taps32, 500)
    x = sig.cuda().requires_grad_(True)
    out = amplify_torch(x, amp, comp, c["audiogram"], soft_clip=True)
    (got,) = torch.autograd.grad(out, x, G.cuda())
    K = 33
    fir_bound = (K + 2) * 2.0 ** -24 * np.stack([R.fir_abs(r, taps32) for r in sig.numpy().reshape(4, 500)])
    gain_shift = cfg["attenuation"] * fir_bound.max(-1, keepdims=True)
    out_bound = fir_bound * st["gain32"] + np.abs(st["fir"]) * gain_shift + np.abs(st["prod"]) * 2.0 ** -22 + T_TANH
    assert bool((np.abs(out.detach().double().cpu().numpy().reshape(4, 532) - st["out"]) <= out_bound).all())
    Gg = np.abs(G.double().numpy().reshape(4, 532)) * st["gain32"]
    d_abs = Gg * (1 - st["out"] ** 2)
    d_err = Gg * (4 * 2.0 ** -24 * (1 - st["out"] ** 2) + 2 * np.abs(st["out"]) * out_bound) \
        + np.abs(G.double().numpy().reshape(4, 532)) * (1 - st["out"] ** 2) * gain_shift
    bound = np.stack([(K + 2) * 2.0 ** -24 * R.fir_adjoint(d_abs[r], np.abs(taps32), 500) + R.fir_adjoint(d_err[r], np.abs(taps32), 500)
                      for r in range(4)])
    err = np.abs(got.double().cpu().numpy().reshape(4, 500) - want)
    print(f"[ha backward] worst error / bound = {(err / bound).max():.4f}, rel {rel_err(got.cpu().reshape(4, 500), want):.3e}")
    assert bool((err <= bound).all())
    assert rel_err(got.cpu().reshape(4, 500), want) < ACT_TOL


def test_forward_and_backward_replay_from_a_graph():
    from sehip.audio import amplify_torch
    fx = _golden()
    amp, comp, audiogram = _chain_objects()
    sig, G = torch.from_numpy(fx["signal"]).cuda(), torch.from_numpy(fx["G"]).cuda()
    # eager, on a leaf of its own (dropped before the capture); it also caches the taps on the device
    x = sig.clone().requires_grad_(True)
    out_e = amplify_torch(x, amp, comp, audiogram)
    (grad_e,) = torch.autograd.grad(out_e, x, G)
    out_e, grad_e = out_e.detach().clone(), grad_e.clone()
    del x
    torch.cuda.synchronize()
    x_s = torch.zeros_like(sig).requires_grad_(True)               # first used inside the capture
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_s = amplify_torch(x_s, amp, comp, audiogram)
        (grad_s,) = torch.autograd.grad(out_s, x_s, G)
    for _ in range(2):
        with torch.no_grad():
            x_s.copy_(sig)
        graph.replay()
        torch.cuda.synchronize()
        assert _bits(out_s.detach(), out_e) and _bits(grad_s, grad_e)
        with torch.no_grad():
            out_s.zero_()
            grad_s.zero_()
