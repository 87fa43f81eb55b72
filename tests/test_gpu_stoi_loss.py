"""GPU: sehip.loss.stoi_loss / stoi_loss_rows / StoiLoss (csrc/stoi_loss.hip) against tests/stoi_loss_ref.py, the float64 torch
restatement of tests/stoi_ref.py with autograd.

The whole gradient is gated per row by ||g - g64|| / ||g64|| <= G with G COMPUTED here: 8 x the largest such deviation of the oracle's own
float32 restatement over this file's cases (one restatement is one sample of fp32 rounding; 8 is the factor of the metric's gate).  Every
backward launch is also run on the device's own operands against float64 on those operands: the two non-linear ones (segments, bands)
under a gate built the same way from the float32 restatement of that step, the two adjoints (compaction, resampler) as linear maps under
the fp32 dot-product bound (terms + 2) 2^-24 sum |w| |g| of the forward resampler's test.  Measured on an MI355X: DESIGN.md section 20.
Signals: stoi_ref.am_signal as clean, estimate = clean + RandomState(100 + seed).randn scaled to 20, 0 and -5 dB."""
import numpy as np
import pytest
import torch

import stoi_loss_ref as LR
import stoi_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 12345.0
# (sr, n): 6000 and 8000 samples at 10 kHz (45 and 61 frames: more than one block of 16 / 8 segments) and the same durations elsewhere
GRAD_CASES = ((10000, 6000), (10000, 8000), (16000, 9600), (16000, 12800), (48000, 28800), (48000, 38400), (44100, 26460), (44100, 35280),
              (8000, 4800), (8000, 6400))
SNRS = (0.0, -5.0, 20.0)                                  # of a case's three rows
# The seeds of a case's three clean rows.  Which cells the plain variant clips is a property of the CLEAN signal (a cell 15 dB below its
# segment's level in a band), hardly of the noise: in float64 the count is the same at 0, -5 and -10 dB.  So the seeds are chosen per rate,
# on the oracle alone, such that EVERY row has at least 10 clipped cells and no cell within 1e-3 of the branch point at both durations
# (10 kHz keeps seed 1 at 0 dB and seed 2 at -5 dB; seeds 1 .. 3 at 16 k / 48 k / 44.1 k clip nothing, seed 2 at 8 kHz sits 6.9e-4 from
# the branch point).  test_cases_are_what_they_claim asserts it.
SEEDS = {10000: (1, 2, 14), 16000: (7, 10, 12), 48000: (4, 24, 31), 44100: (16, 24, 41), 8000: (5, 11, 24)}
EDGE_CASES = ((10000, 4095), (10000, 4223), (10000, 4351))  # 29 / 30 / 31 spectra: no segment, one, two
MIXED_CASES = ((10000, 6000), (16000, 9600))              # rows: a gap, too short, an all-zero estimate, a plain one
_cache = {}


def noisy(x, seed, snr):
    r = np.random.RandomState(100 + seed).randn(len(x))
    return x + r * np.sqrt(np.mean(x * x) / (np.mean(r * r) * 10 ** (snr / 10)))


def rows_of(sr, n, kind):
    if kind == "grad":
        xs = [R.am_signal(n, sr, seed) for seed in SEEDS[sr]]
        ys = [noisy(x, seed, snr) for x, seed, snr in zip(xs, SEEDS[sr], SNRS)]
    elif kind == "edge":
        xs = [R.am_signal(n, sr, 4)]
        ys = [noisy(xs[0], 4, 0.0)]
    else:                                                 # (the silenced-gap case is the first row here, not a case of its own)
        gap, short = R.am_signal(n, sr, 5), R.am_signal(n, sr, 6)
        gap[int(0.4 * n):int(0.6 * n)] *= 1e-4            # 80 dB down: far below the 40 dB range
        short[int(0.2 * sr):] *= 1e-4                     # 0.2 s: 2000 samples at 10 kHz, fewer than 30 frames are left
        xs = [gap, short, R.am_signal(n, sr, 7), R.am_signal(n, sr, 8)]
        ys = [noisy(xs[0], 5, 0.0), noisy(xs[1], 6, 0.0), np.zeros(n), noisy(xs[3], 8, -5.0)]
    # the device's inputs ARE float32: the oracle gets the same samples
    return np.stack(xs).astype(np.float32), np.stack(ys).astype(np.float32)


def case(sr, n, kind="grad"):
    """inputs and the oracle's (loss, gradient, per-row values) in float64 and float32 for both variants; computed once and shared"""
    key = (sr, n, kind)
    if key not in _cache:
        xs, ys = rows_of(sr, n, kind)
        ref = {(ext, dt): LR.loss_and_grad(xs, ys, sr, ext, dt) for ext in (False, True) for dt in (torch.float64, torch.float32)}
        _cache[key] = (xs, ys, ref)
    return _cache[key]


def all_cases():
    return [(sr, n, "grad") for sr, n in GRAD_CASES] + [(sr, n, "edge") for sr, n in EDGE_CASES] + [(sr, n, "mixed") for sr, n in MIXED_CASES]


def rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def gate():
    """G = 8 x the largest per-row deviation of the float32 restatement's gradient from float64's over every case of the file"""
    if "gate" not in _cache:
        worst = 0.0
        for sr, n, kind in all_cases():
            _, _, ref = case(sr, n, kind)
            for ext in (False, True):
                g64, g32 = ref[(ext, torch.float64)][1], ref[(ext, torch.float32)][1]
                for a, b in zip(g32, g64):
                    if np.any(b != 0):
                        worst = max(worst, rel(a, b))
        _cache["gate"] = (8 * worst, worst)
    return _cache["gate"]


def on_device(a, shape=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if shape is None else t.reshape(shape)


def device_loss_and_grad(xs, ys, sr, ext, per_row=False, weights=None):
    from sehip.loss import stoi_loss, stoi_loss_rows
    x, y = on_device(xs), on_device(ys).requires_grad_(True)
    if per_row:
        val = stoi_loss_rows(y, x, sr=sr, extended=ext)
        val.backward(weights)
    else:
        val = stoi_loss(y, x, sr=sr, extended=ext)
        val.backward()
    return val.detach(), y.grad


def guarded(numel, dtype=torch.float32):
    return torch.full((numel + 2 * GUARD,), FILL if dtype == torch.float32 else 12345, device="cuda", dtype=dtype)


def guards_intact(buf):
    fill = FILL if buf.dtype == torch.float32 else 12345
    return bool((buf[:GUARD] == fill).all()) and bool((buf[-GUARD:] == fill).all())


def forward_state(xs, ys, sr, ext=False):
    """one forward pass of the functional form -> its workspace (kept, src, tob and, off 10 kHz, the resampled pair stay on the device)"""
    from sehip.loss import stoi_loss, stoi_loss_workspace
    x, y = on_device(xs), on_device(ys)
    stoi_loss(y, x, sr=sr, extended=ext)
    ws = stoi_loss_workspace(x.shape, sr, ext, x.device)
    est10 = y if ws.sig is None else ws.sig[ws.rows:]
    return ws, est10


# ---- the cases and the gate, on the oracle alone ---------------------------------------------------------------------------------------
def test_cases_are_what_they_claim():
    """frame counts, row kinds, and the clip-branch condition of the plain variant in float64: every row of every gradient case has at
    least 10 clipped cells and no cell closer than 1e-3 (relative) to the branch point"""
    for sr, n in GRAD_CASES:
        xs, ys, ref = case(sr, n)
        assert R.frame_count(R.out_len(n, sr) if sr != 10000 else n) in (45, 61)
        for x, y, seed, snr in zip(xs, ys, SEEDS[sr], SNRS):
            st = LR.stoi_steps(x, torch.from_numpy(y.astype(np.float64)), sr)
            assert st["T"] >= 31
            _, mask, dist = LR.correlate(st["x_tob"], st["y_tob"], detail=True)
            clipped, margin = int(mask.sum()), float(dist.min())
            print(f"[stoi_loss] sr {sr} n {n} seed {seed} at {snr:g} dB: {clipped} clipped cells, nearest {margin:.2e} from the branch point")
            assert clipped >= 10 and margin >= 1e-3, (sr, n, seed, clipped, margin)
    for (sr, n), t in zip(EDGE_CASES, (29, 30, 31)):
        xs, ys, ref = case(sr, n, "edge")
        assert LR.stoi_steps(xs[0], torch.from_numpy(ys[0].astype(np.float64)), sr)["T"] == t
        assert (ref[(False, torch.float64)][2][0] == 1e-5) == (t < 30)
    for sr, n in MIXED_CASES:
        xs, ys, ref = case(sr, n, "mixed")
        vals, grads = ref[(False, torch.float64)][2], ref[(False, torch.float64)][1]
        n10 = n if sr == 10000 else R.out_len(n, sr)
        assert 30 < len(LR.kept_frames(xs[0], sr)) < R.frame_count(n10)
        assert vals[1] == 1e-5 and not grads[1].any() and not grads[2].any() and np.isfinite(grads).all()
    g, worst = gate()
    print(f"[stoi_loss] float32 restatement: worst per-row gradient deviation {worst:.3e}, gate {g:.3e}")
    assert 0 < g <= 1e-4, g                                          # else the comparison is ill-posed


# ---- value and whole gradient ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extended", [False, True])
@pytest.mark.parametrize("sr,n,kind", all_cases())
def test_value_and_gradient(sr, n, kind, extended):
    from sehip.metric import STOI, stoi_rows
    g_gate, _ = gate()
    xs, ys, ref = case(sr, n, kind)
    loss64, g64, d64 = ref[(extended, torch.float64)]
    x, y = on_device(xs), on_device(ys)
    val, grad = device_loss_and_grad(xs, ys, sr, extended)
    assert val.dim() == 0 and val.dtype == torch.float32 and grad.shape == y.shape and grad.dtype == torch.float32
    assert torch.equal(val, -STOI(x, y, sr=sr, extended=extended))                   # bit for bit
    w = torch.linspace(0.5, 1.5, len(xs), device="cuda")
    vrows, grows = device_loss_and_grad(xs, ys, sr, extended, per_row=True, weights=w)
    assert torch.equal(vrows, -stoi_rows(x, y, sr=sr, extended=extended))
    assert abs(float(val) - loss64) <= 1e-5
    grad, grows = grad.cpu().double().numpy(), grows.cpu().double().numpy()
    assert np.isfinite(grad).all() and np.isfinite(grows).all()
    worst = 0.0
    for i in range(len(xs)):
        if not g64[i].any():
            assert not grad[i].any() and not grows[i].any(), i      # exact zeros: a row without a segment, an all-zero estimate
            continue
        worst = max(worst, rel(grad[i], g64[i]), rel(grows[i], g64[i] * len(xs) * float(w[i])))
    print(f"[stoi_loss] sr {sr} n {n} {kind} extended {extended}: worst per-row gradient deviation {worst:.3e} (gate {g_gate:.3e})")
    assert worst <= g_gate, (worst, g_gate)


def test_exact_zeros_and_run_to_run_bits():
    """10 kHz, the mixed rows: samples that lie only in dropped frames, the tail past the last frame, the too-short row and the all-zero
    estimate get exact zeros; two runs give the same bits; a STOI() call between forward and backward changes nothing"""
    from sehip.loss import StoiLoss
    from sehip.metric import STOI
    sr, n = MIXED_CASES[0]
    xs, ys, _ = case(sr, n, "mixed")
    runs = [device_loss_and_grad(xs, ys, sr, False) for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    grad = runs[0][1].cpu().numpy()
    frames = R.frame_count(n)
    for i in (0, 3):
        covered = np.zeros(n, dtype=bool)
        for f in LR.kept_frames(xs[i], sr):
            covered[f * R.HOP:f * R.HOP + R.N_FRAME] = True
        tail = n - ((frames - 1) * R.HOP + R.N_FRAME)
        assert tail > 0 and not covered[n - tail:].any()
        assert (~covered).sum() > tail + 256 if i == 0 else (~covered).sum() == tail     # the gap row has dropped-frame-only samples
        assert not grad[i][~covered].any(), i
        assert np.count_nonzero(grad[i][covered]) > 0.95 * covered.sum()                 # (the last compacted hop is read by no spectrum)
    assert not grad[1].any() and not grad[2].any()
    # a module owns its buffers: validation by the metric at the same shape in between, and a functional call, disturb nothing
    mod = StoiLoss(sr=sr)
    x, y = on_device(xs), on_device(ys).requires_grad_(True)
    loss = mod(y, x)
    STOI(x.flip(0), y.detach().flip(0) * 0.5, sr=sr)
    device_loss_and_grad(xs[::-1].copy(), ys[::-1].copy(), sr, False)
    loss.backward()
    assert torch.equal(loss.detach(), runs[0][0]) and torch.equal(y.grad, runs[0][1])


# ---- op-local gates ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extended", [False, True])
@pytest.mark.parametrize("sr,n,kind", [(10000, 8000, "grad"), (16000, 9600, "grad"), (16000, 9600, "mixed")])
def test_segments_backward_on_the_devices_bands(sr, n, kind, extended):
    from sehip._lib import call, lib, ptr, stream
    xs, ys, _ = case(sr, n, kind)
    ws, _ = forward_state(xs, ys, sr, extended)
    rows, frames = ws.rows, ws.frames
    tob, kept = ws.tob.cpu().double(), ws.kept.cpu().numpy()
    gout = torch.linspace(0.5, 1.5, rows, device="cuda")
    seg = guarded(lib().sehip_stoil_segment_floats(rows, frames))
    dtob = guarded(rows * 15 * (frames - 1))
    call("sehip_stoil_segments", ptr(ws.tob), ptr(ws.kept), rows, frames, int(extended), ptr(gout), 1, 0.25, ptr(seg[GUARD:]),
         ptr(dtob[GUARD:]), stream())
    assert guards_intact(seg) and guards_intact(dtob)
    got = dtob[GUARD:-GUARD].reshape(rows, 15, frames - 1).cpu().double().numpy()
    worst = gated = 0.0
    for i in range(rows):
        t = kept[i] - 1
        assert not got[i][:, max(t, 0):].any()
        if t < 30:
            assert not got[i].any()
            continue
        want = {}
        for dt in (torch.float64, torch.float32) if tob[1, i].any() else ():
            yt = tob[1, i, :, :t].to(dt).requires_grad_(True)
            d = LR.correlate(tob[0, i, :, :t].to(dt), yt, extended)
            want[dt] = torch.autograd.grad(-float(gout[i]) * 0.25 * d, yt)[0].double().numpy()
        if not tob[1, i].any():                                  # an all-zero estimate: finite, and weighted by 0 in the next step
            assert np.isfinite(got[i]).all()
            continue
        gated = max(gated, 8 * rel(want[torch.float32], want[torch.float64]))
        worst = max(worst, rel(got[i][:, :t], want[torch.float64]))
    print(f"[stoi_loss] segments backward sr {sr} extended {extended}: {worst:.3e} (gate {gated:.3e})")
    assert 0 < gated <= 1e-4 and worst <= gated


def band_step(frames_t, dt):
    """[15][T] band magnitudes of [T][256] frames of the compacted signal (windowed, zero-padded to 512)"""
    return LR.band_magnitudes(torch.fft.rfft(LR.window(dt) * frames_t, n=R.NFFT, dim=1))


@pytest.mark.parametrize("sr,n,kind", [(10000, 6000, "grad"), (16000, 9600, "mixed")])
def test_bands_backward_on_the_devices_operands(sr, n, kind):
    from sehip._lib import call, ptr, stream
    xs, ys, _ = case(sr, n, kind)
    ws, est10 = forward_state(xs, ys, sr)
    rows, frames, n10 = ws.rows, ws.frames, ws.n10
    kept, src = ws.kept.cpu().numpy(), ws.src.cpu().numpy()
    dtob_h = np.random.RandomState(5).randn(rows, 15, frames - 1).astype(np.float32)
    fgrad = guarded(rows * (frames - 1) * 256)
    call("sehip_stoil_bands", ptr(est10.contiguous()), rows, n10, ptr(ws.kept), ptr(ws.src), ptr(ws.tob), ptr(on_device(dtob_h)),
         ptr(fgrad[GUARD:]), stream())
    assert guards_intact(fgrad)
    got = fgrad[GUARD:-GUARD].reshape(rows, frames - 1, 256).cpu().double().numpy()
    y10 = est10.cpu().double()
    worst = gated = 0.0
    for i in range(rows):
        t = kept[i] - 1
        if t < 30:
            assert bool((got[i] == FILL).all())                  # a row without a segment: nothing is written, nothing is read later
            continue
        assert bool((got[i][t:] == FILL).all())
        want = {}
        for dt in (torch.float64, torch.float32):
            yc = LR.compact(y10[i].to(dt), src[i, :kept[i]], dt)
            fr = yc.unfold(0, R.N_FRAME, R.HOP)[:t].clone().requires_grad_(True)
            want[dt] = torch.autograd.grad((torch.from_numpy(dtob_h[i, :, :t]).to(dt) * band_step(fr, dt)).sum(), fr)[0].double().numpy()
        if not y10[i].any():
            assert not got[i][:t].any() and not want[torch.float64].any()
            continue
        gated = max(gated, 8 * rel(want[torch.float32], want[torch.float64]))
        worst = max(worst, rel(got[i][:t], want[torch.float64]))
    print(f"[stoi_loss] bands backward sr {sr}: {worst:.3e} (gate {gated:.3e})")
    assert 0 < gated <= 1e-4 and worst <= gated


def compact_adjoint_host(fg, src, n10, absolute=False):
    """scatter form, float64: overlap-add the frame gradients at hop 128, then window and scatter the kept frames back"""
    win = R.window()
    k = len(src)
    t = k - 1
    fg = np.abs(fg) if absolute else fg
    gyc = np.zeros((k + 1) * R.HOP)
    for j in range(t):
        gyc[j * R.HOP:j * R.HOP + R.N_FRAME] += fg[j]
    out = np.zeros(n10)
    for j, f in enumerate(src):
        out[f * R.HOP:f * R.HOP + R.N_FRAME] += win * gyc[j * R.HOP:j * R.HOP + R.N_FRAME]
    return out


def test_compaction_adjoint_is_the_linear_map():
    """every sample within (4 + 2) 2^-24 sum |w| |g| (at most 4 products per sample) of float64, exact zeros outside the kept frames, the
    inverse table exact, and <C y, g> = <y, C^T g> against the ORACLE's compaction: the forward fuses the compaction into the non-linear
    bands kernel, so there is no linear forward launch to pair this adjoint with (the resampler's identity below runs against its kernel)"""
    from sehip._lib import call, ptr, stream
    sr, n = MIXED_CASES[0]
    xs, ys, _ = case(sr, n, "mixed")
    ws, _ = forward_state(xs, ys, sr)
    rows, frames, n10 = ws.rows, ws.frames, ws.n10
    kept, src = ws.kept.cpu().numpy(), ws.src.cpu().numpy()
    fg_h = np.random.RandomState(6).randn(rows, frames - 1, 256).astype(np.float32)
    inv, out = guarded(rows * frames, torch.int32), guarded(rows * n10)
    call("sehip_stoil_compact", ptr(on_device(fg_h)), ptr(ws.kept), ptr(ws.src), rows, n10, ptr(inv[GUARD:]), ptr(out[GUARD:]), stream())
    assert guards_intact(inv) and guards_intact(out)
    inv_h = inv[GUARD:-GUARD].reshape(rows, frames).cpu().numpy()
    got = out[GUARD:-GUARD].reshape(rows, n10).cpu().double().numpy()
    worst = 0.0
    for i in range(rows):
        want_inv = -np.ones(frames, dtype=np.int64)
        want_inv[src[i, :kept[i]]] = np.arange(kept[i])
        assert np.array_equal(inv_h[i], want_inv)
        if kept[i] < 31:
            assert not got[i].any()
            continue
        s = src[i, :kept[i]]
        want = compact_adjoint_host(fg_h[i].astype(np.float64), s, n10)
        bound = 6 * 2.0 ** -24 * compact_adjoint_host(fg_h[i].astype(np.float64), s, n10, absolute=True)
        err = np.abs(got[i] - want)
        assert bool((err <= bound).all()), (i, int(err.argmax()), float(err.max()))
        assert not got[i][bound == 0].any()
        worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
        # the adjoint identity against the oracle's forward compaction: frames t < T of compact(y)
        y = ys[i].astype(np.float64)
        cy = R.compact(y, s)
        lhs = sum(float(np.dot(cy[t * R.HOP:t * R.HOP + R.N_FRAME], fg_h[i, t].astype(np.float64))) for t in range(kept[i] - 1))
        rhs = float(np.dot(y, got[i]))
        assert abs(lhs - rhs) <= float(np.dot(np.abs(y), bound)), (lhs, rhs)
    print(f"[stoi_loss] compaction adjoint: worst error / bound {worst:.3e}")


@pytest.mark.parametrize("sr,n", [(16000, 1003), (48000, 2001), (44100, 1777), (8000, 999)])
def test_resampler_adjoint_is_the_linear_map(sr, n):
    """every sample within (terms + 2) 2^-24 sum |w| |g| of float64 (terms = ceil((2 L + 1) / q) outputs reach one input), and the
    adjoint identity <A x, g> = <x, A^T g> against the forward kernel, both sides accumulated in float64 on the host"""
    from sehip import metric
    from sehip._lib import call, ptr, stream
    table, p, q, L = metric.stoi_resample_table(sr, "cuda")
    m = metric.stoi_out_len(n, sr)
    _, _, _, tab = R.phase_table(sr)
    tab = tab.astype(np.float32).astype(np.float64)                 # the table the device reads
    kt = tab.shape[1]
    rng = np.random.RandomState(sr)
    g_h = rng.randn(2, m).astype(np.float32)
    x_h = np.stack([R.am_signal(n, sr, seed=sr + i) for i in range(2)]).astype(np.float32)
    outs = []
    for _ in range(2):
        out = guarded(2 * n)
        call("sehip_stoil_resample_adj", ptr(on_device(g_h)), 2, n, ptr(table), p, q, L, ptr(out[GUARD:]), stream())
        assert guards_intact(out)
        outs.append(out[GUARD:-GUARD].reshape(2, n).cpu())
    assert torch.equal(outs[0], outs[1])
    got = outs[0].double().numpy()
    fwd = torch.empty(4, m, device="cuda")
    xd = on_device(x_h)
    call("sehip_stoi_resample", ptr(xd), ptr(xd), 2, n, ptr(table), p, q, L, ptr(fwd), stream())
    fwd = fwd[:2].cpu().double().numpy()
    base = np.arange(m, dtype=np.int64) * q + L
    idx = (base // p)[:, None] - np.arange(kt)[None, :]
    ok = (idx >= 0) & (idx < n)
    terms = -(-(2 * L + 1) // q)
    worst = 0.0
    for i in range(2):
        want, mag = np.zeros(n), np.zeros(n)
        np.add.at(want, idx[ok], (tab[base % p] * g_h[i].astype(np.float64)[:, None])[ok])
        np.add.at(mag, idx[ok], np.abs(tab[base % p] * g_h[i].astype(np.float64)[:, None])[ok])
        bound = (terms + 2) * 2.0 ** -24 * mag
        err = np.abs(got[i] - want)
        assert bool((err <= bound).all()), (sr, i, int(err.argmax()), float(err.max()))
        worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
        fmag = (np.abs(tab[base % p]) * np.where(ok, np.abs(x_h[i].astype(np.float64))[np.clip(idx, 0, n - 1)], 0.0)).sum(axis=1)
        tol = float(np.dot(np.abs(g_h[i]), (kt + 2) * 2.0 ** -24 * fmag) + np.dot(np.abs(x_h[i]), bound))
        lhs, rhs = float(np.dot(fwd[i], g_h[i].astype(np.float64))), float(np.dot(x_h[i].astype(np.float64), got[i]))
        assert abs(lhs - rhs) <= tol, (lhs, rhs, tol)
    print(f"[stoi_loss] resampler adjoint {sr}: worst error / bound {worst:.3e} ({terms} terms per input)")


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_loss():
    from sehip import SehipError, stoi_loss
    x = torch.zeros(1, 1, 8000, device="cuda")
    with pytest.raises(SehipError, match="stoi_loss"):
        stoi_loss(x[..., :408], x[..., :408], sr=16000)            # 255 samples at 10 kHz
    with pytest.raises(SehipError, match="stoi_loss"):
        stoi_loss(x, x, sr=16001)
    with pytest.raises(ValueError, match="stoi_loss"):
        stoi_loss(x, x[..., :4000])
    with pytest.raises(SehipError, match="stoi_loss"):
        stoi_loss(x.cpu(), x)
    y = x.clone().requires_grad_(True)
    loss = stoi_loss(y, x.requires_grad_(True))                    # an all-zero pair: finite, and nothing flows to the clean signal
    loss.backward()
    assert x.grad is None and not y.grad.any() and float(loss.detach()) == 0.0


# ---- graph -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extended", [False, True])
def test_captured_forward_and_backward_equal_eager_bits(extended):
    from sehip.loss import StoiLoss
    sr, n = 16000, 9600
    xa, ya, _ = case(sr, n, "mixed")
    xb, yb, _ = case(sr, n, "grad")
    xb, yb = np.concatenate([xb, xb[:1]]), np.concatenate([yb, yb[:1]])     # four rows as well
    eager = [device_loss_and_grad(x, y, sr, extended) for x, y in ((xa, ya), (xb, yb))]
    mod = StoiLoss(sr=sr, extended=extended)
    # eager warm-up on tensors of its own: a leaf that an eager forward has used stays bound to that forward's stream
    warm = on_device(ya).requires_grad_(True)
    torch.autograd.grad(mod(warm, on_device(xa)), warm)
    del warm
    torch.cuda.synchronize()
    x_s, y_s = on_device(xa), on_device(ya).requires_grad_(True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss_s = mod(y_s, x_s)
        (grad_s,) = torch.autograd.grad(loss_s, y_s)
    for (x, y), (loss, grad) in (((xb, yb), eager[1]), ((xa, ya), eager[0])):
        with torch.no_grad():
            x_s.copy_(on_device(x))
            y_s.copy_(on_device(y))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(loss_s, loss) and torch.equal(grad_s, grad)


# ---- Solver --------------------------------------------------------------------------------------------------------------------------------
def solver_config(tmp, loss):
    from sehip.utils import dict2obj
    return dict2obj({
        "seed": 10, "root": None, "ha": None,
        "model": {"name": "conv-tasnet", "audio_channels": 1, "num_spk": 2, "sources": ["None", "None"], "skip": False, "sample_rate": 8000,
                  "segment": 1, "causal": True, "norm_type": "cLN", "N": 32, "L": 8, "B": 32, "H": 96, "P": 3, "X": 3, "R": 2},
        "optim": {"optim": "adam", "lr": 3e-4, "beta1": 0.9, "beta2": 0.999, "loss": loss, "clip_grad": 5, "pit": False, "load": False},
        "dset": {"name": "synthetic", "sample_rate": 8000},
        "solver": {"epochs": 1, "save_checkpoint_interval": 1000, "all_steps": True, "total_steps": 0, "patience": 0,
                   "root": str(tmp), "resume": None, "preloaded_model": None,
                   "validation": {"interval": 1000, "metric": "loss", "total_steps": 0}, "test": {"interval": 1000}},
    })


def test_solver_trains_on_stoi_eager_and_graphed(tmp_path):
    """one train_step and one train_step_graphed of a small causal ConvTasNet with optim.loss 'stoi', from the same initial state: the
    loss is -STOI of that batch at the data set's sample rate, every gradient is finite, the graphed step gives the eager loss bits and
    the eager gradients as closely as a second eager step does (the model's backward sums with atomics; see the end)"""
    import copy
    from sehip import STOI, distrib
    from sehip.loss import StoiLoss
    from sehip.solver import ScalarLog, Solver
    cfg = solver_config(tmp_path, "stoi")
    torch.manual_seed(0)
    state = copy.deepcopy(distrib.get_model(cfg.model).state_dict())
    src = np.stack([[R.am_signal(8000, 8000, seed=50 + 2 * b + s)] for b in range(2) for s in range(2)]).reshape(2, 2, 1, 8000)
    src = torch.from_numpy(src.astype(np.float32))
    mix = src.sum(1)
    out = []
    for graphed in (False, False, True):
        model = distrib.get_model(cfg.model)
        model.load_state_dict(state)
        loss_fn = distrib.get_loss_function(cfg.optim)
        assert isinstance(loss_fn, StoiLoss) and not loss_fn.extended
        solver = Solver(copy.deepcopy(cfg), model, distrib.get_optimizer(cfg.optim, model), loss_fn, device="gpu", writer=ScalarLog())
        assert loss_fn.sr == 8000
        seen = {}
        loss_fn.register_forward_hook(lambda m, inp, res: seen.update(enhanced=inp[0].detach().clone(), sources=inp[1].detach().clone()))
        mx, sr = solver._prepare_batch(mix, src)
        loss, _ = (solver.train_step_graphed if graphed else solver.train_step)(mx, sr)
        torch.cuda.synchronize()
        grads = solver.model.flat_grads
        assert bool(torch.isfinite(grads).all()) and bool(grads.any())
        if not graphed:                                             # (the hook of the graphed step saw the capture's placeholders)
            assert seen["enhanced"].shape == seen["sources"].shape and seen["enhanced"].numel() == 4 * 8000
            assert torch.equal(loss, -STOI(seen["sources"], seen["enhanced"], sr=8000))
            assert -1 < float(loss) < 0
        out.append((loss.clone(), grads.clone()))
    (l0, g0), (l1, g1), (lg, gg) = out
    top = float(g0.abs().max())
    again, graph = float((g0 - g1).abs().max()), float((g0 - gg).abs().max())
    print(f"[stoi_loss] solver: eager {float(l0):.9g} graphed {float(lg):.9g}; largest gradient {top:.3e}, a second eager step differs "
          f"by {again:.3e}, the graphed one by {graph:.3e}")
    # The loss (forward only) has the eager bits, and the loss's own gradient is bit-reproducible (the graph test above).  The model's
    # weight gradients are not, eager against eager either: without solver.cudnn_deterministic (which use_graph excludes) its backward
    # sums with fp32 atomics, whose arrival order moves last bits.  One ulp of the largest element is 2^-24 = 6e-8 of it; 16 of them:
    assert torch.equal(l0, l1) and torch.equal(l0, lg)
    assert again <= 1e-6 * top and graph <= 1e-6 * top, (again, graph, top)
