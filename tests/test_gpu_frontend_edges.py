"""GPU: the kernels every training step passes through, whatever the model -- csrc/stft.hip + csrc/mask.h (STFT, mask, iSTFT, clamp and
their backward) and csrc/loss.hip (SI-SNR, permutation-invariant SI-SNR, the SI-SDR metric, l1 / mse, psa) -- against the float64
restatements of tests/frontend_ref.py, at the edges tests/test_gpu_frontend.py, test_pit.py, test_psa_loss.py and test_gpu_evaluate.py
do not reach: an active clamp, window lengths that are no multiple of 8 (the scalar store path of istft_frames_kernel and the lane that
straddles `win`), digital silence, second trips of every row / stride loop, misaligned rows, S = 1 / 4 / 6 speakers and an exact tie,
the grid caps of l1 / mse / psa, SI-SNR at 20 - 60 dB.  Every output buffer sits between sentinel bands (Banded of
tests/test_gpu_wavunet.py), is pre-filled with NaN, and must come back finite with the bands intact.

Gates (constants of tests/test_gpu_wavunet.py):
  fp32 sums (spectrum bins, waveform samples)  |got - f64| <= SUM_TOL * sum |addends|, per element.  The waveform is compared after the
      clamp on both sides: the clamp is 1-Lipschitz, so this asks no more than the gate before the clamp and no less wherever it is idle.
  bf16 outputs (enc, dmask)  check_small: rms within OUT_TOL (times the ratio documented there), every element within ULP_TOL, against
      float64 from the kernel's own fp32 operands.
  fp32 gradients, loss values  norm-relative error <= max(4 x the fp32 CPU oracle's deviation from float64 on the same inputs, 1e-6).
  values in dB  max(4 x the fp32 oracle's deviation, 4.343 * 2 * SUM_TOL = 1.74e-4 dB).
tests/test_frontend_ref_host.py checks the restatements, asserts the conditions on these inputs and shows that every gate rejects a
reference perturbed the way a fault would perturb the kernel.

Measured on an MI355X (every test prints what it gates):
  fp32 sums   spectrum bins worst 2.5e-7 of the absolute addends at two and more samples per frame, 4.7e-6 at [1, 1] (one addend per bin:
              the rounding of a twiddle product against an addend with cos near 0); waveform samples worst 5.0e-8 (gate 2e-5);
              digital silence (13 and 11 all-zero frames of 43): spectrum 6.8e-8, waveform at most 3.7e-8
  bf16        enc and dmask over 36 + 333 tensors: rms at most 0.917 of its bound (every rms equals that of the float64 result rounded
              once, to four digits), worst element 0.9955 of half a bf16 ulp (gate 1.02); clamp active on 35.1 / 32.3 / 32.5 % of the
              samples in modes 0 / 1 / 2, upstream zeroed on 0.0125 %, waveform 2.0e-8 of the absolute addends there
  SI-SNR      gradient 1.0 - 1.5 x the fp32 oracle's deviation at every shape (1.2e-7 .. 1.7e-7, bound 1e-6), 2.2e-7 at [1, 1] (7 x the
              oracle's 3.2e-8, under the 1e-6 floor); per row at 0 / 20 / 40 / 60 dB 1.3e-7 / 2.6e-7 / 2.5e-6 / 2.6e-5, which is 1.53 /
              0.98 / 1.00 / 1.00 x the oracle (bound 4 x); rows at most 3.7e-6 dB off (bound 1.74e-4); zero rows: gradient exactly 0
  PIT         permutation identical at S = 1, 2, 4, 6 and 70 rows per pair (gaps 9.8 - 39.8 dB), identity on the tie; pair matrix at most
              1.2e-5 dB, loss 1.6e-6 dB off (bound 1.74e-4); gradient 0.9 - 1.2 x the oracle (1.0e-7 .. 1.3e-7, bound 1e-6)
  SI-SDR      (70, 64) / (3, 16000) / (1, 8) / silent rows among others / all silent: 2.7e-7 / 4.0e-7 / 1.8e-7 / 5.9e-7 / 1.3e-6 dB off
              float64, where the fp32 numpy restatement is 2.7e-7 / 5.5e-7 / 7.7e-7 / 1.1e-7 / 1.3e-6 dB off (bound 1.74e-4 dB in all five)
  l1 / mse    loss at most 6.5e-8, gradient at most 4.6e-8 (bound 1e-6), 4 198 403 elements included; l1 gradient exactly 0 on equal elements
  psa         loss at most 7.1e-8, gradient at most 8.2e-8 (bound 1e-6), 2 099 201 complex elements included
"""
import pytest
import torch

import frontend_ref as R
from test_gpu_frontend import GEOMETRIES
from test_gpu_wavunet import SUM_TOL, Banded, check_small, check_sum

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
CONFIGS = [(w, h, "hann") for w, h in GEOMETRIES + [(398, 100), (396, 99), (64, 16)]] + [(400, 100, "hamming"), (400, 100, None)]
BN = [(1, 1), (3, 257), (5, 1999), (2, 4000)]


@pytest.fixture(scope="module", autouse=True)
def device():
    from sehip import _lib
    assert torch.cuda.is_available()
    _lib.call("sehip_check_device", 0)


def call(name, *args):
    from sehip import _lib
    _lib.call(name, *args, torch.cuda.current_stream().cuda_stream)


class Bands:
    """the output buffers of one test: Banded, pre-filled so that an element the kernel leaves out shows"""

    def __init__(self):
        self.all = {}

    def new(self, name, n, dtype=F32):
        b = Banded(n, dtype)
        b.view.fill_(float("nan") if dtype.is_floating_point else -7)
        self.all[f"{name} #{len(self.all)}"] = b
        return b

    def settle(self):
        torch.cuda.synchronize()
        for name, b in self.all.items():
            assert b.intact(), name
            assert bool(torch.isfinite(b.view.double()).all()) and bool((b.view != -7).all() or b.view.dtype.is_floating_point), name
        self.all = {}


def dev(t):
    return t.contiguous().cuda()


def hip_stft(bands, wav, window, win, hop):
    b, n = wav.shape
    t = R.frames_of(n, win, hop)
    spec, enc = bands.new("spec", b * t * 257 * 2), bands.new("enc", b * t * 256 * 2, BF16)
    call("sehip_stft_fwd", wav.data_ptr(), window.data_ptr(), b, n, win, hop, 512, spec.ptr, enc.ptr)
    return spec.view.view(b, t, 257, 2), enc.view.view(b, t, 256, 2)


def hip_istft(bands, spec, mask, window, inv, win, hop, length, mode):
    b, t = spec.shape[:2]
    frames, wav = bands.new("frames", b * t * win), bands.new("wav", b * length)
    call("sehip_istft_fwd", spec.data_ptr(), mask.data_ptr(), window.data_ptr(), inv.data_ptr(), b, t, win, hop, 512, length, mode,
         frames.ptr, wav.ptr)
    return wav.view.view(b, length)


def hip_istft_bwd(bands, dwav, wav, spec, mask, window, inv, win, hop, length, mode):
    b, t = spec.shape[:2]
    dmask = bands.new("dmask", b * t * 256 * 2, BF16)
    call("sehip_istft_bwd", dwav.data_ptr(), wav.data_ptr(), spec.data_ptr(), mask.data_ptr(), window.data_ptr(), inv.data_ptr(), b, t,
         win, hop, 512, length, mode, dmask.ptr)
    return dmask.view.view(b, t, 256, 2)


def istft_round_trip(bands, what, spec_d, mask, dwav, win, hop, length, mode, win_type="hann", zero_mask=None):
    """forward and backward of one (mask, length, mode) on the device against float64 computed from the spectrum the kernel wrote;
    returns (float64 waveform before the clamp, the device waveform, the upstream gradient that was used)"""
    window = dev(R.window32(win, win_type))
    inv = dev(R.inv_energy(win, hop, spec_d.shape[1], length, win_type))
    spec = spec_d.cpu()
    y, add = R.istft(spec, mask, win, hop, length, mode, win_type)
    dwav = torch.where(R.near_limit(y), torch.zeros(()), dwav[:, :length])        # an fp32 sample may clamp where float64 does not
    mask_d, dwav_d = dev(mask), dev(dwav)
    out = hip_istft(bands, spec_d, mask_d, window, inv, win, hop, length, mode)
    dmask = hip_istft_bwd(bands, dwav_d, out, spec_d, mask_d, window, inv, win, hop, length, mode)
    bands.settle()
    err = check_sum(what + " waveform", out.cpu(), R.clamp(y), add)
    want = R.istft_dmask(spec, mask, dwav, win, hop, length, mode, win_type)
    if zero_mask is not None:                                                    # mode 0: NaN in the reference, defined as 0 in mask.h
        assert bool(torch.isnan(want[zero_mask]).all()) and bool((dmask.cpu()[zero_mask] == 0).all()), what
        want = torch.where(zero_mask, torch.zeros((), dtype=R.D), want)
    assert bool(torch.isfinite(want).all())
    check_small(what + " dmask", dmask.double().cpu(), want)
    return y, out.cpu(), dwav, err


# ------------------------------------------------------------------------------------------------------------------------------------
# STFT and iSTFT: geometries, window types, ragged frame counts, lengths
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,n", BN)
@pytest.mark.parametrize("win,hop,win_type", CONFIGS)
def test_stft_istft_geometries(win, hop, win_type, b, n):
    g = torch.Generator().manual_seed(1000 * win + n)
    bands = Bands()
    wav = 0.3 * torch.randn(b, n, generator=g)
    spec_d, enc = hip_stft(bands, dev(wav), dev(R.window32(win, win_type)), win, hop)
    bands.settle()
    want, add = R.stft(wav, win, hop, win_type)
    t = want.shape[1]
    worst = [check_sum("spec", spec_d.cpu(), want, add), 0.0]
    check_small(f"enc {win}/{hop}/{win_type}", enc.double().cpu(), want[:, :, 1:])
    for mode in (0, 1, 2):
        for length in sorted({n, 1, t * hop}):
            mask = 0.7 * torch.randn(b, t, 256, 2, generator=g)
            dwav = torch.randn(b, t * hop, generator=g)
            worst[1] = max(worst[1], istft_round_trip(bands, f"{win}/{hop}/{win_type} [{b}, {n}] mode {mode} length {length}", spec_d, mask,
                                                      dwav, win, hop, length, mode, win_type)[3])
    print(f"{win}/{hop}/{win_type} [{b}, {n}]: {b * t} frames; spectrum {worst[0]:.1e}, waveform {worst[1]:.1e} of the absolute addends "
          f"(gate {SUM_TOL:.0e})")


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_clamp_is_active(mode):
    win, hop = R.CLAMP_GEOM
    bands = Bands()
    wav, mask, dwav = R.clamp_inputs(mode)
    n = wav.shape[1]
    spec_d, _ = hip_stft(bands, dev(wav), dev(R.window32(win)), win, hop)
    y, out, used, err = istft_round_trip(bands, f"clamp mode {mode}", spec_d, mask, dwav, win, hop, n, mode)
    share, near = float((y.abs() > 1).double().mean()), float((used != dwav).double().mean())
    print(f"clamp mode {mode}: {100 * share:.1f} % of the samples clamp, upstream zeroed on {100 * near:.4f} %; waveform {err:.1e} of the "
          f"absolute addends (gate {SUM_TOL:.0e})")
    assert 0.05 < share < 0.60 and near <= 1e-3
    over = y.abs() > 1 + 1e-4
    assert torch.equal(out[over], torch.sign(y[over]).float())                   # exactly +-1
    assert bool((out.abs() <= 1).all())


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_digital_silence(mode):
    bands = Bands()
    wav, mask, dwav = R.silence_inputs()
    spec_d, enc = hip_stft(bands, dev(wav), dev(R.window32(400)), 400, 100)
    bands.settle()
    want, add = R.stft(wav, 400, 100)
    spec_err = check_sum("spec", spec_d.cpu(), want, add)                        # all-zero frames: no addends, exactly 0
    silent = add.sum((-1, -2)) == 0
    assert min(int(v) for v in silent.sum(-1)) >= 10 and bool((spec_d.cpu()[silent] == 0).all()) and bool((enc.cpu()[silent] == 0).all())
    zero = None
    if mode == 0:
        zero = torch.zeros(mask.shape, dtype=torch.bool)
        zero[:, :, R.SILENT_ROWS] = True
    err = istft_round_trip(bands, f"silence mode {mode}", spec_d, mask, dwav, 400, 100, 4000, mode, zero_mask=zero)[3]
    print(f"silence mode {mode}: all-zero frames per row {[int(v) for v in silent.sum(-1)]} of {silent.shape[1]}; spectrum {spec_err:.1e}, "
          f"waveform {err:.1e} of the absolute addends (gate {SUM_TOL:.0e})")


# ------------------------------------------------------------------------------------------------------------------------------------
# SI-SNR
# ------------------------------------------------------------------------------------------------------------------------------------
UP = 3.0


def hip_sisnr(bands, est_d, ref_d, upstream=UP):
    rows, n = est_d.shape
    rowstat, loss, dest = bands.new("rowstat", rows * 4), bands.new("loss", 1), bands.new("dest", rows * n)
    up = torch.full((1,), upstream, device="cuda")
    call("sehip_sisnr_fwd", est_d.data_ptr(), ref_d.data_ptr(), rows, n, rowstat.ptr, loss.ptr)
    call("sehip_sisnr_bwd", est_d.data_ptr(), ref_d.data_ptr(), rowstat.ptr, up.data_ptr(), rows, n, dest.ptr)
    bands.settle()
    return float(loss.view), rowstat.view.view(rows, 4)[:, 2].cpu(), dest.view.view(rows, n).cpu()


def gate_sisnr(what, est, ref, got, per_row=False):
    loss, rows, grad = got
    l64, r64, g64 = R.sisnr(est, ref, UP)
    l32, r32, g32 = R.sisnr(est, ref, UP, torch.float32)
    R.check_db(what + " loss", loss, l64, R.db_bound(l32, l64, SUM_TOL))
    R.check_db(what + " rows", rows, r64, R.db_bound(r32, r64, SUM_TOL))
    if per_row:
        for i in range(est.shape[0]):
            err = R.check_rel(f"{what} gradient of row {i} at {float(r64[i]):.1f} dB", grad[i], g64[i], R.rel_bound(g32[i], g64[i]))
            print(f"    {err / max(R.rel(g32[i], g64[i]), 1e-30):.2f} x the fp32 oracle's deviation")
    else:
        err = R.check_rel(what + " gradient", grad, g64, R.rel_bound(g32, g64))
        print(f"    {err / max(R.rel(g32, g64), 1e-30):.2f} x the fp32 oracle's deviation")
    return g64


@pytest.mark.parametrize("rows,n", [(1, 1), (3, 257), (5, 1023), (3, 1028), (2, 4100), (70, 64)])
def test_sisnr_shapes(rows, n):
    """n = 1028, 4100: the vectorised loop, one and two trips of 1024 float4; 257, 1023: the scalar loop; 70 rows: a second trip of the
    finalize kernel's 64-row step"""
    est, ref = R.noisy_pair((rows, n), rows + n)
    gate_sisnr(f"[{rows}, {n}]", est, ref, hip_sisnr(Bands(), dev(est), dev(ref)))


@pytest.mark.parametrize("off_est,off_ref", [(1, 0), (0, 1), (1, 1)])
def test_sisnr_rows_off_the_16_byte_boundary(off_est, off_ref):
    est, ref = R.noisy_pair((2, 4096), 11)
    on_dev = []
    for t, off in ((est, off_est), (ref, off_ref)):
        buf = torch.zeros(2 * 4096 + 4, device="cuda")
        view = buf[off:off + 2 * 4096].view(2, 4096)
        view.copy_(t)
        assert view.data_ptr() % 16 == 4 * off and view.is_contiguous()
        on_dev.append(view)
    gate_sisnr(f"[2, 4096] est + {4 * off_est} B, ref + {4 * off_ref} B", est, ref, hip_sisnr(Bands(), *on_dev))


def test_sisnr_gradient_at_high_snr():
    est, ref = R.snr_batch()
    gate_sisnr("0 / 20 / 40 / 60 dB", est, ref, hip_sisnr(Bands(), dev(est), dev(ref)), per_row=True)


def test_sisnr_silent_rows():
    est, ref = R.silent_row_batch()
    got = hip_sisnr(Bands(), dev(est), dev(ref))
    g64 = gate_sisnr("silent rows", est, ref, got)
    assert bool((g64[[1, 2, 4]] == 0).all()) and bool((got[2][[1, 2, 4]] == 0).all()) and bool(torch.isfinite(got[2]).all())


# ------------------------------------------------------------------------------------------------------------------------------------
# permutation-invariant SI-SNR
# ------------------------------------------------------------------------------------------------------------------------------------
def hip_pit(bands, est_d, tgt_d):
    b, s, c, n = est_d.shape
    rowstat, pair = bands.new("rowstat", s * s * b * c * 4), bands.new("pairloss", s * s)
    perm, loss, dest = bands.new("perm", s, torch.int32), bands.new("loss", 1), bands.new("dest", est_d.numel())
    up = torch.full((1,), UP, device="cuda")
    call("sehip_sisnr_pit_fwd", est_d.data_ptr(), tgt_d.data_ptr(), b, s, c, n, rowstat.ptr, pair.ptr, perm.ptr, loss.ptr)
    call("sehip_sisnr_pit_bwd", est_d.data_ptr(), tgt_d.data_ptr(), rowstat.ptr, perm.ptr, up.data_ptr(), b, s, c, n, dest.ptr)
    bands.settle()
    return float(loss.view), perm.view.cpu().tolist(), pair.view.view(s, s).cpu(), dest.view.view(est_d.shape).cpu()


@pytest.mark.parametrize("shape", R.PIT_SHAPES)
def test_pit_speaker_counts(shape):
    """S = 1, 2, 4 and PIT_MAXS = 6 (720 permutations in the single-thread walk); [35, 2, 2, 64]: 70 rows per pair, a second trip of the
    select kernel's 64-row step"""
    est, tgt = R.pit_inputs(shape)
    loss, perm, pair, grad = hip_pit(Bands(), dev(est), dev(tgt))
    l64, p64, m64, g64 = R.pit(est, tgt, UP)
    l32, p32, m32, g32 = R.pit(est, tgt, UP, torch.float32)
    gap = R.pit_gap(m64)[0]
    print(f"{shape}: gap {gap:.1f} dB, permutation {perm}")
    assert gap > 1.0 and perm == p64 == p32
    R.check_db(f"{shape} pair matrix", pair, m64, R.db_bound(m32, m64, SUM_TOL))
    R.check_db(f"{shape} loss", loss, l64, R.db_bound(l32, l64, SUM_TOL))
    err = R.check_rel(f"{shape} gradient", grad, g64, R.rel_bound(g32, g64))
    print(f"    {err / R.rel(g32, g64):.2f} x the fp32 oracle's deviation")


def test_pit_tie_keeps_the_first_permutation():
    est, tgt = R.pit_tie_inputs()
    loss, perm, pair, grad = hip_pit(Bands(), dev(est), dev(tgt))
    l64, p64, m64, g64 = R.pit(est, tgt, UP)
    l32, _, m32, g32 = R.pit(est, tgt, UP, torch.float32)
    assert torch.equal(pair[0], pair[1]) and perm == p64 == [0, 1]                # strict '<': the first of itertools.permutations
    R.check_db("tie loss", loss, l64, R.db_bound(l32, l64, SUM_TOL))
    R.check_rel("tie gradient", grad, g64, R.rel_bound(g32, g64))


# ------------------------------------------------------------------------------------------------------------------------------------
# SI-SDR metric
# ------------------------------------------------------------------------------------------------------------------------------------
def hip_si_sdr(reference, estimation):
    rows, n = reference.shape
    bands = Bands()
    ratios, out = bands.new("ratios", rows), bands.new("out", 1)
    r, e = dev(reference), dev(estimation)
    call("sehip_sisdr_metric", r.data_ptr(), e.data_ptr(), rows, n, ratios.ptr, out.ptr)
    bands.settle()
    return float(out.view)


def metric_cases():
    cases = {}
    for shape in ((70, 64), (3, 16000), (1, 8)):
        est, ref = R.noisy_pair(shape, 5 + shape[0])
        cases[str(shape)] = (ref, est)
    est, ref = R.silent_row_batch()
    cases["silent rows among others"] = (ref, est)
    cases["all silent"] = (torch.zeros(2, 100), torch.zeros(2, 100))
    return cases


@pytest.mark.parametrize("case", ["(70, 64)", "(3, 16000)", "(1, 8)", "silent rows among others", "all silent"])
def test_si_sdr_metric(case):
    import numpy as np
    ref, est = metric_cases()[case]
    got = hip_si_sdr(ref, est)
    want = R.si_sdr_metric(ref.numpy(), est.numpy())
    fp32 = R.si_sdr_metric(ref.numpy(), est.numpy(), np.float32)
    R.check_db(f"SI-SDR {case}: {got:.4f} dB (the fp32 numpy restatement is {abs(fp32 - want):.3e} dB off)", got, want,
               R.db_bound(fp32, want, SUM_TOL))


# ------------------------------------------------------------------------------------------------------------------------------------
# l1 / mse / psa
# ------------------------------------------------------------------------------------------------------------------------------------
def scalar_gate(what, got, want, oracle32):
    return R.check_rel(what, torch.tensor([got]), want.reshape(1), R.rel_bound(oracle32.reshape(1), want.reshape(1)))


@pytest.mark.parametrize("n", R.POINTWISE_SIZES)
@pytest.mark.parametrize("name", ["l1", "mse"])
def test_l1_mse_sizes(name, n):
    """1, 255, 257: below, at and above one workgroup; 4 194 304 + 4099: past both grid caps, a ragged last stride.  l1: 5 % of the
    elements equal, gradient exactly 0 there"""
    x, y = R.pointwise_inputs(n, equal_share=0.05 if name == "l1" else 0.0)
    mode = 0 if name == "l1" else 1
    bands = Bands()
    acc, loss, dx = bands.new("acc", 1, torch.float64), bands.new("loss", 1), bands.new("dx", n)
    xd, yd, up = dev(x), dev(y), torch.full((1,), UP, device="cuda")
    call("sehip_pointwise_loss_fwd", xd.data_ptr(), yd.data_ptr(), n, mode, acc.ptr, loss.ptr)
    call("sehip_pointwise_loss_bwd", xd.data_ptr(), yd.data_ptr(), n, mode, up.data_ptr(), dx.ptr)
    bands.settle()
    l64, g64 = R.pointwise(name, x, y, UP)
    l32, g32 = R.pointwise(name, x, y, UP, torch.float32)
    if float(l64) == 0.0:                                                        # n = 1 with the one element equal
        assert float(loss.view) == 0.0
    else:
        scalar_gate(f"{name} [{n}] loss", float(loss.view), l64, l32)
    R.check_rel(f"{name} [{n}] gradient", dx.view.cpu(), g64, R.rel_bound(g32, g64))
    if name == "l1":
        same = x == y
        assert (n < 255 or bool(same.any())) and bool((dx.view.cpu()[same] == 0).all()) and bool((dx.view.cpu()[~same] != 0).all())


@pytest.mark.parametrize("n", R.PSA_SIZES)
def test_psa_sizes(n):
    enh, tgt, mix = R.psa_inputs(n)
    bands = Bands()
    acc, loss, de = bands.new("acc", 1, torch.float64), bands.new("loss", 1), bands.new("denh", 2 * n)
    e, t, m, up = dev(enh), dev(tgt), dev(mix), torch.full((1,), UP, device="cuda")
    call("sehip_psa_loss_fwd", e.data_ptr(), t.data_ptr(), m.data_ptr(), n, acc.ptr, loss.ptr)
    call("sehip_psa_loss_bwd", e.data_ptr(), t.data_ptr(), m.data_ptr(), n, up.data_ptr(), de.ptr)
    bands.settle()
    l64, g64 = R.psa(enh, tgt, mix, UP)
    l32, g32 = R.psa(enh, tgt, mix, UP, torch.float32)
    scalar_gate(f"psa [{n}] loss", float(loss.view), l64, l32)
    R.check_rel(f"psa [{n}] gradient", de.view.view(n, 2).cpu(), g64, R.rel_bound(g32, g64))
