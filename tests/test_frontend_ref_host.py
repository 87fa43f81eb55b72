"""CPU: the float64 restatements of tests/frontend_ref.py against what the project already trusts (the fp32 oracle's conv_stft /
conv_istft at the four geometries of tests/test_gpu_frontend.py, and the stored vectors of the imported reference), the conditions on
every input of tests/test_gpu_frontend_edges.py (so that a failing condition shows without a GPU), and the evidence that each gate of that
file bites: the float64 reference is perturbed the way a fault would perturb the kernel -- no clamp in the backward, a truncated bf16
rounding, one dropped last sample of a row, a swapped permutation -- and the gate, with the fp32 oracle standing in for the kernel,
accepts the true reference and rejects the perturbed one."""
import numpy as np
import pytest
import torch

import frontend_ref as R
from oracle import dccrn_oracle as O
from test_gpu_frontend import GEOMETRIES
from test_gpu_wavunet import SUM_TOL, check_small, check_sum
from util import load_golden, max_abs, rel_err

EDGE_GEOMETRIES = [(398, 100), (396, 99), (64, 16)]
BN = [(1, 1), (3, 257), (5, 1999), (2, 4000)]


# ---- the restatement against the oracle and the stored vectors -------------------------------------------------------------------------
@pytest.mark.parametrize("win,hop", GEOMETRIES)
def test_stft_istft_restatement_equals_the_fp32_oracle(win, hop):
    g = torch.Generator().manual_seed(1)
    b, n = 2, 4000
    wav = 0.3 * torch.randn(b, n, generator=g)
    mask = 0.7 * torch.randn(b, R.frames_of(n, win, hop), 256, 2, generator=g)
    dwav = torch.randn(b, n, generator=g)
    spec64, _ = R.stft(wav, win, hop)
    for mode in (0, 1, 2):
        spec32, out32, dm32 = R.oracle32(wav, mask, dwav, win, hop, n, mode)
        assert rel_err(spec32, spec64) < 1e-6
        y, add = R.istft(spec32, mask, win, hop, n, mode)
        assert float(y.abs().max()) < 1.0 or mode == 1                           # (the clamp is all but idle on these inputs)
        assert rel_err(out32, R.clamp(y)) < 2e-6
        assert bool(((out32.double() - R.clamp(y)).abs() <= 2e-6 * add).all())
        assert rel_err(dm32, R.istft_dmask(spec32, mask, dwav, win, hop, n, mode)) < 1e-5


def test_bases_against_the_stored_rows():
    g = load_golden("stft_bases_rows.npz")
    a, s, w = R.bases(400)
    rows = g["rows"]
    assert max_abs(a[rows], g["stft"]) < 1e-6 and max_abs(s[rows], g["istft"]) < 1e-6 and max_abs(w, g["window"]) < 1e-7
    # the closed form the kernel uses: pinv(K) = (1 / 256) (I - c (1 1^T + s s^T)) K^T with c = 1 / (512 + win), s_n = (-1)^n
    for win in (400, 398, 396, 64, 512):
        a, s, w = R.bases(win, None)                                             # (window of ones: the bare bases)
        sign = torch.tensor([(-1.0) ** n for n in range(win)], dtype=R.D)
        one = torch.ones(win, dtype=R.D)
        closed = (torch.eye(win, dtype=R.D) - (torch.outer(one, one) + torch.outer(sign, sign)) / (512 + win)) @ a.t() / 256
        assert max_abs(closed.t(), s) < 1e-12, win


def test_losses_against_the_stored_vectors():
    g = load_golden("sisnr_cases.npz")
    for k in ("a", "b", "zero_target", "equal"):
        est, ref = torch.from_numpy(g[k + "/est"]), torch.from_numpy(g[k + "/ref"])
        loss, rows, _ = R.sisnr(est.reshape(-1, est.shape[-1]), ref.reshape(-1, ref.shape[-1]))
        want = float(g[k + "/si_snr"])
        assert abs(-float(loss) - want) < 2e-4 * max(1.0, abs(want)) and abs(float(rows.mean()) + float(loss)) < 1e-9, k
    g = load_golden("pit_cases.npz")
    seen = 0
    for case in ("s2_swap", "s2_id", "s3_rot", "s2_c2", "s2_l1", "s3_mse"):
        if str(g[case + ".lname"]) != "sisdr":
            continue
        est, tgt = torch.from_numpy(g[case + ".est"]), torch.from_numpy(g[case + ".tgt"])
        loss, perm, m, grad = R.pit(est, tgt)
        assert abs(float(loss) - float(g[case + ".loss"][0])) < 2e-5 * max(1.0, abs(float(g[case + ".loss"][0])))
        assert perm == [i for i, _ in sorted(g[case + ".comb"].tolist(), key=lambda p: p[1])] == R.pit_gap(m)[1]
        assert rel_err(grad, torch.from_numpy(g[case + ".grad"])) < 1e-5
        seen += 1
    assert seen >= 3
    for case in ("a", "b"):
        v = {k[2:]: torch.from_numpy(np.asarray(x)) for k, x in load_golden("psa_loss.npz").items() if k.startswith(case + "/")}
        loss, grad = R.psa(v["enh"], v["tgt"], v["mix"])
        assert abs(float(loss) - float(v["loss"])) < 1e-6 * abs(float(v["loss"])) and rel_err(grad, v["denh"]) < 1e-6


def test_si_sdr_metric_restatement():
    est, ref = R.noisy_pair((3, 16000), 5)
    assert abs(R.si_sdr_metric(ref.numpy(), est.numpy()) - R.si_sdr_metric(ref.numpy(), est.numpy(), np.float32)) < 1e-4
    z = np.zeros((2, 100), np.float32)
    assert abs(R.si_sdr_metric(z, z) - 10 * np.log10(R.SDR_EPS)) < 1e-9


# ---- the conditions on the inputs of the GPU tests ---------------------------------------------------------------------------------------
def test_shapes_reach_every_ragged_frame_count():
    seen = set()
    for win, hop in GEOMETRIES + EDGE_GEOMETRIES:
        frames = [b * R.frames_of(n, win, hop) for b, n in BN]
        assert all(f > 0 for f in frames)
        assert any(f % 4 for f in frames), (win, hop, frames)                     # every geometry has a partly filled last workgroup
        seen |= {f % 4 for f in frames}
    assert seen >= {1, 2, 3}                                                     # ... which holds 1, 2 and 3 frames over the set
    assert [w % 8 for w, _ in EDGE_GEOMETRIES] == [6, 4, 0] and [w % 4 for w, _ in EDGE_GEOMETRIES] == [2, 0, 0]


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_clamp_inputs_clamp(mode):
    win, hop = R.CLAMP_GEOM
    wav, mask, dwav = R.clamp_inputs(mode)
    spec32, _, _ = R.oracle32(wav, mask, dwav, win, hop, wav.shape[1], mode)
    y, _ = R.istft(spec32, mask, win, hop, wav.shape[1], mode)
    share, near = float((y.abs() > 1).double().mean()), float(R.near_limit(y).double().mean())
    print(f"mode {mode}: {100 * share:.1f} % of the samples clamp, {100 * near:.4f} % within 1e-4 of the limit")
    assert 0.05 < share < 0.60 and near <= 1e-3


def test_silence_inputs_are_silent():
    wav, mask, dwav = R.silence_inputs()
    counts = R.silent_frames(wav, 400, 100)
    print("all-zero frames per row:", counts, "of", R.frames_of(4000, 400, 100))
    assert min(counts) >= 10 and R.frames_of(4000, 400, 100) == 43
    assert bool((wav[:, -200:] == 0).all())                                      # a zeroed tail, as collate_fn_pad leaves it
    spec, add = R.stft(wav, 400, 100)
    silent = add.sum((-1, -2)) == 0
    assert [int(v) for v in silent.sum(-1)] == counts and bool((spec[silent] == 0).all())
    # mode 0: the reference gradient is NaN at the zero mask rows and only there, 4 of 256 bins
    dm = R.istft_dmask(spec.float(), mask, dwav, 400, 100, 4000, 0)
    nan = torch.isnan(dm)
    zero = torch.zeros_like(nan)
    zero[:, :, R.SILENT_ROWS] = True
    assert torch.equal(nan, zero) and abs(float(nan.double().mean()) - 4 / 256) < 1e-12
    for mode in (1, 2):
        assert bool(torch.isfinite(R.istft_dmask(spec.float(), mask, dwav, 400, 100, 4000, mode)).all())
    # the oracle's convention at silent bins (phase 0, +0) is what mask.h restates: magnitude sqrt(1e-8) times the mask's own phase
    est = R.apply_mask(spec.float().double(), mask.double(), 0)[silent]          # [frames, 514]
    m = mask.double()[silent]
    rho = (m[..., 0] ** 2 + m[..., 1] ** 2).sqrt()
    unit = torch.where(rho[..., None] > 0, m / rho[..., None].clamp(min=1e-300), torch.tensor([1.0, 0.0], dtype=R.D))
    want = torch.tanh(rho)[..., None] * 1e-4 * unit
    assert max_abs(est[:, 1:257], want[..., 0]) < 1e-18 and max_abs(est[:, 258:], want[..., 1]) < 1e-18


def test_sisnr_inputs():
    est, ref = R.snr_batch()
    _, rows, _ = R.sisnr(est, ref)
    assert max_abs(rows, torch.tensor(R.SNR_DB, dtype=R.D)) < 0.5                 # est is not orthogonal to the noise: within 0.5 dB
    est, ref = R.silent_row_batch()
    loss, rows, grad = R.sisnr(est, ref, 3.0)
    assert bool((ref[1] == 0).all() and (est[2] == 0).all() and (est[4] == 0).all() and (ref[4] == 0).all())
    assert bool(torch.isfinite(grad).all()) and bool((grad[[1, 2, 4]] == 0).all()) and bool((grad[[0, 3]] != 0).any())
    assert max_abs(rows[[1, 2, 4]], torch.full((3,), -80.0, dtype=R.D)) < 1e-6


def test_pit_inputs():
    for shape in R.PIT_SHAPES:
        est, tgt = R.pit_inputs(shape)
        _, perm, m, _ = R.pit(est, tgt)
        gap, best = R.pit_gap(m)
        print(shape, f"gap between the best and the second permutation {gap:.1f} dB, permutation {perm}")
        assert gap > 1.0 and perm == best == [(j + 1) % shape[1] for j in range(shape[1])]
    est, tgt = R.pit_tie_inputs()
    _, perm, m, _ = R.pit(est, tgt)
    assert torch.equal(est[:, 0], est[:, 1]) and torch.equal(m[0], m[1]) and R.pit_gap(m)[0] == 0.0 and perm == [0, 1]


def test_pointwise_inputs():
    assert R.POINTWISE_SIZES[-1] > R.CAP_FLOATS and R.PSA_SIZES[-1] == 2099201 and 2 * R.PSA_SIZES[-1] > R.CAP_FLOATS
    x, y = R.pointwise_inputs(R.POINTWISE_SIZES[-1], equal_share=0.05)
    share = float((x == y).double().mean())
    assert 0.045 < share < 0.055
    _, grad = R.pointwise("l1", x, y, 3.0)
    assert bool((grad[x == y] == 0).all()) and bool((grad[x != y] != 0).all())


# ---- every gate rejects a reference perturbed the way a fault would perturb the kernel --------------------------------------------------
def test_gate_rejects_a_backward_without_the_clamp():
    win, hop = R.CLAMP_GEOM
    for mode in (0, 1, 2):
        wav, mask, dwav = R.clamp_inputs(mode)
        n = wav.shape[1]
        spec32, _, _ = R.oracle32(wav, mask, dwav, win, hop, n, mode)
        y, _ = R.istft(spec32, mask, win, hop, n, mode)
        dwav = torch.where(R.near_limit(y), torch.zeros(()), dwav)
        _, out32, dm32 = R.oracle32(wav, mask, dwav, win, hop, n, mode)
        assert bool((out32[y.abs() > 1 + 1e-4].abs() == 1).all())
        standin = dm32.bfloat16().double()
        check_small(f"mode {mode} dmask", standin, R.istft_dmask(spec32, mask, dwav, win, hop, n, mode))
        with pytest.raises(AssertionError):
            check_small(f"mode {mode} dmask, no clamp", standin, R.istft_dmask(spec32, mask, dwav, win, hop, n, mode, clamped=False))


def test_gate_rejects_a_truncated_bf16_rounding():
    for (b, n) in [(3, 257), (2, 4000)]:
        wav = 0.3 * torch.randn(b, n, generator=torch.Generator().manual_seed(2))
        spec32, _, _ = R.oracle32(wav, torch.zeros(b, R.frames_of(n, 400, 100), 256, 2), torch.zeros(b, n), 400, 100, n, 1)
        want = R.stft(wav, 400, 100)[0][:, :, 1:]
        check_small("enc", spec32[:, :, 1:].bfloat16().double(), want)
        with pytest.raises(AssertionError):                                      # the kernel's stand-in truncates
            check_small("enc, truncated", R.bf16_truncate(spec32[:, :, 1:]).double(), want)
        with pytest.raises(AssertionError):                                      # the same fault planted in the reference
            check_small("enc, reference half an ulp up", spec32[:, :, 1:].bfloat16().double(), R.bf16_half_ulp_up(want))


def test_gates_reject_one_dropped_last_sample():
    # fp32 sums: the last sample of every waveform row missing from the reference
    wav = 0.3 * torch.randn(3, 257, generator=torch.Generator().manual_seed(3))
    spec32, _, _ = R.oracle32(wav, torch.zeros(3, R.frames_of(257, 400, 100), 256, 2), torch.zeros(3, 257), 400, 100, 257, 1)
    spec, add = R.stft(wav, 400, 100)
    live = add > 0                                                               # (the oracle's fp32 basis is not exactly 0 where sin is)
    check_sum("spec", spec32[live], spec[live], add[live])
    short = wav.clone()
    short[:, -1] = 0.0
    with pytest.raises(AssertionError):
        check_sum("spec, last sample dropped", spec32[live], R.stft(short, 400, 100)[0][live], add[live])
    # ... and the last frame missing from the reference of the waveform (modes 'C' and 'E')
    mask = 0.7 * torch.randn(3, spec.shape[1], 256, 2, generator=torch.Generator().manual_seed(4))
    for mode in (1, 0):
        _, out32, _ = R.oracle32(wav, mask, torch.zeros(3, 257), 400, 100, 257, mode)
        y, add_y = R.istft(spec32, mask, 400, 100, 257, mode)
        check_sum("waveform", out32, R.clamp(y), add_y)
        short_mask = mask.clone()
        short_mask[:, -1] = 0.0                                                  # (a zero mask row silences the frame in both modes)
        with pytest.raises(AssertionError):
            check_sum("waveform, last frame dropped", out32, R.clamp(R.istft(spec32, short_mask, 400, 100, 257, mode)[0]), add_y)
    # losses: the reference computed on rows without their last sample
    for shape, seed in [((3, 257), 4), ((2, 4100), 5)]:
        est, ref = R.noisy_pair(shape, seed)
        loss, rows, grad = R.sisnr(est, ref, 3.0)
        _, rows32, grad32 = R.sisnr(est, ref, 3.0, torch.float32)
        gb, rb = R.rel_bound(grad32, grad), R.db_bound(rows32, rows, SUM_TOL)
        R.check_rel("gradient", grad32, grad, gb)
        R.check_db("rows", rows32, rows, rb)
        _, rows_s, grad_s = R.sisnr(est[:, :-1], ref[:, :-1], 3.0)
        with pytest.raises(AssertionError):
            R.check_rel("gradient, last sample dropped", grad32, torch.nn.functional.pad(grad_s, [0, 1]), gb)
        with pytest.raises(AssertionError):
            R.check_db("rows, last sample dropped", rows32, rows_s, rb)
    x, y = R.pointwise_inputs(257)
    for name in ("l1", "mse"):
        loss, grad = R.pointwise(name, x, y, 3.0)
        loss32, grad32 = R.pointwise(name, x, y, 3.0, torch.float32)
        lb, gb = R.rel_bound(loss32, loss), R.rel_bound(grad32, grad)
        R.check_rel(name, loss32, loss, lb)
        loss_s, grad_s = R.pointwise(name, x[:-1], y[:-1], 3.0)
        with pytest.raises(AssertionError):
            R.check_rel(name + ", last sample dropped", loss32, loss_s, lb)
        with pytest.raises(AssertionError):
            R.check_rel(name + " gradient, last sample dropped", grad32, torch.nn.functional.pad(grad_s, [0, 1]), gb)


def test_gates_reject_one_dropped_psa_element():
    enh, tgt, mix = R.psa_inputs(257)
    loss, grad = R.psa(enh, tgt, mix, 3.0)
    loss32, grad32 = R.psa(enh, tgt, mix, 3.0, torch.float32)
    lb, gb = R.rel_bound(loss32, loss), R.rel_bound(grad32, grad)
    R.check_rel("psa", loss32, loss, lb)
    R.check_rel("psa gradient", grad32, grad, gb)
    loss_s, grad_s = R.psa(enh[:-1], tgt[:-1], mix[:-1], 3.0)
    with pytest.raises(AssertionError):
        R.check_rel("psa, last element dropped", loss32, loss_s, lb)
    with pytest.raises(AssertionError):
        R.check_rel("psa gradient, last element dropped", grad32, torch.nn.functional.pad(grad_s, [0, 0, 0, 1]), gb)


def test_gates_reject_a_swapped_permutation():
    est, tgt = R.pit_inputs((3, 2, 2, 301))
    loss, perm, m, grad = R.pit(est, tgt, 3.0)
    loss32, perm32, m32, grad32 = R.pit(est, tgt, 3.0, torch.float32)
    lb, mb, gb = R.db_bound(loss32, loss, SUM_TOL), R.db_bound(m32, m, SUM_TOL), R.rel_bound(grad32, grad)
    assert perm32 == perm
    R.check_db("loss", loss32, loss, lb)
    R.check_db("pair matrix", m32, m, mb)
    R.check_rel("gradient", grad32, grad, gb)
    loss_w, perm_w, m_w, grad_w = R.pit(est, tgt, 3.0, force_perm=perm[::-1])
    assert perm32 != perm_w
    with pytest.raises(AssertionError):
        R.check_db("loss, swapped", loss32, loss_w, lb)
    with pytest.raises(AssertionError):
        R.check_rel("gradient, swapped", grad32, grad_w, gb)
    with pytest.raises(AssertionError):
        R.check_db("pair matrix, transposed", m32, m.t(), mb)
