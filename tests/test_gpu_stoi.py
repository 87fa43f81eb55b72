"""GPU: sehip.metric.STOI / stoi_rows (csrc/stoi.hip) against tests/stoi_ref.py, the float64 restatement of the published algorithm
(`pystoi` is not available here: parity with it is by that restatement only).

Resampler and frame selection are checked op-local (fp32 dot-product bound; exact indices), the band magnitudes and the value against
a gate that is COMPUTED here: G = 8 x the largest deviation of the oracle's own float32 restatement from its float64 over this file's
cases (the device sums in another order and has its own FFT and resampler rounding; one restatement is one sample of that error), and
G must stay under 1e-5 or the test is ill-posed.  Measured on an MI355X (this file's cases): see DESIGN.md section 17.
Signals: tests/stoi_ref.py am_signal, a seeded sum of five amplitude-modulated sines plus noise."""
import numpy as np
import pytest
import torch

import stoi_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64
RESAMPLE_CASES = ((16000, 1003), (48000, 2001), (44100, 1777), (8000, 999))
# (sr, n): the three smallest give T = 29, 30, 31 frames for a row that keeps every frame; 40000 samples at 10 kHz are 311 frames (two
# rounds of the selection scan, 18 / 36 blocks of segments); the rest are half a second through each resampler
VALUE_CASES = ((10000, 4095), (10000, 4223), (10000, 4351), (10000, 40000), (16000, 8000), (48000, 24000), (44100, 22050), (8000, 4000))
SELECT_KINDS = ("none", "mid", "start", "end", "alt", "near")
_cache = {}


def gapped(x, kind, sr):
    """x with a part turned down: 1e-4 (80 dB, far below the 40 dB range) or, 'near', 0.015 (frames on both sides of the threshold)"""
    x, n = x.copy(), len(x)
    if kind == "mid":
        x[int(0.4 * n):int(0.6 * n)] *= 1e-4
    elif kind == "start":
        x[:int(0.25 * n)] *= 1e-4
    elif kind == "end":
        x[int(0.75 * n):] *= 1e-4
    elif kind == "alt":                                   # every other pair of frames (256 samples at 10 kHz)
        blk = int(round(256 * sr / 10000))
        for i in range(0, n, 2 * blk):
            x[i:i + blk] *= 1e-4
    elif kind == "near":
        x[int(0.4 * n):int(0.6 * n)] *= 0.015
    elif kind == "short":                                 # fewer than 30 frames are left
        x[int(0.2 * sr):] *= 1e-4                         # 0.2 s: 2000 samples at 10 kHz
    else:
        assert kind == "none"
    return x


def value_case(sr, n):
    """four pairs of one call -- every frame kept, a gap, fewer than 30 frames, all zero -- and the oracle's float64 and float32 steps
    for both variants; computed once and shared"""
    key = (sr, n)
    if key not in _cache:
        rng = np.random.RandomState(7 + sr % 1000 + n)
        base = R.am_signal(n, sr, seed=n + sr)
        xs = [gapped(base, "none", sr), gapped(R.am_signal(n, sr, seed=n + sr + 1), "mid", sr), gapped(base, "short", sr), np.zeros(n)]
        ys = [x + 0.03 * rng.randn(n) for x in xs[:3]] + [0.03 * rng.randn(n)]
        xs = [x.astype(np.float32) for x in xs]           # the device's inputs ARE float32: the oracle gets the same samples
        ys = [y.astype(np.float32) for y in ys]
        steps = {(ext, dt): [R.stoi_steps(x, y, sr, ext, dt) for x, y in zip(xs, ys)]
                 for ext in (False, True) for dt in (np.float64, np.float32)}
        _cache[key] = (np.stack(xs), np.stack(ys), steps)
    return _cache[key]


def gates():
    """G for d and for the band magnitudes (relative to the row's largest), from the float32 restatement over every case of the file"""
    if "gates" not in _cache:
        gd = gt = 0.0
        for sr, n in VALUE_CASES:
            _, _, steps = value_case(sr, n)
            for ext in (False, True):
                for s64, s32 in zip(steps[(ext, np.float64)], steps[(ext, np.float32)]):
                    assert np.array_equal(s64["src"], s32["src"])
                    gd = max(gd, abs(float(s32["d"]) - float(s64["d"])))
                    for k in ("x_tob", "y_tob"):
                        if s64[k].size and s64[k].max() > 0:
                            gt = max(gt, float(np.abs(s32[k] - s64[k]).max() / s64[k].max()))
        _cache["gates"] = (8 * gd, 8 * gt)
    return _cache["gates"]


def test_value_cases_are_what_they_claim():
    """input checks on the oracle alone: the frame counts, the row kinds and the margins from the selection threshold"""
    want_t = {4095: 29, 4223: 30, 4351: 31}
    for sr, n in VALUE_CASES:
        _, _, steps = value_case(sr, n)
        rows = steps[(False, np.float64)]
        if n in want_t:
            assert rows[0]["T"] == want_t[n]
        else:
            assert rows[0]["T"] >= 30 and 30 <= rows[1]["T"] < rows[0]["T"]
        assert rows[2]["T"] < 30 and rows[2]["d"] == 1e-5
        assert rows[3]["mask"].all() and rows[3]["d"] == (0.0 if rows[3]["T"] >= 30 else 1e-5)
        for r in rows[:3]:
            assert np.abs(R.threshold_margin(r["levels"])).min() >= 0.01
    gd, gt = gates()
    print(f"[stoi] gate d {gd:.3e}  gate tob {gt:.3e}")
    assert 0 < gd <= 1e-5 and 0 < gt <= 1e-5, (gd, gt)


# ---- resampler, op-local ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr,n", RESAMPLE_CASES)
def test_resample_within_the_fp32_dot_product_bound(sr, n):
    from sehip import metric
    from sehip._lib import call, ptr, stream
    dev = torch.device("cuda")
    x = np.stack([R.am_signal(n, sr, seed=sr + i).astype(np.float32) for i in range(4)])       # 2 clean rows, 2 estimate rows
    table, p, q, L = metric.stoi_resample_table(sr, dev)
    m = metric.stoi_out_len(n, sr)
    assert m == R.out_len(n, sr)
    kt = 2 * L // p + 1
    xd = torch.from_numpy(x).to(dev)
    outs = []
    for _ in range(2):
        buf = torch.full((4 * m + GUARD,), 12345.0, device=dev)
        call("sehip_stoi_resample", ptr(xd[:2].contiguous()), ptr(xd[2:].contiguous()), 2, n, ptr(table), p, q, L, ptr(buf), stream())
        outs.append(buf.cpu())
    assert torch.equal(outs[0], outs[1])                          # run-to-run bits
    assert bool((outs[0][4 * m:] == 12345.0).all())               # guard words
    got = outs[0][:4 * m].reshape(4, m).double().numpy()
    worst = 0.0
    for i in range(4):
        want = R.resample(x[i], sr)
        bound = (kt + 2) * 2.0 ** -24 * R.resample(x[i], sr, absolute=True)      # p sum |w| |x| with p folded into the table
        err = np.abs(got[i] - want)
        worst = max(worst, float((err / bound).max()))
        assert bool((err <= bound).all()), (sr, i, int(err.argmax()), float(err.max()))
    print(f"[stoi] resample {sr}: worst error / bound {worst:.3e} (taps per output {kt})")


# ---- selection, op-local and exact ----------------------------------------------------------------------------------------------------
def test_selection_equals_the_oracle():
    from sehip._lib import call, lib, ptr, stream
    dev = torch.device("cuda")
    sr, n = 16000, 8000
    base = R.am_signal(n, sr, seed=3)
    x10 = np.stack([R.resample(gapped(base, k, sr), sr).astype(np.float32) for k in SELECT_KINDS])
    want = []
    for kind, row in zip(SELECT_KINDS, x10):
        e, _ = R.levels(row)
        mg = R.threshold_margin(e)
        assert np.abs(mg).min() >= 0.01, (kind, float(np.abs(mg).min()))          # input check: no frame sits on the threshold
        if kind == "near":
            assert mg[mg > 0].min() < 1 and (-mg[mg < 0]).min() < 1               # a kept and a dropped frame within 1 dB of it
        want.append(R.select(e)[1])
    assert len(want[0]) == 38 and len({len(w) for w in want}) >= 4
    rows, n10 = x10.shape
    frames = lib().sehip_stoi_frames(n10)
    assert frames == R.frame_count(n10)
    xd = torch.from_numpy(x10).to(dev)
    level = torch.empty(rows, frames, device=dev)
    kept = torch.full((rows,), -1, device=dev, dtype=torch.int32)
    src = torch.full((rows, frames), -1, device=dev, dtype=torch.int32)
    call("sehip_stoi_levels", ptr(xd), rows, n10, ptr(level), stream())
    call("sehip_stoi_select", ptr(level), rows, frames, ptr(kept), ptr(src), stream())
    kept, src, level = kept.cpu().numpy(), src.cpu().numpy(), level.cpu().numpy()
    for i, kind in enumerate(SELECT_KINDS):
        e, _ = R.levels(x10[i])
        assert np.abs(level[i] - e).max() < 1e-3, (kind, float(np.abs(level[i] - e).max()))   # dB; the margins above are >= 0.01
        assert kept[i] == len(want[i]), (kind, kept[i], len(want[i]))
        assert np.array_equal(src[i, :kept[i]], want[i]), kind
        assert bool((src[i, kept[i]:] == -1).all()), kind          # nothing is written past the row's count


# ---- band magnitudes and the value ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extended", [False, True])
@pytest.mark.parametrize("sr,n", VALUE_CASES)
def test_bands_and_value_within_the_gate(sr, n, extended):
    from sehip import metric
    dev = torch.device("cuda")
    gd, gt = gates()
    assert 0 < gd <= 1e-5 and 0 < gt <= 1e-5, (gd, gt)             # else the comparison is ill-posed
    xs, ys, steps = value_case(sr, n)
    want = steps[(extended, np.float64)]
    x, y = torch.from_numpy(xs).to(dev).reshape(2, 2, n), torch.from_numpy(ys).to(dev).reshape(2, 2, n)
    d = metric.stoi_rows(x, y, sr=sr, extended=extended)
    mean = metric.STOI(x, y, sr=sr, extended=extended)
    assert d.shape == (4,) and mean.dim() == 0 and d.dtype == mean.dtype == torch.float32
    ws = metric.stoi_workspace(4, n, sr, x.device)
    kept, src, tob = ws["kept"].cpu().numpy(), ws["src"].cpu().numpy(), ws["tob"].cpu().double().numpy()
    d = d.cpu().numpy()
    dev_d = dev_t = 0.0
    for i, st in enumerate(want):
        assert kept[i] == len(st["src"]) and np.array_equal(src[i, :kept[i]], st["src"]), i
        t = st["T"]
        for sig, key in enumerate(("x_tob", "y_tob")):
            if t > 0 and st[key].max() > 0:
                dev_t = max(dev_t, float(np.abs(tob[sig, i, :, :t] - st[key]).max() / st[key].max()))
        dev_d = max(dev_d, abs(float(d[i]) - float(st["d"])))
    print(f"[stoi] sr {sr} n {n} extended {extended}: |d - oracle| {dev_d:.3e} (gate {gd:.3e})  tob {dev_t:.3e} (gate {gt:.3e})")
    assert want[3]["d"] == (0.0 if want[3]["T"] >= 30 else 1e-5)
    assert d[2] == np.float32(1e-5) and d[3] == np.float32(want[3]["d"])      # exact: the too-few-frames rows and the zero row
    assert bool((tob[0, 3, :, :want[3]["T"]] == 0).all())
    assert dev_t <= gt, (dev_t, gt)
    assert dev_d <= gd, (dev_d, gd)
    assert abs(float(mean) - float(np.mean([float(s["d"]) for s in want]))) <= gd
    # the mean of four values <= 1: three fp32 additions below 4 (half an ulp of 4 each, 2^-22), a quarter of that, one division
    assert abs(float(mean) - float(d.astype(np.float64).mean())) <= 3 * 2.0 ** -24 + 2.0 ** -24


def test_refusals_and_no_grad():
    from sehip import STOI, SehipError
    dev = torch.device("cuda")
    x = torch.zeros(1, 1, 8000, device=dev)
    with pytest.raises(SehipError):
        STOI(x[..., :408], x[..., :408], sr=16000)                 # 255 samples at 10 kHz
    with pytest.raises(SehipError):
        STOI(x, x, sr=0)
    with pytest.raises(SehipError):
        STOI(x, x, sr=16001)
    with pytest.raises(ValueError):
        STOI(x, x[..., :4000])
    with pytest.raises(SehipError):
        STOI(x, x.clone().requires_grad_(True))
    assert not STOI(x, x).requires_grad


# ---- graph ------------------------------------------------------------------------------------------------------------------------------
def test_graph_replay_equals_eager_bit_for_bit():
    from sehip import STOI
    from sehip.metric import stoi_rows
    dev = torch.device("cuda")
    sr, n = 16000, 8000
    base = R.am_signal(n, sr, seed=11)
    noise = 0.03 * np.random.RandomState(12).randn(2, n)
    plain = np.stack([base, R.am_signal(n, sr, seed=13)])
    gap = np.stack([gapped(plain[0], "mid", sr), gapped(plain[1], "start", sr)])
    to = lambda a: torch.from_numpy(a.astype(np.float32)).to(dev).reshape(2, 1, n)
    x, y = to(plain), to(plain + noise)
    eager_plain = [STOI(x, y, sr=sr).clone() for _ in range(2)]
    eager_gap = [STOI(to(gap), to(gap + noise), sr=sr).clone() for _ in range(2)]
    rows_gap = stoi_rows(to(gap), to(gap + noise), sr=sr).clone()
    assert torch.equal(eager_plain[0], eager_plain[1]) and torch.equal(eager_gap[0], eager_gap[1])     # run-to-run bits
    assert not torch.equal(eager_plain[0], eager_gap[0])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                       # (captures on a side stream)
        out = STOI(x, y, sr=sr)
    g.replay()
    assert torch.equal(out, eager_plain[0])
    x.copy_(to(gap))
    y.copy_(to(gap + noise))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager_gap[0])
    assert torch.equal(stoi_rows(x, y, sr=sr), rows_gap)


# ---- Solver -----------------------------------------------------------------------------------------------------------------------------
KW = dict(kernel_num=[16, 16, 32, 32, 64, 64], rnn_units=128, length=8000)


def solver_config(tmp, metric):
    from sehip.utils import dict2obj
    return dict2obj({
        "seed": 10, "root": None, "ha": None,
        "model": dict(name="dccrn", audio_channels=1, num_spk=1, **KW),
        "optim": {"optim": "adam", "lr": 3e-4, "beta1": 0.9, "beta2": 0.999, "loss": "si-sdr", "clip_grad": 5, "pit": False, "load": True},
        "dset": {"name": "synthetic", "sample_rate": 16000},
        # (fixed-order reductions: the two forward passes the test compares are the same bits)
        "solver": {"epochs": 1, "cudnn_deterministic": True, "save_checkpoint_interval": 1, "all_steps": True, "total_steps": 0, "patience": 0, "root": str(tmp),
                   "resume": None, "preloaded_model": None, "validation": {"interval": 1, "metric": metric, "total_steps": 0},
                   "test": {"interval": 1}},
    })


@pytest.fixture
def deterministic_switch():
    """the Solver's cudnn_deterministic sets a process-wide library switch: put it back for the tests that run after this file"""
    from sehip._lib import lib
    from sehip.utils import set_deterministic
    before = bool(lib().sehip_get_deterministic())
    yield
    set_deterministic(before)


def make_solver(tmp, metric):
    from sehip import distrib
    from sehip.solver import Solver, ScalarLog
    cfg = solver_config(tmp, metric)
    torch.manual_seed(cfg.seed)
    model = distrib.get_model(cfg.model)
    opt = distrib.get_optimizer(cfg.optim, model)
    batches = []
    for s in range(2):
        clean = np.stack([R.am_signal(8000, 16000, seed=20 + 2 * s + i) for i in range(2)]).astype(np.float32)
        noisy = clean + 0.03 * np.random.RandomState(30 + s).randn(2, 8000).astype(np.float32)
        batches.append((torch.from_numpy(noisy).reshape(2, 1, 8000), torch.from_numpy(clean).reshape(2, 1, 1, 8000), [None], [None], ["x"], [s]))
    solver = Solver(cfg, model, opt, distrib.get_loss_function(cfg.optim), train_dataloader=batches, validation_dataloader=batches,
                    device="gpu", writer=ScalarLog())
    return solver, batches


def test_solver_validates_by_stoi(tmp_path, deterministic_switch):
    from sehip import STOI
    solver, batches = make_solver(tmp_path, "stoi")
    dev = solver.device
    assert solver.find_max
    score = solver._run_one_epoch(0, 1, train=False)
    assert isinstance(score, float) and solver.score["stoi"] == score
    direct = []
    solver.model.eval()
    with torch.no_grad():
        for noisy, clean, *_ in batches:
            enhanced = solver.model(noisy.to(dev))
            direct.append(float(STOI(clean.to(dev).squeeze(1), enhanced, sr=16000)))
    assert score == (direct[0] + direct[1]) / 2, (score, direct)
    assert 0 < score < 1
    assert solver._is_best(score, find_max=solver.find_max) and solver.score["best_score"] == score
    # compute_metric: src/solver.py:704-721 on device tensors
    noisy, clean = batches[0][0].to(dev), batches[0][1].to(dev).squeeze(1)
    sc, ref = solver.compute_metric(noisy, enhanced=clean, clean=clean)
    for dct in (sc, ref):
        assert sorted(dct) == ["sisdr", "stoi"]
        assert all(len(v) == 1 and v[0].is_cuda and v[0].dim() == 0 for v in dct.values())
    assert abs(float(sc["stoi"][0]) - 1) < 1e-5 and float(ref["stoi"][0]) < float(sc["stoi"][0])
    assert float(ref["stoi"][0]) == float(STOI(clean, noisy, sr=16000))


def test_loss_metric_leaves_the_validation_loop_alone(tmp_path, monkeypatch, deterministic_switch):
    from sehip import metric
    from sehip._lib import lib
    solver, _ = make_solver(tmp_path, "loss")

    def refuse(*a, **k):
        raise AssertionError("validation.metric 'loss' must not compute a metric")

    monkeypatch.setattr(metric, "STOI", refuse)
    monkeypatch.setattr(metric, "SI_SDR", refuse)
    solver.score["loss"] = 1.25
    assert solver._run_one_epoch(0, 1, train=False) == 1.25        # 'loss' returns the TRAIN loss, as the reference does
    assert solver.score["stoi"] == [] and solver.score["sisdr"] == []
    assert not lib().sehip_last_kernel().decode().startswith("stoi")


def test_solver_validates_an_stft_domain_model_by_sisdr(tmp_path, deterministic_switch):
    """an STFT-domain model (`unet`): the metric is taken on waveforms, so the Solver keeps the time-domain sources and takes the
    output back through istft_custom"""
    from sehip import SI_SDR
    from sehip.evaluate import istft_custom, stft_custom
    from sehip.solver import ScalarLog
    from sehip.train import main
    from sehip.utils import dict2obj
    cfg = dict2obj({
        "seed": 10, "root": None, "ha": None,
        "model": {"name": "unet", "audio_channels": 1, "num_spk": 1, "sample_rate": 16000, "segment": 1.024, "n_fft": 512, "hop_length": 128,
                  "win_length": 512, "center": True, "unet_channels": 1, "unet_layer": 4, "bilinear": False, "drop_out": 0.5},
        "optim": {"optim": "adam", "lr": 3e-4, "beta1": 0.9, "beta2": 0.999, "loss": "mse", "clip_grad": 5, "pit": False, "load": False},
        "dset": {"name": "synthetic", "norm": None, "sample_rate": 16000},
        "solver": {"epochs": 1, "save_checkpoint_interval": 1000, "all_steps": True, "total_steps": 0, "patience": 0,
                   "root": str(tmp_path), "resume": None, "preloaded_model": None,
                   "validation": {"interval": 1000, "metric": "sisdr", "total_steps": 0}, "test": {"interval": 1000}},
    })
    clean = np.stack([R.am_signal(16384, 16000, seed=40 + i) for i in range(2)]).astype(np.float32)
    noisy = clean + 0.03 * np.random.RandomState(41).randn(2, 16384).astype(np.float32)
    batch = (torch.from_numpy(noisy).reshape(2, 1, 16384), torch.from_numpy(clean).reshape(2, 1, 1, 16384), [None], [None], ["x"], [0])
    solver = main(cfg, return_solver=True, device="gpu", train_dataloader=[batch], validation_dataloader=[batch], writer=ScalarLog())
    assert solver.find_max
    score = solver._run_one_epoch(0, 1, train=False)
    assert isinstance(score, float) and solver.score["sisdr"] == score and np.isfinite(score)
    dev = solver.device
    solver.model.eval()
    with torch.no_grad():
        out = solver.model(stft_custom(batch[0].to(dev), cfg.model))
        direct = float(SI_SDR(batch[1].to(dev).reshape(2, 1, 16384), istft_custom(out.contiguous(), 16384, cfg.model)))
    # the same forward pass twice: if its sums are taken in another order the last bits of the output move, and a ratio of signal
    # energies of a few dB moves by parts in 1e6 -- 1e-3 dB is far above that and far below any wiring mistake
    assert abs(score - direct) < 1e-3, (score, direct)
    assert solver._is_best(score, find_max=True)
