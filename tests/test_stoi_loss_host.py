"""CPU: the oracle of sehip.loss.stoi_loss (tests/stoi_loss_ref.py) against tests/stoi_ref.py -- the value to 1e-12, the gradient against
central differences of stoi_ref.stoi in float64 -- its conventions, and everything of the loss that comes before a launch: the
refusals, the registry, the Solver's refusals and the exports.  No GPU call."""
import numpy as np
import pytest
import torch

import stoi_loss_ref as LR
import stoi_ref as R

CASES = ((10000, 6000), (16000, 9600), (8000, 4800))       # 45 frames at 10 kHz each
_cache = {}


def pair(sr, n):
    """clean am_signal with its middle turned down 80 dB (frames are dropped), estimate = clean + noise at 0 dB"""
    if (sr, n) not in _cache:
        x = R.am_signal(n, sr, seed=1)
        x[int(0.45 * n):int(0.55 * n)] *= 1e-4
        r = np.random.RandomState(101).randn(n)
        _cache[(sr, n)] = (x, x + r * np.sqrt(np.mean(x * x) / np.mean(r * r)))
    return _cache[(sr, n)]


@pytest.mark.parametrize("extended", [False, True])
@pytest.mark.parametrize("sr,n", CASES)
def test_float64_restatement_reproduces_the_value(sr, n, extended):
    x, y = pair(sr, n)
    st = LR.stoi_steps(x, torch.from_numpy(y), sr, extended)
    want = R.stoi_steps(x, y, sr, extended)
    assert np.array_equal(st["src"], want["src"]) and 30 <= st["T"] < R.frame_count(len(want["x10"])) - 1
    assert abs(float(st["d"]) - float(want["d"])) <= 1e-12
    assert np.abs(st["y_tob"].numpy() - want["y_tob"]).max() <= 1e-12 * want["y_tob"].max()


def clip_mask(x, y, sr):
    st = LR.stoi_steps(x, torch.from_numpy(y), sr)
    return st["src"], LR.correlate(st["x_tob"], st["y_tob"], detail=True)[1].numpy()


@pytest.mark.parametrize("extended", [False, True])
@pytest.mark.parametrize("sr,n", CASES)
def test_gradient_matches_central_differences(sr, n, extended):
    """16 randomly chosen samples per case.  Step h = 1e-4 (the estimate's samples are ~0.1): the kept-frame set and the clip branches are
    asserted unchanged at y +- h e_i, so d is smooth along the step.  The central difference D(h) has the truncation error h^2 d''' / 6;
    halving the step measures it, |D(h / 2) - g| ~ |D(h) - D(h / 2)| / 3, taken twice over here.  The rounding of the two values (a
    float64 evaluation of d carries ~1e-14 of absolute noise through its sums) enters as 2e-14 / (h / 2) = 4e-10."""
    h = 1e-4
    x, y = pair(sr, n)
    d, g = LR.stoi_value_and_grad(x, y, sr, extended)
    assert abs(d - R.stoi(x, y, sr, extended)) <= 1e-12
    src0, mask0 = clip_mask(x, y, sr)
    assert mask0.sum() >= 10                                         # the clip branch is exercised
    picks = np.random.RandomState(sr + n).choice(n, 16, replace=False)
    worst = 0.0
    for i in picks:
        cd = []
        for step in (h, h / 2):
            vals = []
            for sign in (1, -1):
                yp = y.copy()
                yp[i] += sign * step
                if step == h and not extended:
                    src, mask = clip_mask(x, yp, sr)
                    assert np.array_equal(src, src0) and np.array_equal(mask, mask0), i
                vals.append(R.stoi(x, yp, sr, extended))
            cd.append((vals[0] - vals[1]) / (2 * step))
        tol = 2 * abs(cd[0] - cd[1]) / 3 + 2e-14 / (h / 2)
        worst = max(worst, abs(g[i] - cd[1]) / tol)
        assert abs(g[i] - cd[1]) <= tol, (i, g[i], cd, tol)
    assert np.abs(g[picks]).max() > 1e-6                             # (the tolerance's floor of 4e-10 is far below the gradient)
    print(f"[stoi_loss] central differences sr {sr} extended {extended}: worst error / tolerance {worst:.3e}")


@pytest.mark.parametrize("extended", [False, True])
def test_conventions(extended):
    x, y = pair(10000, 6000)
    d, g = LR.stoi_value_and_grad(x, np.zeros_like(y), 10000, extended)        # an all-zero estimate: sqrt' (0) = 0
    assert d == 0.0 and np.isfinite(g).all() and not g.any()
    d, g = LR.stoi_value_and_grad(np.zeros_like(x), y, 10000, extended)        # an all-zero clean row
    assert np.isfinite(d) and np.isfinite(g).all()
    d, g = LR.stoi_value_and_grad(np.zeros_like(x), np.zeros_like(y), 10000, extended)
    assert np.isfinite(d) and np.isfinite(g).all()
    short = x.copy()
    short[2000:] *= 1e-4                                                       # fewer than 30 spectra are left
    d, g = LR.stoi_value_and_grad(short, y, 10000, extended)
    assert d == 1e-5 and not g.any()
    # the tie rule: min passes the gradient to its first argument on a tie
    a = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64, requires_grad=True)
    b = torch.tensor([1.0, 1.0, 4.0], dtype=torch.float64, requires_grad=True)
    LR.tmin(a, b).sum().backward()
    assert a.grad.tolist() == [1, 0, 1] and b.grad.tolist() == [0, 1, 0]
    z = torch.zeros(3, dtype=torch.float64, requires_grad=True)
    LR.gsqrt(z).sum().backward()
    assert z.grad.tolist() == [0, 0, 0]


def test_refusals_fire_before_any_launch():
    from sehip import SehipError, StoiLoss, stoi_loss
    from sehip._lib import lib
    from sehip.loss import StoiLossWorkspace, stoi_loss_rows
    x = torch.zeros(1, 1, 8000)
    for fn in (stoi_loss, stoi_loss_rows, StoiLoss()):
        with pytest.raises(SehipError, match="stoi_loss"):
            fn(x, x)                                                 # CPU tensors: no fallback
    with pytest.raises(SehipError, match="stoi_loss"):
        stoi_loss(x.numpy(), x)
    with pytest.raises(SehipError, match="stoi_loss.*255 samples"):
        StoiLossWorkspace(1, 408, 16000, "cpu")
    with pytest.raises(SehipError, match="stoi_loss.*16001"):
        StoiLossWorkspace(1, 8000, 16001, "cpu")                    # 10000 / 16001: p, q outside 128 / 1024
    with pytest.raises(SehipError, match="stoi_loss"):
        StoiLossWorkspace(1, 8000, 0, "cpu")
    with pytest.raises(SehipError, match="stoi_loss.*rows"):
        StoiLossWorkspace(40000, 8000, 16000, "cpu")
    ws = StoiLossWorkspace(3, 9600, 16000, "cpu")
    assert (ws.n10, ws.frames) == (6000, 45) and ws.seg.numel() == 3 * 15 * 450 and ws.fgrad.shape == (3, 44, 256) and ws.g10.shape == (3, 6000)
    # the C ABI validates before any HIP call
    L = lib()
    assert L.sehip_stoil_segment_floats(2, 45) == 2 * 15 * 450 and L.sehip_stoil_segment_floats(2, 20) == 2 * 450
    assert L.sehip_stoil_segment_floats(0, 45) == -1
    assert L.sehip_stoil_segments(None, None, 1, 45, 0, None, 0, 1.0, None, None, None) != 0 and b"null pointer" in L.sehip_last_error()
    assert L.sehip_stoil_segments(None, None, 1, 45, 2, None, 0, 1.0, None, None, None) != 0 and b"extended" in L.sehip_last_error()
    assert L.sehip_stoil_segments(None, None, 1, 45, 0, None, 3, 1.0, None, None, None) != 0 and b"gstride" in L.sehip_last_error()
    assert L.sehip_stoil_bands(None, 1, 255, None, None, None, None, None, None) != 0 and b"len=255" in L.sehip_last_error()
    assert L.sehip_stoil_compact(None, None, None, 0, 6000, None, None, None) != 0 and b"rows=0" in L.sehip_last_error()
    assert L.sehip_stoil_resample_adj(None, 1, 8000, None, 5, 5, 290, None, None) != 0 and b"1 / 1" in L.sehip_last_error()
    assert L.sehip_stoil_resample_adj(None, 1, 8000, None, 200, 3, 290, None, None) != 0 and b"ratio" in L.sehip_last_error()


def test_registry_and_exports():
    import sehip
    from sehip import _lib, distrib, loss
    from sehip.utils import dict2obj
    for name, ext in (("stoi", False), ("estoi", True)):
        fn = distrib.get_loss_function(dict2obj({"loss": name}))
        assert isinstance(fn, loss.StoiLoss) and fn.extended == ext and fn.sr == 16000
    assert sehip.stoi_loss is loss.stoi_loss and sehip.stoi_loss_rows is loss.stoi_loss_rows and sehip.StoiLoss is loss.StoiLoss
    L = _lib.lib()
    for name in ("sehip_stoil_segment_floats", "sehip_stoil_segments", "sehip_stoil_bands", "sehip_stoil_compact", "sehip_stoil_resample_adj"):
        assert name in _lib.declared_symbols() and hasattr(L, name), name


def solver_config(model, loss, pit_apply=False):
    from sehip.utils import dict2obj
    return dict2obj({"model": {"name": model}, "optim": {"loss": loss, "pit_apply": pit_apply}, "dset": {"sample_rate": 16000},
                     "solver": {"epochs": 1}})


@pytest.mark.parametrize("loss", ["stoi", "estoi"])
def test_solver_refuses_stft_models_and_pit_apply(loss):
    from sehip import SehipError
    from sehip.model.types import STFT_MODELS
    from sehip.solver import Solver
    for model in sorted(STFT_MODELS):
        with pytest.raises(SehipError, match=f"(?s)'{loss}'.*'{model}'"):
            Solver(solver_config(model, loss), model=None)
    with pytest.raises(SehipError, match=f"'{loss}'.*pit_apply"):
        Solver(solver_config("conv-tasnet", loss, pit_apply=True), model=None)
