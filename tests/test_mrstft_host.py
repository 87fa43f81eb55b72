"""CPU: the oracle of sehip.loss.mrstft_loss (tests/mrstft_ref.py) against a direct-DFT statement of one small case, its gradient
conventions, and everything of the loss that comes before a launch: the frame count, the refusals of the C ABI, the registry, the
Solver's refusals and the exports.  No GPU call."""
import ctypes

import numpy as np
import pytest
import torch

import mrstft_ref as MR


def direct_magnitudes(x, n_fft, hop, win):
    """numpy float64, nothing shared with torch.stft: reflect padding by n_fft / 2, the periodic hann of win centred in n_fft, one DFT sum
    per frame and bin"""
    n = len(x)
    pad = n_fft // 2
    idx = np.arange(-pad, n + pad)
    idx = np.where(idx < 0, -idx, np.where(idx >= n, 2 * (n - 1) - idx, idx))
    xp = x[idx]
    w = np.zeros(n_fft)
    lp = (n_fft - win) // 2
    w[lp:lp + win] = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(win) / win)
    T = 1 + n // hop
    k = np.arange(n_fft // 2 + 1)[:, None] * np.arange(n_fft)[None, :]
    basis = np.exp(-2j * np.pi * k / n_fft)
    out = np.empty((n_fft // 2 + 1, T))
    for t in range(T):
        s = basis @ (w * xp[t * hop:t * hop + n_fft])
        out[:, t] = np.sqrt(np.maximum(s.real ** 2 + s.imag ** 2, 1e-7))
    return out


def test_restatement_against_a_direct_dft():
    res = ((64, 16, 48), (128, 50, 100))
    r = np.random.RandomState(3)
    src = 0.1 * r.randn(2, 150)
    enh = src + 0.05 * r.randn(2, 150)
    enh[1, 100:] = 0.0                                               # clamped cells
    want = 0.0
    for i, (n_fft, hop, win) in enumerate(res):
        X = np.stack([direct_magnitudes(row, n_fft, hop, win) for row in enh])
        Y = np.stack([direct_magnitudes(row, n_fft, hop, win) for row in src])
        got = MR.magnitudes(torch.from_numpy(enh), n_fft, hop, win).numpy()
        assert got.shape == X.shape == (2, n_fft // 2 + 1, 1 + 150 // hop)
        assert np.abs(got - X).max() <= 1e-12 * X.max()
        sc, mag = np.sqrt(((Y - X) ** 2).sum()) / np.sqrt((Y * Y).sum()), np.abs(np.log(Y) - np.log(X)).mean()
        t = MR.terms(torch.from_numpy(enh), torch.from_numpy(src), res)[i]
        assert abs(float(t[0]) - sc) <= 1e-12 * sc and abs(float(t[1]) - mag) <= 1e-12 * mag
        want += (0.5 * sc + 2.0 * mag) / len(res)
    got = float(MR.loss(torch.from_numpy(enh), torch.from_numpy(src), res, 0.5, 2.0))
    assert abs(got - want) <= 1e-12 * want


def test_conventions_of_the_restatement():
    res = ((64, 16, 64),)
    src = 0.1 * torch.randn(2, 200, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    out = MR.all_grads(src.clone(), src, res)                        # enhanced == sources: sc = 0 with a zero gradient, not NaN
    assert float(out["terms"][0, 0]) == 0.0 and float(out["terms"][0, 1]) == 0.0
    assert not out["g_sc"].any() and not out["g_mag"].any()
    half = src.clone()
    half[:, 50:] = 0.0
    out = MR.all_grads(half * 0.5, half, res)                        # clamped cells pass nothing: finite, and zero past the last frame
    assert torch.isfinite(out["g_full"]).all() and out["g_full"][:, :40].any() and not out["g_full"][:, 120:].any()   # that reads sample 49
    e = half.clone().requires_grad_(True)
    s = src.clone().requires_grad_(True)
    MR.loss(e, s, res).backward()
    assert s.grad is None                                            # the clean signal receives no gradient
    p = torch.tensor([0.0, 1e-7, 2e-7], dtype=torch.float64, requires_grad=True)
    MR.gclamp(p).sum().backward()
    assert p.grad.tolist() == [0, 1, 1]
    z = torch.zeros(3, dtype=torch.float64, requires_grad=True)
    (MR.gsqrt(z).sum() + MR.gabs(z).sum()).backward()
    assert z.grad.tolist() == [0, 0, 0]


def test_frame_count_from_the_library():
    from sehip._lib import lib
    L = lib()
    for n, n_fft, hop in ((4000, 1024, 120), (1025, 2048, 240), (1200, 512, 50), (1300, 128, 128), (1300, 64, 16)):
        assert L.sehip_stft_custom_frames(n, n_fft, hop, 1) == 1 + n // hop == L.sehip_mrl_frames(n, hop)
        assert L.sehip_mrl_blocks(n, hop) == (1 + n // hop + 1) // 2
    assert L.sehip_mrl_frames(4000, 0) == 0 and L.sehip_mrl_blocks(0, 16) == 0


def c_res(res):
    return (ctypes.c_int * max(3 * len(res), 1))(*[v for r in res for v in r])


BAD = (  # (resolutions, n, what the message names)
    (((96, 16, 64),), 4000, b"n_fft=96"),
    (((4096, 16, 64),), 4000, b"n_fft=4096"),
    (((512, 128, 513),), 4000, b"win_length=513"),
    (((512, 257, 256),), 4000, b"hop=257"),
    (((512, 128, 512),), 256, b"n=256"),
    (((512, 0, 512),), 4000, b"hop=0"),
    ((), 4000, b"resolutions=0"),
    (((512, 128, 512),) * 9, 4000, b"resolutions=9"),
)


@pytest.mark.parametrize("res,n,names", BAD)
def test_every_refusal_through_the_c_abi(res, n, names):
    """each entry point reports the error (a status and a message that names the argument) without throwing and before any HIP call"""
    from sehip._lib import lib
    L = lib()
    assert L.sehip_mrl_check(len(res), c_res(res), 1, n) != 0 and names in L.sehip_last_error()
    assert L.sehip_mrl_finalize(None, len(res), c_res(res), 1, n, 1.0, 1.0, None, None, None, None) != 0 and names in L.sehip_last_error()
    if len(res) == 1:
        (n_fft, hop, win), = res
        assert L.sehip_mrl_forward(None, None, 1, n, n_fft, hop, win, None, None, None) != 0 and names in L.sehip_last_error()
        assert L.sehip_mrl_backward(None, None, 1, n, n_fft, hop, win, None, None, None, 1.0, 1.0, None, None) != 0
        assert names in L.sehip_last_error()
        assert L.sehip_mrl_gather(None, 1, n, n_fft, hop, win, 0, None, None) != 0 and names in L.sehip_last_error()
        assert L.sehip_mrl_magnitudes(None, 1, n, n_fft, hop, win, None, None, None) != 0 and names in L.sehip_last_error()


def test_refusals_fire_before_any_launch():
    from sehip import MRSTFTLoss, SehipError, mrstft_loss, mrstft_terms, ops
    from sehip._lib import lib
    from sehip.loss import MRSTFT_RESOLUTIONS, MRSTFTWorkspace
    L = lib()
    ok = c_res(((512, 128, 512),))
    assert L.sehip_mrl_check(1, ok, 1, 257) == 0 and L.sehip_mrl_check(1, ok, 0, 4000) != 0 and b"rows=0" in L.sehip_last_error()
    assert L.sehip_mrl_forward(None, None, 1, 4000, 512, 128, 512, None, None, None) != 0 and b"null pointer" in L.sehip_last_error()
    assert L.sehip_mrl_gather(None, 1, 4000, 512, 128, 512, 2, None, None) != 0 and b"accumulate" in L.sehip_last_error()
    x = torch.zeros(1, 1, 4000)
    for fn in (mrstft_loss, mrstft_terms, MRSTFTLoss()):
        with pytest.raises(SehipError, match="mrstft"):
            fn(x, x)                                                 # CPU tensors: no fallback
    with pytest.raises(SehipError, match="mrstft_loss"):
        mrstft_loss(x.numpy(), x)
    with pytest.raises(SehipError, match="stft_magnitudes"):
        ops.stft_magnitudes(x, 512, 128, 512)
    with pytest.raises(SehipError, match="mrstft_loss.*n=1024"):
        MRSTFTWorkspace(1, 1024, MRSTFT_RESOLUTIONS, "cpu")          # the 2048 resolution needs more than 1024 samples
    with pytest.raises(SehipError, match="mrstft_loss.*n_fft=100"):
        MRSTFTWorkspace(1, 4000, ((100, 10, 100),), "cpu")
    with pytest.raises(SehipError, match="mrstft_loss.*triples"):
        MRSTFTWorkspace(1, 4000, ((512, 128),), "cpu")
    ws = MRSTFTWorkspace(3, 4000, MRSTFT_RESOLUTIONS, "cpu")
    assert ws.blocks == [3 * 17, 3 * 9, 3 * 41] and ws.offsets == [0, 51, 78] and ws.partials.shape == (201, 3)
    assert ws.fgrad.numel() == 3 * max(34 * 600, 17 * 1200, 81 * 240) and ws.terms.shape == (3, 2)
    w = ws.windows[0]
    assert w.shape == (1024,) and not w[:212].any() and not w[812:].any() and float(w[212 + 300]) == 1.0


def test_registry_and_exports():
    import sehip
    from sehip import _lib, distrib, loss
    from sehip.utils import dict2obj
    fn = distrib.get_loss_function(dict2obj({"loss": "mrstft"}))
    assert isinstance(fn, loss.MRSTFTLoss) and fn.wave_l1 == 0.0 and fn.resolutions == loss.MRSTFT_RESOLUTIONS == MR.RESOLUTIONS
    assert (fn.sc_weight, fn.mag_weight) == (1.0, 1.0)
    fn = distrib.get_loss_function(dict2obj({"loss": "l1+mrstft"}))
    assert isinstance(fn, loss.MRSTFTLoss) and fn.wave_l1 == 1.0 and fn.resolutions == loss.MRSTFT_RESOLUTIONS
    fn = distrib.get_loss_function(dict2obj({"loss": "mrstft", "mrstft_resolutions": [[512, 128, 512], [256, 64, 200]]}))
    assert fn.resolutions == ((512, 128, 512), (256, 64, 200))
    for name in ("mrstft_loss", "mrstft_terms", "MRSTFTLoss", "mrstft_loss_workspace"):
        assert getattr(sehip, name) is getattr(loss, name)
    assert callable(sehip.ops.stft_magnitudes)
    L = _lib.lib()
    for name in ("sehip_mrl_frames", "sehip_mrl_blocks", "sehip_mrl_check", "sehip_mrl_forward", "sehip_mrl_finalize", "sehip_mrl_backward",
                 "sehip_mrl_gather", "sehip_mrl_magnitudes"):
        assert name in _lib.declared_symbols() and hasattr(L, name), name


def solver_config(model, loss, pit_apply=False):
    from sehip.utils import dict2obj
    return dict2obj({"model": {"name": model}, "optim": {"loss": loss, "pit_apply": pit_apply}, "dset": {"sample_rate": 16000},
                     "solver": {"epochs": 1}})


@pytest.mark.parametrize("loss", ["mrstft", "l1+mrstft"])
def test_solver_refuses_stft_models_and_pit_apply(loss):
    import re
    from sehip import SehipError
    from sehip.model.types import STFT_MODELS
    from sehip.solver import Solver
    for model in sorted(STFT_MODELS):
        with pytest.raises(SehipError, match=f"(?s)'{re.escape(loss)}'.*'{model}'"):
            Solver(solver_config(model, loss), model=None)
    with pytest.raises(SehipError, match=f"'{re.escape(loss)}'.*pit_apply"):
        Solver(solver_config("conv-tasnet", loss, pit_apply=True), model=None)
