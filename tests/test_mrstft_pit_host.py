"""CPU: the oracle of sehip.loss.pit_mrstft_loss (tests/mrstft_pit_ref.py) against a brute force over mrstft_ref.loss on speaker slices,
its invariance under a permutation of the targets' speakers, and everything of the loss that comes before a launch: the declared and
exported symbols, the refusals, the registry and the Solver's refusals.  No GPU call."""
import ctypes
from itertools import permutations

import pytest
import torch

import mrstft_pit_ref as PR
import mrstft_ref as MR

RES = ((64, 16, 48), (128, 50, 100))


def small(B=2, S=3, C=2, n=300, seed=4):
    g = torch.Generator().manual_seed(seed)
    tgt = 0.1 * torch.randn(B, S, C, n, generator=g, dtype=torch.float64) * (1 + torch.arange(S, dtype=torch.float64)).reshape(1, S, 1, 1)
    enh = tgt[:, [2, 0, 1][:S]] + 0.02 * torch.randn(B, S, C, n, generator=g, dtype=torch.float64)
    return enh, tgt


@pytest.mark.parametrize("wave_l1", [0.0, 0.5])
def test_restatement_against_a_brute_force_over_slices(wave_l1):
    """S * S calls of the plain oracle on (enhance[:, i], target[:, j]), the reference's walk written out, autograd through the chosen sum"""
    enh, tgt = small()
    S, n = enh.shape[1], enh.shape[-1]
    e = enh.clone().requires_grad_(True)

    def pair(i, j):
        x, y = e[:, i].reshape(-1, n), tgt[:, j].reshape(-1, n)
        return MR.loss(x, y, RES, 0.5, 2.0) + wave_l1 * (x - y).abs().mean()
    m = [[pair(i, j) for j in range(S)] for i in range(S)]
    best, lmin = None, 1e9
    for pe in permutations(range(S)):
        l = sum(float(m[pe[j]][j].detach()) for j in range(S))
        if lmin > l:
            best, lmin = list(pe), l
    want = sum(m[best[j]][j] for j in range(S)) / S
    want_grad, = torch.autograd.grad(want, e)
    assert best == [1, 2, 0]                                          # enhance[:, i] is target[:, (2, 0, 1)[i]]

    e2 = enh.clone().requires_grad_(True)
    terms = PR.pair_terms(e2, tgt, RES)
    got_m = PR.pair_matrix(terms, PR.wave_l1_pairs(e2, tgt), 0.5, 2.0, wave_l1)
    assert terms.shape == (len(RES), S, S, 2)
    for i in range(S):
        for j in range(S):
            assert abs(float(got_m[i, j]) - float(m[i][j])) <= 1e-12 * float(m[i][j])
            t = MR.terms(enh[:, i].reshape(-1, n), tgt[:, j].reshape(-1, n), RES)
            assert torch.allclose(terms[:, i, j], t, rtol=1e-12, atol=0)
    assert PR.walk(got_m)[0] == best
    got = PR.loss(e2, tgt, RES, 0.5, 2.0, wave_l1)
    got_grad, = torch.autograd.grad(got, e2)
    assert abs(float(got) - float(want)) <= 1e-12 * float(want)
    assert float((got_grad - want_grad).norm()) <= 1e-10 * float(want_grad.norm())
    e3 = enh.clone().requires_grad_(True)
    t3 = tgt.clone().requires_grad_(True)
    PR.loss(e3, t3, RES, 1.0, 1.0, wave_l1).backward()
    assert t3.grad is None and bool(e3.grad.any())                   # the target receives no gradient
    out = PR.all_grads(enh, tgt, RES, wave_l1)
    assert out["perm_full"] == best and out["g_full"].shape == enh.shape and out["gap_full"] > 1.0


def test_loss_is_unchanged_when_the_targets_speakers_are_permuted():
    enh, tgt = small()
    base = float(PR.loss(enh, tgt, RES, 1.0, 1.0, 0.25))
    perm0 = PR.walk(PR.pair_matrix(PR.pair_terms(enh, tgt, RES), PR.wave_l1_pairs(enh, tgt), 1.0, 1.0, 0.25))[0]
    for order in permutations(range(3)):
        t2 = tgt[:, list(order)]
        assert abs(float(PR.loss(enh, t2, RES, 1.0, 1.0, 0.25)) - base) <= 1e-13 * base
        m = PR.pair_matrix(PR.pair_terms(enh, t2, RES), PR.wave_l1_pairs(enh, t2), 1.0, 1.0, 0.25)
        assert PR.walk(m)[0] == [perm0[order[j]] for j in range(3)]  # the estimate follows its target to the new place


def test_walk_takes_the_first_minimum_in_itertools_order():
    assert PR.walk(torch.ones(3, 3))[0] == [0, 1, 2]                 # every permutation ties: the first one stays
    m = torch.tensor([[5.0, 1.0], [1.0, 5.0]])
    assert PR.walk(m)[0] == [1, 0] and PR.gap(m) == pytest.approx(4.0)
    assert PR.walk(torch.ones(1, 1))[0] == [0] and PR.gap(torch.ones(1, 1)) == float("inf")


def test_planted_inputs_have_the_planted_answer():
    enh, tgt, perm = PR.planted(1, 3, 2, 1025)
    assert enh.shape == tgt.shape == (1, 3, 2, 1025) and enh.dtype == tgt.dtype == torch.float32 and perm == [2, 0, 1]
    assert float((enh[:, 0] - tgt[:, 1]).abs().max()) < 0.06 < float((enh[:, 0] - tgt[:, 0]).abs().max())
    again = PR.planted(1, 3, 2, 1025)
    assert torch.equal(again[0], enh) and torch.equal(again[1], tgt)


def test_symbols_are_declared_and_exported():
    import sehip
    from sehip import _lib, loss
    L = _lib.lib()
    for name in ("sehip_mrl_pair_blocks", "sehip_mrl_pair_forward", "sehip_mrl_pair_select", "sehip_mrl_pair_backward"):
        assert name in _lib.declared_symbols() and hasattr(L, name), name
    for name in ("pit_mrstft_loss", "pit_mrstft_terms", "PitMRSTFTLoss", "pit_mrstft_workspace"):
        assert getattr(sehip, name) is getattr(loss, name)
    # the partials' size: (2 S S + S) sums per workgroup, B C workgroups per frame pair
    assert L.sehip_mrl_pair_blocks(3, 6, 1, 1300, 240) == (2 * 36 + 6) * 3 * L.sehip_mrl_blocks(1300, 240) == 78 * 3 * 3
    assert L.sehip_mrl_pair_blocks(2, 2, 1, 4000, 50) == 10 * 2 * 41
    assert L.sehip_mrl_pair_blocks(2, 7, 1, 4000, 50) == 0 and L.sehip_mrl_pair_blocks(2, 0, 1, 4000, 50) == 0
    assert L.sehip_mrl_pair_blocks(0, 2, 1, 4000, 50) == 0 and L.sehip_mrl_pair_blocks(2, 2, 1, 4000, 0) == 0
    assert L.sehip_mrl_pair_blocks(65536, 2, 1, 4000, 50) == 0


def c_res(res):
    return (ctypes.c_int * max(3 * len(res), 1))(*[v for r in res for v in r])


def test_every_refusal_through_the_c_abi():
    """each entry point reports the error (a status and a message that names the argument) without throwing and before any HIP call"""
    from sehip._lib import lib
    L = lib()
    fwd = lambda B, S, C, n, nf, hop, win: L.sehip_mrl_pair_forward(None, None, B, S, C, n, nf, hop, win, None, None, None)
    bwd = lambda B, S, C, n, nf, hop, win: L.sehip_mrl_pair_backward(None, None, B, S, C, n, nf, hop, win, None, None, None, None, 1.0, 1.0,
                                                                     None, None)
    sel = lambda res, B, S, C, n: L.sehip_mrl_pair_select(None, len(res), c_res(res), B, S, C, n, 1.0, 1.0, None, 0.0, None, None, None,
                                                          None, None, None)
    for fn in (fwd, bwd):
        for args, names in (((2, 7, 1, 4000, 512, 128, 512), b"S=7"), ((2, 0, 1, 4000, 512, 128, 512), b"S=0"),
                            ((0, 2, 1, 4000, 512, 128, 512), b"rows=0"), ((65535, 2, 2, 4000, 512, 128, 512), b"rows=131070"),
                            ((2, 2, 1, 4000, 96, 16, 64), b"n_fft=96"), ((2, 2, 1, 4000, 4096, 16, 64), b"n_fft=4096"),
                            ((2, 2, 1, 4000, 512, 128, 513), b"win_length=513"), ((2, 2, 1, 4000, 512, 257, 256), b"hop=257"),
                            ((2, 2, 1, 256, 512, 128, 512), b"n=256"), ((2, 2, 1, 4000, 512, 0, 512), b"hop=0"),
                            ((2, 2, 1, 4000, 512, 128, 512), b"null pointer")):
            assert fn(*args) != 0 and names in L.sehip_last_error(), (args, L.sehip_last_error())
    ok = ((512, 128, 512),)
    for args, names in (((ok, 2, 7, 1, 4000), b"S=7"), ((ok, 0, 2, 1, 4000), b"rows=0"), (((), 2, 2, 1, 4000), b"resolutions=0"),
                        ((ok * 9, 2, 2, 1, 4000), b"resolutions=9"), ((ok, 2, 2, 1, 256), b"n=256"), ((ok, 2, 2, 1, 4000), b"null pointer")):
        assert sel(*args) != 0 and names in L.sehip_last_error(), (args, L.sehip_last_error())


def test_refusals_fire_before_any_allocation_or_launch():
    from sehip import PitMRSTFTLoss, SehipError, pit_mrstft_loss, pit_mrstft_terms, pit_mrstft_workspace
    from sehip.loss import MRSTFT_RESOLUTIONS, PitMRSTFTWorkspace, _pit_mrstft_check
    x = torch.zeros(2, 2, 1, 4000)
    for fn in (pit_mrstft_loss, pit_mrstft_terms, PitMRSTFTLoss()):
        with pytest.raises(SehipError, match="pit_mrstft"):
            fn(x, x)                                                 # CPU tensors: no fallback
    with pytest.raises(SehipError, match="pit_mrstft_loss"):
        pit_mrstft_loss(x.numpy(), x)
    # the shape refusals, with the device check stood down for host tensors: whatever passes here has allocated and launched nothing
    import sehip._lib as _lib
    real = _lib.require_gpu
    _lib.require_gpu = lambda t, what: None
    try:
        with pytest.raises(ValueError, match="pit_mrstft_loss.*shapes differ"):
            _pit_mrstft_check(x, x[..., :3000])
        with pytest.raises(SehipError, match="pit_mrstft_loss.*batch, speakers"):
            _pit_mrstft_check(x[0, 0], x[0, 0])                      # [1, 4000]: fewer than 3 axes
        with pytest.raises(SehipError, match="S=7"):
            _pit_mrstft_check(torch.zeros(1, 7, 1, 4000), torch.zeros(1, 7, 1, 4000))
        with pytest.raises(SehipError, match="empty"):
            _pit_mrstft_check(torch.zeros(0, 2, 1, 4000), torch.zeros(0, 2, 1, 4000))
        _pit_mrstft_check(x, x)
    finally:
        _lib.require_gpu = real
    with pytest.raises(SehipError, match="pit_mrstft_loss.*n=1024"):
        PitMRSTFTWorkspace((2, 2, 1, 1024), MRSTFT_RESOLUTIONS, "cpu")     # the 2048 resolution needs more than 1024 samples
    with pytest.raises(SehipError, match="pit_mrstft_loss.*n_fft=100"):
        PitMRSTFTWorkspace((2, 2, 1, 4000), ((100, 10, 100),), "cpu")
    with pytest.raises(SehipError, match="pit_mrstft_loss.*triples"):
        PitMRSTFTWorkspace((2, 2, 1, 4000), ((512, 128),), "cpu")
    with pytest.raises(SehipError, match="rows=70000"):
        PitMRSTFTWorkspace((35000, 2, 2, 4000), MRSTFT_RESOLUTIONS, "cpu")  # mrl_check on B C rows, before the buffers
    with pytest.raises(SehipError, match="S=7"):
        PitMRSTFTWorkspace((2, 7, 1, 4000), MRSTFT_RESOLUTIONS, "cpu")
    with pytest.raises(SehipError, match="batch, speakers"):
        pit_mrstft_workspace((2, 4000), MRSTFT_RESOLUTIONS, "cpu")
    ws = PitMRSTFTWorkspace((3, 2, 2, 4000), MRSTFT_RESOLUTIONS, "cpu")
    assert ws.view == (3, 2, 2, 4000) and ws.floats == [10 * 6 * 17, 10 * 6 * 9, 10 * 6 * 41] and ws.offsets == [0, 1020, 1560]
    assert ws.partials.shape == (4020,) and ws.terms.shape == (3, 2, 2, 2) and ws.matrix.shape == (2, 2) and ws.stats.shape == (3, 2, 2)
    assert ws.perm.shape == (2,) and ws.perm.dtype == torch.int32 and ws.loss.shape == ()
    assert ws.fgrad.numel() == 12 * max(34 * 600, 17 * 1200, 81 * 240) and ws.generation == 0 and ws.nbytes() > 4 * ws.fgrad.numel()


def test_registry():
    from sehip import distrib, loss
    from sehip.utils import dict2obj
    fn = distrib.get_loss_function(dict2obj({"loss": "pit-mrstft"}))
    assert isinstance(fn, loss.PitMRSTFTLoss) and fn.wave_l1 == 0.0 and fn.resolutions == loss.MRSTFT_RESOLUTIONS == MR.RESOLUTIONS
    assert (fn.sc_weight, fn.mag_weight) == (1.0, 1.0) and callable(fn.workspace)
    fn = distrib.get_loss_function(dict2obj({"loss": "pit-l1+mrstft"}))
    assert isinstance(fn, loss.PitMRSTFTLoss) and fn.wave_l1 == 1.0 and fn.resolutions == loss.MRSTFT_RESOLUTIONS
    fn = distrib.get_loss_function(dict2obj({"loss": "pit-l1+mrstft", "mrstft_resolutions": [[512, 128, 512], [256, 64, 200]]}))
    assert fn.resolutions == ((512, 128, 512), (256, 64, 200)) and fn.wave_l1 == 1.0
    assert not isinstance(distrib.get_loss_function(dict2obj({"loss": "l1+mrstft"})), loss.PitMRSTFTLoss)   # the plain names stay plain


def solver_config(model, loss, pit_apply=False):
    from sehip.utils import dict2obj
    return dict2obj({"model": {"name": model}, "optim": {"loss": loss, "pit_apply": pit_apply}, "dset": {"sample_rate": 16000},
                     "solver": {"epochs": 1}})


@pytest.mark.parametrize("loss", ["pit-mrstft", "pit-l1+mrstft"])
def test_solver_refuses_the_three_bad_combinations(loss):
    """from the configuration alone (model=None: nothing is built, no device is touched)"""
    import re
    from sehip import SehipError
    from sehip.model.types import MULTI_SPEECH_SEPERATION_MODELS, STFT_MODELS
    from sehip.solver import Solver
    for model in sorted(STFT_MODELS):                                # spectra, not waveforms ('rnn-stft-mask' separates, but in the STFT domain)
        with pytest.raises(SehipError, match=f"(?s)'{re.escape(loss)}'.*'{model}'.*spectra"):
            Solver(solver_config(model, loss), model=None)
    for model in ("dccrn", "wav-unet"):                              # waveforms, but one speaker
        assert model not in MULTI_SPEECH_SEPERATION_MODELS
        with pytest.raises(SehipError, match=f"(?s)'{re.escape(loss)}'.*'{model}'.*speakers"):
            Solver(solver_config(model, loss), model=None)
    for model in ("conv-tasnet", "demucs"):                          # PIT twice
        with pytest.raises(SehipError, match=f"'{re.escape(loss)}'.*permutation-invariant by itself.*pit_apply"):
            Solver(solver_config(model, loss, pit_apply=True), model=None)


@pytest.mark.parametrize("loss", ["mrstft", "l1+mrstft"])
def test_the_plain_names_with_pit_apply_point_to_the_new_ones(loss):
    import re
    from sehip import SehipError
    from sehip.solver import Solver
    with pytest.raises(SehipError, match=f"'{re.escape(loss)}'.*pit_apply.*'pit-mrstft' / 'pit-l1\\+mrstft'"):
        Solver(solver_config("conv-tasnet", loss, pit_apply=True), model=None)
