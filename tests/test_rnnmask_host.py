"""CPU: rnn-stft-mask (sehip.model.RNNBaseSTFTMask) -- registry, schema, rejections, the plan's host arithmetic, the dropout generator's
twin, and the fp32 restatement tests/rnnmask_ref.py pinned against vectors of the imported reference (tests/golden/rnnmask_*.npz).

Tolerances of the restatement: 5e-5 relative for activations, outputs and gradients and 1e-5 for the running statistics, the values
tests/test_oracle_golden.py uses for its oracles (activations / est 5e-5, statistics 1e-5)."""
import numpy as np
import pytest
import torch

import rnnmask_ref as R
from util import rel_err

TAGS = sorted(R.FIXTURES)
ACT_TOL, STAT_TOL = 5e-5, 1e-5
_FX = {}


def fixture(tag):
    if tag not in _FX:
        _FX[tag] = R.load_fixture(tag)
    return _FX[tag]


def kw(tag):
    return dict(R.FIXTURES[tag]["kw"])


def test_registry_returns_rnnmask():
    from sehip import SehipError, distrib, utils
    from sehip.model import RNNBaseSTFTMask
    for tag in TAGS:
        m = distrib.get_model(utils.dict2obj(dict(name="rnn-stft-mask", **kw(tag))))
        assert isinstance(m, RNNBaseSTFTMask) and m.cfg.rnn_type == kw(tag)["rnn_type"]
    assert distrib.MODEL_REGISTRY["rnn-stft-mask"] is RNNBaseSTFTMask
    with pytest.raises(SehipError, match="has no HIP path yet"):        # the bare name is the constructor's default, the Elman cell
        distrib.get_model(utils.dict2obj({"name": "rnn-stft-mask"}))
    with pytest.raises(SehipError, match="has no HIP path yet"):
        RNNBaseSTFTMask(rnn_type="rnn")


@pytest.mark.parametrize("tag", TAGS)
def test_schema_and_optimizer(tag):
    from sehip import distrib, utils
    from sehip.model import RNNBaseSTFTMask
    from sehip.optim import FlatOptimizer
    fx = fixture(tag)
    m = RNNBaseSTFTMask(**kw(tag))
    sd = m.state_dict()
    assert list(sd) == list(fx["sd"]) and all(tuple(sd[k].shape) == tuple(v.shape) and sd[k].dtype == v.dtype for k, v in fx["sd"].items())
    names = R.param_names(fx["sd"])
    assert [n for n, _ in m.named_parameters()] == names
    m.load_state_dict(fx["adam"], strict=True)
    back = m.state_dict()
    assert all(torch.equal(back[k], fx["adam"][k]) for k in back)
    m.load_state_dict(fx["sd"], strict=True)
    assert float(m.flat_params.abs().sum()) == pytest.approx(sum(float(fx["sd"][k].abs().sum()) for k in names), rel=1e-5)
    opt = distrib.get_optimizer(utils.dict2obj({"optim": "adam", "lr": 3e-4, "beta1": 0.9, "beta2": 0.999}), m)
    assert isinstance(opt, FlatOptimizer) and len(opt.state_dict()["state"]) == len(names)
    assert m.set_deterministic(True) is m


def test_initialisation_and_seed():
    from sehip.model import RNNBaseSTFTMask
    torch.manual_seed(3)
    a = RNNBaseSTFTMask(rnn_type="lstm", rnn_hidden=256, rnn_layer=2, bidirectional=True)
    torch.manual_seed(3)
    b = RNNBaseSTFTMask(rnn_type="lstm", rnn_hidden=256, rnn_layer=2, bidirectional=True)
    assert a.dropout_seed == b.dropout_seed and torch.equal(a.flat_params, b.flat_params)
    sd = a.state_dict()
    w = sd["rnn.weight_hh_l1_reverse"]
    assert tuple(w.shape) == (1024, 256) and tuple(sd["rnn.weight_ih_l0"].shape) == (1024, 257) and tuple(sd["rnn.weight_ih_l1"].shape) == (1024, 512)
    assert float(w.abs().max()) <= 1 / 16 and float(w.std()) == pytest.approx(1 / 16 / 3 ** 0.5, rel=0.05)
    fc = sd["fc_layers.0.weight"]
    bound = 1 / 512 ** 0.5
    assert tuple(fc.shape) == (514, 512) and float(fc.abs().max()) <= bound and float(fc.std()) == pytest.approx(bound / 3 ** 0.5, rel=0.05)
    assert float(sd["fc_layers.0.bias"].abs().max()) <= bound and float(sd["fc_layers.0.bias"].std()) > 0
    assert bool((sd["batchnorm.weight"] == 1).all()) and bool((sd["batchnorm.bias"] == 0).all())
    assert bool((sd["batchnorm.running_var"] == 1).all()) and int(sd["batchnorm.num_batches_tracked"]) == 0
    # the shipped configuration
    m = RNNBaseSTFTMask(rnn_type="lstm", rnn_hidden=896, rnn_layer=3, bidirectional=True, drop_out=0.5, num_spk=2, audio_channels=2)
    want = 2 * (4 * 896 * 257 + 4 * 896 * 896) + 2 * 2 * (4 * 896 * 1792 + 4 * 896 * 896) + 2 * 1792 + 514 * 1792 + 514
    assert sum(p.numel() for p in m.parameters()) == want


@pytest.mark.parametrize("arg, value", [("rnn_type", "rnn"), ("rnn_type", "elman"), ("rnn_layer", 0), ("rnn_layer", 9), ("rnn_hidden", 48),
                                        ("rnn_hidden", 1056), ("rnn_hidden", 0), ("bidirectional", 1), ("num_spk", 0), ("num_spk", 7),
                                        ("n_fft", 63), ("n_fft", 0), ("drop_out", -0.1), ("drop_out", 1.5), ("activation", "tanh"),
                                        ("audio_channels", 0)])
def test_constructor_rejections(arg, value):
    from sehip import SehipError
    from sehip.model import RNNBaseSTFTMask
    args = dict(rnn_type="lstm")
    args[arg] = value
    with pytest.raises(SehipError, match=arg):
        RNNBaseSTFTMask(**args)


def test_accepted_scope_and_cpu_tensor():
    from sehip import SehipError
    from sehip.model import RNNBaseSTFTMask
    for h in (32, 256, 896, 1024):
        RNNBaseSTFTMask(rnn_type="gru", rnn_hidden=h, rnn_layer=1)
    RNNBaseSTFTMask(rnn_type="lstm", rnn_layer=8, rnn_hidden=32, num_spk=6, n_fft=30, drop_out=1.0, bidirectional=True)
    m = RNNBaseSTFTMask(**kw("rnnmask_gru_uni"))
    with pytest.raises(SehipError, match="CPU tensor"):
        m(torch.zeros(2, 1, 33, 17, 2))
    with pytest.raises(SehipError, match="expected"):
        m(torch.zeros(2, 2, 33, 17, 2))
    with pytest.raises(SehipError, match="expected"):
        m(torch.zeros(2, 1, 32, 17, 2))


# ---- the restatement against the reference's vectors ------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_restatement_reproduces_reference(tag):
    fx = fixture(tag)
    names = R.param_names(fx["sd"])
    p = {k: (v.clone().requires_grad_(True) if k in names else v.clone()) for k, v in fx["sd"].items()}
    taps, run = {}, {}
    est = R.rnnmask_forward(p, fx["input"], taps=taps, running=run, **kw(tag))
    assert rel_err(est.detach(), fx["est"]) < ACT_TOL
    assert set(taps) == set(fx["tap"])
    for k, v in fx["tap"].items():
        assert rel_err(taps[k].detach(), v) < ACT_TOL, k
    for k, v in fx["run"].items():
        assert rel_err(run[k].float(), v.float()) < STAT_TOL, k
    (est * fx["G"]).sum().backward()
    for k in names:
        assert rel_err(p[k].grad, fx["gradG"][k]) < ACT_TOL, k
        p[k].grad = None
    loss = torch.nn.functional.mse_loss(R.rnnmask_forward(p, fx["input"], **kw(tag)), fx["target"])
    assert abs(float(loss) - float(fx["loss"])) < 1e-5 * float(fx["loss"])
    loss.backward()
    for k in names:
        assert rel_err(p[k].grad, fx["grad"][k]) < ACT_TOL, k
    q = dict(fx["sd"])
    q.update(run)
    with torch.no_grad():
        assert rel_err(R.rnnmask_forward(q, fx["input"], training=False, **kw(tag)), fx["est_eval"]) < ACT_TOL


def test_restatement_in_float64_and_with_masks():
    tag = "rnnmask_lstm_bi"
    fx = fixture(tag)
    p64 = {k: (v.double() if v.is_floating_point() else v) for k, v in fx["sd"].items()}
    est = R.rnnmask_forward(p64, fx["input"].double(), **kw(tag))
    assert est.dtype == torch.float64 and rel_err(est, fx["est"]) < ACT_TOL
    ones = [torch.ones(6, 21, 64)]
    assert torch.equal(R.rnnmask_forward(fx["sd"], fx["input"], drop_masks=ones, **kw(tag)), R.rnnmask_forward(fx["sd"], fx["input"], **kw(tag)))
    half = [R.device_mask(11, 0, 0, 6, 21, 64, 0.5)]
    dropped = R.rnnmask_forward(fx["sd"], fx["input"], drop_masks=half, **kw(tag))
    assert rel_err(dropped, fx["est"]) > 1e-2
    assert torch.equal(R.rnnmask_forward(fx["sd"], fx["input"], drop_masks=half, training=False, **kw(tag)),
                       R.rnnmask_forward(fx["sd"], fx["input"], training=False, **kw(tag)))          # eval: no dropout
    sim = R.rnnmask_forward(fx["sd"], fx["input"], sim=R.Bf16Sim, **kw(tag))
    assert 1e-4 < rel_err(sim, fx["est"]) < 5e-2


# ---- the dropout generator's twin ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.25, 0.5])
@pytest.mark.parametrize("seed", [1, 0x1234567890ABCDEF, 2 ** 62 - 5])
def test_dropout_twin_statistics(p, seed):
    n = 2 ** 16
    k0 = R.dropout_keep(seed, 0, 0, n, p)
    bound = 4 * (p * (1 - p) / n) ** 0.5
    assert abs(k0.mean() - (1 - p)) < bound, (k0.mean(), bound)
    k1 = R.dropout_keep(seed, 1, 0, n, p)
    assert abs(k1.mean() - (1 - p)) < bound
    # consecutive counters (and layers) differ like independent draws: agreement p^2 + (1 - p)^2, far from 1
    agree = (k0 == k1).mean()
    assert abs(agree - (p * p + (1 - p) ** 2)) < 0.02
    assert abs((k0 == R.dropout_keep(seed, 0, 1, n, p)).mean() - (p * p + (1 - p) ** 2)) < 0.02
    assert np.array_equal(k0, R.dropout_keep(seed, 0, 0, n, p))
    assert np.array_equal(R.dropout_bits(seed, 0, 0, n), R.dropout_bits(seed, 2 ** 32, 0, n))       # the counter's low word is what counts
    assert R.dropout_keep(seed, 0, 0, n, 0.0).all() and not R.dropout_keep(seed, 0, 0, n, 1.0).any()


def test_dropout_twin_equals_the_plans():
    from sehip import plan_rnnmask as P
    for seed, ctr, layer in ((1, 0, 0), (0xFEDCBA9876543210, 7, 2), (2 ** 62 - 5, 2 ** 32 + 3, 6)):
        for p in (0.0, 0.25, 0.5, 1.0):
            assert np.array_equal(P.drop_keep_mask(seed, ctr, layer, 4096, p), R.dropout_keep(seed, ctr, layer, 4096, p))
    assert P.drop_threshold(0.5) == (1 << 23, 2.0) and P.drop_threshold(1.0) == (1 << 24, 0.0) and P.drop_threshold(0.0) == (0, 1.0)
    m = R.device_mask(5, 0, 0, 3, 4, 8, 0.5)
    assert tuple(m.shape) == (3, 4, 8) and set(m.unique().tolist()) <= {0.0, 2.0}
    keep = R.dropout_keep(5, 0, 0, 96, 0.5).reshape(4, 3, 8)           # the device's order: [rows N][steps L][Hout]
    assert bool(keep[2, 1, 5]) == bool(m[1, 2, 5] > 0)


# ---- the plan's host arithmetic -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_plan_arithmetic_fixtures(tag):
    from sehip import plan_rnnmask as P
    cfg = P.RnnMaskConfig(**kw(tag))
    st = P.RnnMaskStatic(cfg)
    B, C, F, T, _ = R.FIXTURES[tag]["shape"]
    assert (cfg.F, cfg.Fp) == (33, 40) and cfg.SF == cfg.num_spk * 33 and cfg.SFp == {1: 40, 2: 72}[cfg.num_spk]
    shapes = st.buffer_shapes(B, T)
    L, rows = B * C, T * B * C
    assert shapes["feat"][0] == (rows, 40) and shapes["mask"][0] == (rows, cfg.SFp) and shapes["out"][0] == (B, cfg.num_spk, C, 33, T, 2)
    assert shapes["pre0"][0] == (rows, cfg.D, cfg.G, cfg.H) and shapes["gates1"][0] == (rows, cfg.D, 4, cfg.H) and shapes["dG0"] == ((rows, cfg.D, 4, cfg.H), "bf16")
    assert "hd0" in shapes and "hd1" not in shapes and "dx1" in shapes and "dx0" not in shapes
    assert st.step_launches(L) == (2 * L, 2 * L)
    packs = st.pack_launches()
    assert len(packs) == cfg.D * (3 + 4) + 2                           # layer 0 needs no transposed W_ih: the input has no gradient
    offs = sorted((off, (K if tr else N) * ld) for _, _, N, K, tr, ld, off in packs if not (tr and ld == cfg.D * 4 * cfg.H))
    assert all(o % 8 == 0 for o, _ in offs) and all(a + n <= b for (a, n), (b, _) in zip(offs, offs[1:])) and offs[-1][0] + offs[-1][1] <= st.n_wpack
    n_par = sum(int(np.prod(s)) for _, s, kind in cfg.param_specs() if kind == "param")
    assert n_par == {"rnnmask_lstm_bi": 45634, "rnnmask_gru_uni": 45473}[tag]


def test_plan_arithmetic_shipped():
    from sehip import plan_rnnmask as P
    cfg = P.RnnMaskConfig(rnn_type="lstm", rnn_hidden=896, rnn_layer=3, bidirectional=True, drop_out=0.5, num_spk=2, audio_channels=2, n_fft=512,
                          hop_length=128)
    st = P.RnnMaskStatic(cfg)
    assert (cfg.F, cfg.Fp, cfg.SF, cfg.SFp, cfg.Hout) == (257, 264, 514, 520, 1792)
    shapes = st.buffer_shapes(16, 501)                                   # batch 16, stereo, 4-s clips at hop 128
    assert shapes["feat"][0] == (501 * 32, 264) and shapes["pre2"][0] == (501 * 32, 2, 4, 896) and shapes["carry"][0] == (2, 501, 896)
    assert st.step_launches(32) == (96, 96)
    assert st.w[(0, "hh")] - st.w[(0, "ihT")] == 264 * 2 * 4 * 896 and st.w["fcT"] - st.w["fc"] == 514 * 1792
    assert st.n_wpack == st.w["fcT"] + 1792 * 520


def test_static_plan_is_keyed_on_everything_it_holds():
    """models that differ only in drop_out or audio_channels must not share a cached plan: the workspace reads both from it"""
    from sehip.model import RNNBaseSTFTMask
    base = dict(rnn_type="lstm", rnn_hidden=32, rnn_layer=2, n_fft=64)
    a, b = RNNBaseSTFTMask(drop_out=0.0, **base), RNNBaseSTFTMask(drop_out=0.5, **base)
    c, d = RNNBaseSTFTMask(drop_out=0.5, audio_channels=1, **base), RNNBaseSTFTMask(drop_out=0.5, **base)
    assert a.static is not b.static and b.static is not c.static and b.static is d.static
    assert (a.static.cfg.drop_out, b.static.cfg.drop_out, c.static.cfg.audio_channels) == (0.0, 0.5, 1)


def test_pit_pointwise_takes_stft_domain_shapes():
    """the pair-matrix kernel's view of [B, S, ..., n]: unchanged while B x rows fits its grid, one row per (batch, speaker) beyond"""
    from sehip import loss
    assert loss._pit_pointwise_view((3, 2, 2, 33, 21, 2)) == (3, 2, 2 * 33 * 21, 2)            # the fixture: as before
    assert loss._pit_pointwise_view((4, 2, 1, 16000)) == (4, 2, 1, 16000) and loss._pit_pointwise_view((4, 2)) == (4, 2, 1, 1)
    assert loss._pit_pointwise_view((16, 2, 2, 257, 501, 2)) == (16, 2, 1, 2 * 257 * 501 * 2)    # the shipped step: 4.1 M rows of 2 did not fit
    ws = loss.pit_pointwise_workspace((16, 2, 2, 257, 501, 2), "cpu")
    assert ws.shape[1] == 4 and 16 <= ws.shape[0] <= 1024
