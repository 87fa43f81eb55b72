"""CPU: mel-rnn (sehip.model.MelRNN at n_mels = 0) -- registry, schema, initialisation, rejections, the plan's host arithmetic, and the fp32
restatement tests/melrnn_ref.py pinned against vectors of the imported reference (tests/golden/melrnn_*.npz).

Tolerances of the restatement: 5e-5 relative for activations, outputs and gradients and 1e-5 for the running statistics, the values
tests/test_rnnmask_host.py and tests/test_oracle_golden.py use."""
import numpy as np
import pytest
import torch

import melrnn_ref as R
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


def test_registry_returns_melrnn():
    from sehip import SehipError, distrib, utils
    from sehip.model import MelRNN
    for tag in TAGS:
        m = distrib.get_model(utils.dict2obj(dict(name="mel-rnn", **kw(tag))))
        assert isinstance(m, MelRNN) and m.cfg.rnn_type == kw(tag)["rnn_type"]
    assert distrib.MODEL_REGISTRY["mel-rnn"] is MelRNN
    with pytest.raises(SehipError, match="has no HIP path yet"):        # the bare name is the constructor's default, n_mels = 128
        distrib.get_model(utils.dict2obj({"name": "mel-rnn"}))
    with pytest.raises(SehipError, match="has no HIP path yet"):
        MelRNN()
    with pytest.raises(SehipError, match="n_mels=128.*has no HIP path yet.*InverseMelScale"):
        MelRNN(n_mels=128, rnn_type="lstm")
    for name in ("unet", "crn"):
        with pytest.raises(SehipError, match="has no HIP path yet"):
            distrib.get_model(utils.dict2obj({"name": name}))
    # the YAML's way of switching the mel front end off: anything false
    assert MelRNN(n_mels=None, rnn_hidden=32).cfg.n_mels == 0 and MelRNN(n_mels=False, rnn_hidden=32).cfg.F == 257


@pytest.mark.parametrize("tag", TAGS)
def test_schema_and_optimizer(tag):
    from sehip import distrib, utils
    from sehip.model import MelRNN
    from sehip.model.flat import FlatModule
    from sehip.optim import FlatOptimizer
    fx = fixture(tag)
    m = MelRNN(**kw(tag))
    assert isinstance(m, FlatModule)
    sd = m.state_dict()
    assert list(sd) == list(fx["sd"]) and all(tuple(sd[k].shape) == tuple(v.shape) and sd[k].dtype == v.dtype for k, v in fx["sd"].items())
    assert {"fc_layers.0.weight", "fc_layers.0.bias", "fc_layers.2.weight", "fc_layers.2.bias"} <= set(sd)
    assert m.fc_layers[2].weight is dict(m.named_parameters())["fc_layers.2.weight"]
    names = R.param_names(fx["sd"])
    assert [n for n, _ in m.named_parameters()] == names
    m.load_state_dict(fx["adam"], strict=True)
    back = m.state_dict()
    assert all(torch.equal(back[k], fx["adam"][k]) for k in back)
    m.load_state_dict(fx["sd"], strict=True)
    assert float(m.flat_params.abs().sum()) == pytest.approx(sum(float(fx["sd"][k].abs().sum()) for k in names), rel=1e-5)
    opt = distrib.get_optimizer(utils.dict2obj({"optim": "adam", "lr": 3e-4, "beta1": 0.9, "beta2": 0.999}), m)
    assert isinstance(opt, FlatOptimizer) and len(opt.state_dict()["state"]) == len(names)
    assert m.set_deterministic(True) is m and not hasattr(m, "_tail_sink")


def test_initialisation_and_seed():
    from sehip.model import MelRNN
    torch.manual_seed(3)
    a = MelRNN(n_mels=0, rnn_type="rnn", rnn_hidden=256, rnn_layer=2)
    torch.manual_seed(3)
    b = MelRNN(n_mels=0, rnn_type="rnn", rnn_hidden=256, rnn_layer=2)
    assert torch.equal(a.flat_params, b.flat_params)
    sd = a.state_dict()
    w = sd["rnn.weight_hh_l1"]
    assert tuple(w.shape) == (256, 256) and tuple(sd["rnn.weight_ih_l0"].shape) == (256, 257) and tuple(sd["rnn.weight_ih_l1"].shape) == (256, 256)
    assert float(w.abs().max()) <= 1 / 16 and float(w.std()) == pytest.approx(1 / 16 / 3 ** 0.5, rel=0.05)
    assert float(sd["rnn.weight_ih_l0"].abs().max()) <= 1 / 16
    for key, shape, fan_in in (("fc_layers.0", (257, 256), 256), ("fc_layers.2", (257, 257), 257)):
        fc, bias, bound = sd[key + ".weight"], sd[key + ".bias"], 1 / fan_in ** 0.5
        assert tuple(fc.shape) == shape and float(fc.abs().max()) <= bound and float(fc.std()) == pytest.approx(bound / 3 ** 0.5, rel=0.05)
        assert tuple(bias.shape) == (257,) and float(bias.abs().max()) <= bound and float(bias.std()) == pytest.approx(bound / 3 ** 0.5, rel=0.2)
    assert bool((sd["batchnorm.weight"] == 1).all()) and bool((sd["batchnorm.bias"] == 0).all()) and bool((sd["batchnorm.running_mean"] == 0).all())
    assert bool((sd["batchnorm.running_var"] == 1).all()) and int(sd["batchnorm.num_batches_tracked"]) == 0
    # the gated cells keep PyTorch's stacked gate rows
    assert tuple(MelRNN(n_mels=0, rnn_type="lstm", rnn_hidden=64).state_dict()["rnn.weight_hh_l0"].shape) == (256, 64)
    assert tuple(MelRNN(n_mels=0, rnn_type="gru", rnn_hidden=64).state_dict()["rnn.weight_ih_l0"].shape) == (192, 257)
    # what the shipped YAML gives the model
    m = MelRNN(n_mels=0, rnn_type="lstm", rnn_hidden=896, rnn_layer=3, n_fft=512, hop_length=128)
    want = 4 * 896 * 257 + 2 * 4 * 896 * 896 + 3 * 4 * 896 * 896 + 2 * 896 + 257 * 896 + 257 + 257 * 257 + 257
    assert sum(p.numel() for p in m.parameters()) == want


@pytest.mark.parametrize("arg, value", [("n_mels", 128), ("n_mels", 40), ("rnn_type", "elman"), ("rnn_type", None), ("rnn_layer", 0), ("rnn_layer", 9),
                                        ("rnn_layer", 2.0), ("rnn_hidden", 48), ("rnn_hidden", 1056), ("rnn_hidden", 0), ("n_fft", 63), ("n_fft", 0),
                                        ("n_fft", 4098)])
def test_constructor_rejections(arg, value):
    from sehip import SehipError
    from sehip.model import MelRNN
    args = dict(n_mels=0, rnn_type="lstm")
    args[arg] = value
    with pytest.raises(SehipError, match=arg):
        MelRNN(**args)


def test_accepted_scope_and_input_rejections():
    from sehip import SehipError
    from sehip.model import MelRNN
    for cell in ("rnn", "lstm", "gru"):
        for h in (32, 96, 1024):
            MelRNN(n_mels=0, rnn_type=cell, rnn_hidden=h, rnn_layer=1)
    MelRNN(n_mels=0, rnn_layer=8, rnn_hidden=32, n_fft=4096)
    MelRNN(n_mels=0, rnn_hidden=32, n_fft=2, some_other_key=1)
    m = MelRNN(**kw("melrnn_rnn2"))
    with pytest.raises(SehipError, match="CPU tensor"):
        m(torch.zeros(3, 1, 33, 21, 2))
    with pytest.raises(SehipError, match="expected"):               # the reference's squeeze(dim=1) only works on one channel
        m(torch.zeros(3, 2, 33, 21, 2))
    with pytest.raises(SehipError, match="expected"):
        m(torch.zeros(3, 1, 32, 21, 2))
    with pytest.raises(SehipError, match="expected"):
        m(torch.zeros(3, 33, 21, 2))


# ---- the plan's host arithmetic -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_plan_arithmetic_fixtures(tag):
    from sehip import plan_melrnn as P
    cfg = P.MelRnnConfig(**kw(tag))
    st = P.MelRnnStatic(cfg)
    B, C, F, T, _ = R.FIXTURES[tag]["shape"]
    H, G = cfg.H, {"rnn": 1, "lstm": 4, "gru": 3}[cfg.rnn_type]
    GB = 1 if cfg.rnn_type == "rnn" else 4
    assert (cfg.F, cfg.Fp, cfg.D, cfg.Hout, cfg.G, cfg.GB) == (33, 40, 1, H, G, GB)
    shapes = st.buffer_shapes(B, T)
    rows = T * B
    want = {"feat": ((rows, 40), "bf16"), "a1": ((rows, 40), "bf16"), "mask": ((rows, 40), "bf16"), "dpre1": ((rows, 40), "bf16"),
            "dpre2": ((rows, 40), "bf16"), "z": ((rows, H), "bf16"), "dz": ((rows, H), "bf16"), "dy": ((rows, H), "bf16"),
            "out": ((B, 1, 1, 33, T, 2), "f32")}
    for k in range(cfg.rnn_layer):
        want.update({f"pre{k}": ((rows, 1, G, H), "f32"), f"hs{k}": ((rows, H), "bf16"), f"state{k}": ((rows, H), "f32"),
                     f"dG{k}": ((rows, 1, GB, H), "bf16")})
        if cfg.rnn_type != "rnn":
            want[f"gates{k}"] = ((rows, 1, 4, H), "f32")
        if k > 0:
            want[f"dx{k}"] = ((rows, H), "bf16")
    if cfg.rnn_type != "rnn":
        want["carry"] = ((1, T, H), "f32")           # the Elman backward reads dG(l + 1) back as stored: nothing is carried
    assert shapes == want
    assert st.step_launches(B) == (cfg.rnn_layer * B, cfg.rnn_layer * B)
    packs = st.pack_launches()
    assert len(packs) == 3 * cfg.rnn_layer + (cfg.rnn_layer - 1) + 4          # layer 0 needs no transposed W_ih: the input has no gradient
    offs = sorted((off, (K if tr else N) * ld) for _, _, N, K, tr, ld, off in packs)
    assert all(o % 8 == 0 for o, _ in offs) and all(a + n <= b for (a, n), (b, _) in zip(offs, offs[1:])) and offs[-1][0] + offs[-1][1] <= st.n_wpack
    assert st.w["fc2T"] - st.w["fc2"] == 33 * 40 and st.w["fc0T"] - st.w["fc0"] == 33 * H and st.n_wpack == st.w["fc2T"] + 33 * 40
    n_par = sum(int(np.prod(s)) for _, s, kind in cfg.param_specs() if kind == "param")
    assert n_par == {"melrnn_rnn2": 6403, "melrnn_lstm1": 28227, "melrnn_gru2": 14659}[tag] == sum(fixture(tag)["sd"][k].numel() for k in R.param_names(fixture(tag)["sd"]))


def test_plan_arithmetic_shipped():
    from sehip import plan_melrnn as P
    from sehip.model import MelRNN
    cfg = P.MelRnnConfig(rnn_type="lstm", rnn_hidden=896, rnn_layer=3, n_mels=0, n_fft=512, hop_length=128)
    st = P.MelRnnStatic(cfg)
    assert (cfg.F, cfg.Fp, cfg.H) == (257, 264, 896)
    shapes = st.buffer_shapes(32, 501)                                   # [16, 2, 64000] arrives as 32 mono items of 501 frames
    assert shapes["feat"][0] == (501 * 32, 264) and shapes["pre2"][0] == (501 * 32, 1, 4, 896) and shapes["mask"][0] == (501 * 32, 264)
    assert st.step_launches(32) == (96, 96)
    assert st.w[(0, "hh")] - st.w[(0, "ihT")] == 264 * 4 * 896 and st.w[(1, "ihT")] - st.w[(1, "ih")] == 4 * 896 * 896
    el = P.MelRnnStatic(P.MelRnnConfig(rnn_type="rnn", rnn_hidden=896, rnn_layer=3, n_mels=0, n_fft=512))
    assert el.w[(1, "hh")] - el.w[(1, "ihT")] == 896 * 896 and "gates0" not in el.buffer_shapes(32, 501)
    # models of one configuration share the static plan, others do not
    a, b, c = (MelRNN(n_mels=0, rnn_hidden=32, rnn_type=t) for t in ("rnn", "rnn", "gru"))
    assert a.static is b.static and a.static is not c.static


# ---- the restatement against the reference's vectors ------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_restatement_reproduces_reference(tag):
    fx = fixture(tag)
    names = R.param_names(fx["sd"])
    p = {k: (v.clone().requires_grad_(True) if k in names else v.clone()) for k, v in fx["sd"].items()}
    taps, run = {}, {}
    est = R.melrnn_forward(p, fx["input"], taps=taps, running=run, **kw(tag))
    assert rel_err(est.detach(), fx["est"]) < ACT_TOL
    assert set(taps) == set(fx["tap"]) == {f"rnn{k}" for k in range(kw(tag)["rnn_layer"])} | {"bn", "relu", "head"}
    for k, v in fx["tap"].items():
        assert rel_err(taps[k].detach(), v) < ACT_TOL, k
    for k, v in fx["run"].items():
        assert rel_err(run[k].float(), v.float()) < STAT_TOL, k
    (est * fx["G"]).sum().backward()
    for k in names:
        assert rel_err(p[k].grad, fx["gradG"][k]) < ACT_TOL, k
        p[k].grad = None
    loss = torch.nn.functional.mse_loss(R.melrnn_forward(p, fx["input"], **kw(tag)), fx["target"])
    assert abs(float(loss) - float(fx["loss"])) < 1e-5 * float(fx["loss"])
    loss.backward()
    for k in names:
        assert rel_err(p[k].grad, fx["grad"][k]) < ACT_TOL, k
    q = dict(fx["sd"])
    q.update(run)
    with torch.no_grad():
        assert rel_err(R.melrnn_forward(q, fx["input"], training=False, **kw(tag)), fx["est_eval"]) < ACT_TOL


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_two_adam_steps(tag):
    fx = fixture(tag)
    names = R.param_names(fx["sd"])
    p = {k: (v.clone().requires_grad_(True) if k in names else v.clone()) for k, v in fx["sd"].items()}
    opt = torch.optim.Adam([p[k] for k in names], lr=3e-4, betas=(0.9, 0.999))
    for i in range(2):
        run = {}
        loss = torch.nn.functional.mse_loss(R.melrnn_forward(p, fx["input"], running=run, **kw(tag)), fx["target"])
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_([p[k] for k in names], 5)
        opt.step()
        p.update(run)
        assert abs(float(loss) - float(fx["adam_losses"][i])) < 1e-5 * float(fx["adam_losses"][i]), i
    assert float(fx["adam_losses"][1]) < float(fx["adam_losses"][0])
    for k in ("batchnorm.running_mean", "batchnorm.running_var"):
        assert rel_err(p[k], fx["adam"][k]) < STAT_TOL, k
    assert int(p["batchnorm.num_batches_tracked"]) == int(fx["adam"]["batchnorm.num_batches_tracked"]) == 2


def test_restatement_in_float64_and_bf16_storage():
    tag = "melrnn_rnn2"
    fx = fixture(tag)
    p64 = {k: (v.double() if v.is_floating_point() else v) for k, v in fx["sd"].items()}
    est = R.melrnn_forward(p64, fx["input"].double(), **kw(tag))
    assert est.dtype == torch.float64 and rel_err(est, fx["est"]) < ACT_TOL
    sim = R.melrnn_forward(fx["sd"], fx["input"], sim=R.Bf16Sim, **kw(tag))
    assert 1e-4 < rel_err(sim, fx["est"]) < 5e-2
    # the recurrence walks the batch axis: an utterance's output depends on the batch it is in
    alone = R.melrnn_forward(fx["sd"], fx["input"][1:2], **kw(tag))
    assert rel_err(alone, fx["est"][1:2]) > 1e-3
