"""CPU: the Wave-U-Net module (`wav-unet`) -- registry, checkpoint schema against the reference's, un-packing table, rejections, the
library's new entry points -- and the restatement tests/wavunet_ref.py against vectors of the imported reference
(tests/golden/wavunet_*.npz, tools/gen_golden_wavunet.py)."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import wavunet_ref as R
from ctn_variants_ref import grad_dev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAGS = sorted(R.FIXTURES)
_FX = {}


def fixture(tag):
    if tag not in _FX:
        _FX[tag] = R.load_fixture(os.path.join(ROOT, "tests", "golden", tag + ".npz"))
    return _FX[tag]


def model_kw(tag):
    return dict(unet_nlayers=R.FIXTURES[tag]["unet_nlayers"], channels_interval=R.FIXTURES[tag]["channels_interval"])


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def test_registry_returns_wavunet():
    from sehip import SehipError, distrib, utils
    from sehip.model import WavUnet
    m = distrib.get_model(utils.dict2obj({"name": "wav-unet", "unet_nlayers": 3, "channels_interval": 8}))
    assert isinstance(m, WavUnet) and m.cfg.key() == (3, 8)
    for name in ("mel-rnn", "unet", "crn", "rnn-stft-mask"):          # the other four names keep their message
        with pytest.raises(SehipError, match="has no HIP path yet"):
            distrib.get_model(utils.dict2obj({"name": name}))


@pytest.mark.parametrize("tag", TAGS)
def test_schema_optimizer_and_unpack_table(tag):
    from sehip import distrib, utils
    from sehip.model import WavUnet
    fx = fixture(tag)
    m = WavUnet(**model_kw(tag))
    sd = m.state_dict()
    assert list(sd) == list(fx["sd"]) and all(tuple(sd[k].shape) == tuple(v.shape) and sd[k].dtype == v.dtype for k, v in fx["sd"].items())
    names = R.param_names(fx["sd"])
    assert [n for n, _ in m.named_parameters()] == names             # optimizer state indices interchange
    m.load_state_dict(fx["adam"])                                     # a checkpoint with non-trivial running statistics and counters
    back = m.state_dict()
    assert all(torch.equal(back[k], fx["adam"][k]) for k in back)
    assert float(m.flat_params.abs().sum()) == pytest.approx(sum(float(fx["adam"][k].abs().sum()) for k in names), rel=1e-5)
    opt = distrib.get_optimizer(utils.dict2obj({"optim": "adam", "lr": 3e-4, "beta1": 0.9, "beta2": 0.999}), m)
    assert len(opt.state_dict()["state"]) == len(names)
    st = m.static
    L = st.layout
    real = np.concatenate([L.index_array(n).reshape(-1) for n in L.param_names])
    assert len(real) == sum(fx["sd"][k].numel() for k in names)
    assert (st.utab1[real] >= 0).all() and len(np.unique(st.utab1[real])) == len(real)       # exactly one packed-gradient entry each
    pad = np.ones(L.n_params, dtype=bool)
    pad[real] = False
    assert (st.utab1[pad] == -1).all() and int(st.utab1.max() >> 1) < st.n_gpack


def test_default_network_and_initialisation():
    from sehip.model import WavUnet
    m = WavUnet()
    assert sum(p.numel() for p in m.parameters()) == 10132802
    assert [m.cfg.enc_channels(l)[1] for l in (0, 11)] == [24, 288] and [sum(m.cfg.dec_channels(i)[:2]) for i in (0, 11)] == [576, 72]
    sd = m.state_dict()
    w = sd["encoder.3.main.0.weight"]                                  # U(+-1/sqrt(fan_in)): std = bound / sqrt(3)
    bound = 1 / (w.shape[1] * w.shape[2]) ** 0.5
    assert float(w.abs().max()) <= bound and float(w.std()) == pytest.approx(bound / 3 ** 0.5, rel=0.05)
    assert float(sd["encoder.3.main.0.bias"].abs().max()) <= bound and float(sd["encoder.3.main.0.bias"].std()) > 0
    assert bool((sd["middle.1.weight"] == 1).all()) and bool((sd["middle.1.bias"] == 0).all())
    assert bool((sd["decoder.2.main.1.running_var"] == 1).all()) and bool((sd["decoder.2.main.1.running_mean"] == 0).all())
    assert int(sd["out.0.weight"].shape[1]) == 25 and int(sd["decoder.0.main.1.num_batches_tracked"]) == 0
    assert m.valid_length(16000) == 16384


def test_rejections():
    from sehip import SehipError
    from sehip.model import WavUnet
    with pytest.raises(SehipError, match="channels_interval"):
        WavUnet(channels_interval=12)
    with pytest.raises(SehipError, match="unet_nlayers"):
        WavUnet(unet_nlayers=13)
    m = WavUnet(unet_nlayers=2, channels_interval=8)
    with pytest.raises(SehipError, match="CPU tensor"):
        m(torch.zeros(1, 1, 64))
    with pytest.raises(SehipError):
        m(torch.zeros(1, 64))


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_forward_against_reference(tag):
    fx = fixture(tag)
    taps, run = {}, {}
    est = R.wavunet_forward(fx["sd"], fx["mix"], taps=taps, running=run, **model_kw(tag))
    assert sorted(taps) == sorted(fx["tap"])
    for k, v in fx["tap"].items():
        assert tuple(taps[k].shape) == tuple(v.shape) and rel(taps[k], v) < 2e-5, k
    assert rel(est, fx["est"]) < 2e-5
    assert sorted(run) == sorted(fx["run"])
    for k, v in fx["run"].items():
        if k.endswith("num_batches_tracked"):
            assert int(run[k]) == int(v) == 1
        else:
            assert rel(run[k], v) < 2e-5, k
    sd = dict(fx["sd"])
    sd.update(fx["run"])
    assert rel(R.wavunet_forward(sd, fx["mix"], training=False, **model_kw(tag)), fx["est_eval"]) < 2e-5


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_gradients_against_reference(tag):
    fx = fixture(tag)
    g, _ = R.fixed_g_grads(fx["sd"], fx["mix"], fx["G"], **model_kw(tag))
    dev, worst = grad_dev(g, fx["gradG"], list(g))
    assert dev < 5e-4 and worst < 5e-4, (dev, worst)
    from oracle.dccrn_oracle import loss_sisdr
    names = R.param_names(fx["sd"])
    p = {k: (v.clone().requires_grad_(True) if k in names else v) for k, v in fx["sd"].items()}
    loss = loss_sisdr(R.wavunet_forward(p, fx["mix"], **model_kw(tag)), fx["target"])
    assert abs(loss.item() - fx["loss"]) < 1e-3
    loss.backward()
    dev, worst = grad_dev({k: p[k].grad for k in names}, fx["grad"], names)
    assert dev < 5e-4 and worst < 5e-4, (dev, worst)


@pytest.mark.parametrize("t_in", [2, 3, 25, 33, 64])
def test_interpolation_table(t_in):
    """the integer source index and weight (plan_wavunet.up2_table: what csrc/wavunet.hip computes) against F.interpolate"""
    from sehip.plan_wavunet import up2_table
    i0, i1, w = up2_table(t_in)
    assert i0.min() == 0 and i1.max() == t_in - 1 and ((i1 - i0 == 1) | ((i0 == t_in - 1) & (w == 0))).all() and (w >= 0).all() and (w < 1).all()
    z = torch.randn(2, 3, t_in, dtype=torch.float64, generator=torch.Generator().manual_seed(t_in))
    ref = F.interpolate(z, scale_factor=2, mode="linear", align_corners=True)
    got = z[..., torch.as_tensor(i0)] * torch.as_tensor(1 - w) + z[..., torch.as_tensor(i1)] * torch.as_tensor(w)
    assert float((got - ref).abs().max()) < 1e-6
    # every source frame is touched by output positions 2 i - 2 .. 2 i + 2 only (the backward kernel's gather window)
    for i in range(t_in):
        touched = np.flatnonzero(((i0 == i) & (w < 1)) | ((i1 == i) & (w > 0)))
        assert touched.min() >= 2 * i - 2 and touched.max() <= 2 * i + 2
    a0, a1, aw = R.up2_table(t_in)                                  # the restatement's own table is the same
    assert (a0 == i0).all() and (a1 == i1).all() and np.array_equal(aw, w)


def _wun_symbols():
    text = open(os.path.join(ROOT, "include", "sehip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sehip_wun_[a-z0-9_]+)\s*\(", text)))


def test_library_symbols_and_argument_validation():
    from sehip import _lib
    lib = _lib.lib()
    names = _wun_symbols()
    expected = {"sehip_wun_enc0_fwd", "sehip_wun_enc0_wgrad", "sehip_wun_bn_stats", "sehip_wun_bn_finalize", "sehip_wun_bn_apply",
                "sehip_wun_bn_apply_up2", "sehip_wun_up2_bwd", "sehip_wun_bn_bwd_reduce", "sehip_wun_bn_bwd_finalize", "sehip_wun_bn_bwd_apply",
                "sehip_wun_out_fwd", "sehip_wun_out_bwd", "sehip_wun_bn_scratch_floats", "sehip_wun_enc0_wgrad_scratch_floats",
                "sehip_wun_out_bwd_scratch_floats"}
    assert expected <= set(names)
    for n in names:
        assert hasattr(lib, n), n                                     # exported
        assert n in _lib._PROTOS, n                                   # prototyped
    assert sorted(n for n in _lib._PROTOS if n.startswith("sehip_wun_")) == names     # ... and nothing prototyped that is not declared
    # argument validation happens before any launch: safe without a GPU
    assert lib.sehip_wun_bn_apply(None, None, 100, 24, None, None) != 0 and b"null pointer" in lib.sehip_last_error()
    assert lib.sehip_wun_bn_stats(None, 100, 12, None, None) != 0 and b"multiple of 8" in lib.sehip_last_error()
    assert lib.sehip_wun_bn_apply_up2(None, None, 2, 1, 24, None, None) != 0 and b"two source frames" in lib.sehip_last_error()
    assert lib.sehip_wun_bn_bwd_reduce(None, None, None, None, 101, 24, None, None) != 0
    with pytest.raises(_lib.SehipError):
        _lib.call("sehip_wun_out_fwd", None, None, None, None, 100, 24, None, None)
    assert lib.sehip_wun_bn_scratch_floats(1000, 24) > 0 and lib.sehip_wun_bn_scratch_floats(1000, 12) == 0
    assert lib.sehip_wun_enc0_wgrad_scratch_floats(2, 200, 8) >= 2 * 16 * 8


def _emulate(st, p, flat, srcs, T):
    """the engine's product p on one utterance, from the plan's own tables: srcs [T][C of the bound view] per source -> one [T][C] per
    destination (chunk table: (source, frame offset, -, channel offset) per 8 columns of K; column table: (destination, first column,
    valid columns) per 4 outputs; zero outside the source's frames)"""
    kt = st.ktab[p.kt_off:p.kt_off + p.K // 8]
    A = np.zeros((T, p.K))
    for c, (s, toff, _, coff) in enumerate(kt):
        if s < 0:
            continue
        for t in range(T):
            if 0 <= t + toff < T:
                A[t, 8 * c:8 * c + 8] = srcs[s][t + toff, coff:coff + 8]
    w = st.wtab[p.w_off:p.w_off + p.Npad * p.K].reshape(p.Npad, p.K)
    out = A @ np.where(w >= 0, flat[np.maximum(w, 0) >> 1], 0.0).T
    if p.b_off is not None:
        b = st.btab[p.b_off:p.b_off + p.Npad, 0]
        out = out + np.where(b >= 0, flat[np.maximum(b, 0) >> 1], 0.0)
    dsts = [np.zeros((T, c)) for _, c in p.dsts]
    for g, (d, coff, nvalid, _) in enumerate(st.ntab[p.nt_off:p.nt_off + p.Npad // 4]):
        dsts[d][:, coff:coff + nvalid] = out[:, 4 * g:4 * g + nvalid]
    return dsts


def test_products_reproduce_the_convolutions():
    """every kind of product of the plan, emulated on the host from its packing / chunk / column tables, against F.conv1d and
    F.conv_transpose1d: the pair-view decimation, the two-source decoder convolution and its two-destination input gradient"""
    from sehip import plan_wavunet as P
    st = P.WavUnetStatic(P.WavUnetConfig(unet_nlayers=3, channels_interval=8))
    L = st.layout
    rng = np.random.default_rng(0)
    flat = rng.standard_normal(L.n_params)
    get = lambda n: torch.from_numpy(flat[L.param_off[n][0]:L.param_off[n][0] + int(np.prod(L.param_off[n][1]))].reshape(L.param_off[n][1]))
    rnd = lambda c, t: torch.from_numpy(rng.standard_normal((1, c, t)))
    T = 10
    # encoder layer 2 (16 -> 24 channels) over the pair view of z1 [2 T][16]
    z = rnd(16, 2 * T)
    want = F.conv1d(z[:, :, ::2], get("encoder.2.main.0.weight"), get("encoder.2.main.0.bias"), padding=7)
    got, = _emulate(st, st.prods["e2.fwd"], flat, [z[0].t().reshape(T, 32).numpy()], T)
    assert np.allclose(got.T, want[0].numpy(), atol=1e-9)
    dy = rnd(24, T)
    want = F.conv_transpose1d(dy, get("encoder.2.main.0.weight"), padding=7)
    got, = _emulate(st, st.prods["e2.dg"], flat, [dy[0].t().numpy()], T)
    assert np.allclose(got.T, want[0].numpy(), atol=1e-9)
    # the middle block reads encoder 2's z the same way
    z = rnd(24, 2 * T)
    want = F.conv1d(z[:, :, ::2], get("middle.0.weight"), get("middle.0.bias"), padding=7)
    got, = _emulate(st, st.prods["m.fwd"], flat, [z[0].t().reshape(T, 48).numpy()], T)
    assert np.allclose(got.T, want[0].numpy(), atol=1e-9)
    # decoder layer 1: up (24 channels) | skip (16) -> 16, and its input gradient to the two halves
    up, skip = rnd(24, T), rnd(16, T)
    want = F.conv1d(torch.cat([up, skip], 1), get("decoder.1.main.0.weight"), get("decoder.1.main.0.bias"), padding=2)
    got, = _emulate(st, st.prods["d1.fwd"], flat, [up[0].t().numpy(), skip[0].t().numpy()], T)
    assert np.allclose(got.T, want[0].numpy(), atol=1e-9)
    dy = rnd(16, T)
    want = F.conv_transpose1d(dy, get("decoder.1.main.0.weight"), padding=2)
    d_up, d_skip = _emulate(st, st.prods["d1.dg"], flat, [dy[0].t().numpy()], T)
    assert np.allclose(d_up.T, want[0, :24].numpy(), atol=1e-9) and np.allclose(d_skip.T, want[0, 24:].numpy(), atol=1e-9)
    assert [b for b, _ in st.prods["d1.dg"].dsts] == ["d1.dup", "e1.dskip"] and st.prods["d1.fwd"].srcs == [("d1.up", False), ("e1.z", False)]


@pytest.mark.parametrize("tag", TAGS)
def test_plan_on_the_emulated_c_abi(tag, monkeypatch):
    """the plan's own forward() / backward() on the CPU, every library call answered by tests/wavunet_cabi_emulator.py (numpy on the raw
    pointers, from the documented semantics): buffer wiring, pointer offsets, bound tables and launch order against the reference's
    vectors, with the bound the GPU chain test uses (2 x the deviation of the bf16-storage restatement)"""
    from sehip import plan_wavunet as P
    from sehip.model import WavUnet
    from wavunet_cabi_emulator import Emulator
    fx = fixture(tag)
    emu = Emulator()
    monkeypatch.setenv("SEHIP_NO_SIDE_STREAM", "1")
    from sehip import workspace as W
    for mod in (P, W):            # (gemm() and wgrad() launch from the workspace base)
        monkeypatch.setattr(mod, "call", emu)
        monkeypatch.setattr(mod, "stream", lambda: None)
    model = WavUnet(**model_kw(tag))
    model.load_state_dict(fx["sd"])
    cpu = torch.device("cpu")
    B, _, T = fx["mix"].shape
    ws = P.WavUnetWorkspace(model.static, P.WavUnetDeviceTables(model.static, cpu), B, T, cpu)
    est = ws.forward(fx["mix"].contiguous(), model._flat, model._bflat, model._nbt, training=True).clone()
    grads = torch.zeros_like(model._flat)
    ws.backward(fx["G"].contiguous(), model._flat, grads)
    L = model.static.layout
    got = {k: grads[L.param_off[k][0]:L.param_off[k][0] + fx["sd"][k].numel()].view(fx["sd"][k].shape) for k in L.param_names}
    gs, ests = R.fixed_g_grads(fx["sd"], fx["mix"], fx["G"], sim=R.Bf16Sim, **model_kw(tag))
    dev, sim_dev = rel(est, fx["est"]), rel(ests, fx["est"])
    (glob, _), (sglob, _) = grad_dev(got, fx["gradG"], list(got)), grad_dev(gs, fx["gradG"], list(gs))
    print(f"WavUnet {tag} plan on the emulated C ABI: est {dev:.3e} (restatement {sim_dev:.3e}), gradients {glob:.4f} (restatement {sglob:.4f})")
    assert dev < 2 * sim_dev and glob < 2 * sglob
    after = model.state_dict()
    for k, v in fx["run"].items():
        assert (int(after[k]) == 1) if k.endswith("num_batches_tracked") else rel(after[k], v) < 1e-2, k
    n = model.cfg.n
    assert emu.calls.count("sehip_gemm") == 2 * (2 * n)  and emu.calls.count("sehip_wgrad") == 2 * n      # 2 n products forward, 2 n input gradients
    assert emu.calls.count("sehip_wun_bn_apply_up2") == n == emu.calls.count("sehip_wun_up2_bwd") and emu.calls[-1] == "sehip_unpack_grad1"
    # eval mode: running statistics, forward only
    ev = ws.forward(fx["mix"].contiguous(), model._flat, model._bflat, model._nbt, training=False).clone()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    assert rel(ev, R.wavunet_forward(sd, fx["mix"], training=False, **model_kw(tag))) < 2 * sim_dev
    from sehip import SehipError
    with pytest.raises(SehipError, match="eval mode"):
        ws.backward(fx["G"].contiguous(), model._flat, grads)
