"""CPU: the U-Net module (`unet`) -- registry, refusals, checkpoint schema against the reference's, un-packing table, the library's new
entry points -- the restatement tests/unet_ref.py against vectors of the imported reference (tests/golden/unet_*.npz,
tools/gen_golden_unet.py), its pool and its dropout twin, the plan's products emulated from their tables against F.conv2d /
F.conv_transpose2d, and the plan's own forward() / backward() on an emulated C ABI (tests/unet_cabi_emulator.py).

What bf16 storage alone does to the fixtures (the restatement under Bf16Sim against the reference's vectors; the GPU chain test takes its
bound, 2 x these, from the same computation), l1_c1 / l2_c2:
  est 6.22e-3 / 5.39e-3; taps 1.5e-3 (amp) .. 1.9e-2 (dec0 of l2_c2); gradients of <est, G> 0.147 / 0.268 global (0.229 / 0.381 worst large
  tensor: the deepest levels normalise over 36 / 45 values per channel and every pool / LeakyReLU decision next to a tie flips under a
  rounding); the plan on the emulated C ABI: est 6.22e-3 / 5.29e-3, gradients 0.147 / 0.211; with dropout 0.5 (l2_c2, under the twin's
  masks, against the fp32 restatement with the same masks) est 5.38e-3 and gradients 0.169 beside the restatement's 5.07e-3 / 0.183
"""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import unet_ref as R
from ctn_variants_ref import grad_dev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAGS = sorted(R.FIXTURES)
fixture, model_kw = R.fixture, R.model_kw


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def test_registry_returns_unet():
    from sehip import distrib, utils
    from sehip.model import UNet
    m = distrib.get_model(utils.dict2obj({"name": "unet", "unet_channels": 1}))
    assert isinstance(m, UNet) and distrib.MODEL_REGISTRY["unet"] is UNet
    assert m.cfg.key() == (1, 4, 0.5) and sum(p.numel() for p in m.parameters()) == 1959142       # the reference README's 7.5 MB "Unet"
    # the shipped YAML's keys, the DNN's drop_out among them (it reaches every constructor and is not this model's dropout)
    m = distrib.get_model(utils.dict2obj({"name": "unet", "unet_channels": 2, "unet_layer": 2, "bilinear": False, "drop_out": 0.1,
                                          "audio_channels": 1}))
    assert m.cfg.key() == (2, 2, 0.5)
    assert distrib.get_model(utils.dict2obj({"name": "unet", "unet_channels": 1, "unet_layer": 1, "unet_dropout": 0.25})).cfg.p == 0.25


def test_refusals_by_message():
    from sehip import SehipError, distrib, utils
    from sehip.model import UNet
    with pytest.raises(SehipError, match="has no HIP path yet") as e:          # the bare name: the reference's constructor has no default
        distrib.get_model(utils.dict2obj({"name": "unet"}))
    assert "unet_channels" in str(e.value) and "no default" in str(e.value)
    with pytest.raises(SehipError, match="crn.*has no HIP path yet"):
        distrib.get_model(utils.dict2obj({"name": "crn"}))
    with pytest.raises(SehipError, match=r"bilinear=True has no HIP path yet: the transposed-convolution decoder \(bilinear: False, the shipped "
                                         r"setting\) is built"):
        UNet(1, bilinear=True)
    for bad in (0, 16, -1, 1.5, "1", True):
        with pytest.raises(SehipError, match=r"unet_channels=.* must be an integer in 1 \.\. 15"):
            UNet(bad)
    for bad in (0, 5, 2.0, None):
        with pytest.raises(SehipError, match=r"unet_layer=.* must be an integer in 1 \.\. 4"):
            UNet(1, unet_layer=bad)
    for bad in (-0.1, 1.5, "half"):
        with pytest.raises(SehipError, match=r"unet_dropout=.* must be a probability in \[0, 1\]"):
            UNet(1, unet_dropout=bad)
    m = UNet(2, unet_layer=2)
    with pytest.raises(SehipError, match=r"\[R, unet_channels=2, F, T, 2\] expected"):
        m(torch.zeros(2, 2, 8, 8))
    with pytest.raises(SehipError, match=r"\[R, unet_channels=2, F, T, 2\] expected"):
        m(torch.zeros(2, 1, 8, 8, 2))
    with pytest.raises(SehipError, match=r"F and T must be at least 2\^2 = 4"):
        m(torch.zeros(2, 2, 3, 8, 2))
    with pytest.raises(SehipError, match=r"F and T must be at least 2\^2 = 4"):
        m(torch.zeros(2, 2, 8, 3, 2))
    with pytest.raises(SehipError, match="CPU tensor"):
        m(torch.zeros(2, 2, 8, 8, 2))


@pytest.mark.parametrize("tag", TAGS)
def test_schema_optimizer_and_unpack_table(tag):
    from sehip import distrib, utils
    from sehip.model import UNet
    fx = fixture(tag)
    m = UNet(**model_kw(tag))
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
    from sehip.model import UNet
    torch.manual_seed(3)
    m = UNet(1)
    assert m.cfg.width == [16, 32, 64, 128, 256] and m.cfg.Cp == 8 and UNet(9, unet_layer=1).cfg.Cp == 16
    sd = m.state_dict()
    w = sd["encoder.2.maxpool_conv.0.double_conv.3.weight"]            # Conv2d: U(+-1/sqrt(fan_in)), std = bound / sqrt(3)
    bound = 1 / (w.shape[1] * 9) ** 0.5
    assert tuple(w.shape) == (64, 64, 3, 3) and float(w.abs().max()) <= bound and float(w.std()) == pytest.approx(bound / 3 ** 0.5, rel=0.05)
    w = sd["decoder.1.up.weight"]                                      # ConvTranspose2d: torch's fan_in of a transposed weight is size(1) x 4
    bound = 1 / (w.shape[1] * 4) ** 0.5
    assert tuple(w.shape) == (128, 64, 2, 2) and float(w.abs().max()) <= bound and float(w.std()) == pytest.approx(bound / 3 ** 0.5, rel=0.05)
    b = sd["decoder.1.up.bias"]
    assert float(b.abs().max()) <= bound and float(b.std()) > 0
    assert "decoder.0.up.weight" not in sd and tuple(sd["outconv.up.weight"].shape) == (16, 8, 2, 2)
    assert tuple(sd["outconv.conv.double_conv.0.weight"].shape) == (1, 9, 3, 3)
    assert bool((sd["middle.double_conv.4.weight"] == 1).all()) and bool((sd["middle.double_conv.4.bias"] == 0).all())
    assert bool((sd["decoder.2.conv.double_conv.1.running_var"] == 1).all()) and int(sd["outconv.conv.double_conv.4.num_batches_tracked"]) == 0
    torch.manual_seed(3)
    assert UNet(1).dropout_seed == m.dropout_seed                       # torch.manual_seed reproduces the dropout stream


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_forward_against_reference(tag):
    fx = fixture(tag)
    taps, run = {}, {}
    est = R.unet_forward(fx["sd"], fx["mix"], taps=taps, running=run, **model_kw(tag))
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
    assert rel(R.unet_forward(sd, fx["mix"], training=False, **model_kw(tag)), fx["est_eval"]) < 2e-5


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_gradients_and_adam_against_reference(tag):
    fx = fixture(tag)
    g, _ = R.fixed_g_grads(fx["sd"], fx["mix"], fx["G"], **model_kw(tag))
    dev, worst = grad_dev(g, fx["gradG"], list(g))
    assert dev < 5e-4 and worst < 5e-4, (dev, worst)
    names = R.param_names(fx["sd"])
    p = {k: (v.clone().requires_grad_(True) if k in names else v) for k, v in fx["sd"].items()}
    loss = F.mse_loss(R.unet_forward(p, fx["mix"], **model_kw(tag)), fx["target"])
    assert abs(loss.item() - fx["loss"]) < 2e-5 * fx["loss"]
    loss.backward()
    dev, worst = grad_dev({k: p[k].grad for k in names}, fx["grad"], names)
    assert dev < 5e-4 and worst < 5e-4, (dev, worst)
    losses, final = R.adam_steps(fx["sd"], fx["mix"], fx["target"], **model_kw(tag))
    assert all(abs(a - b) < 2e-5 * b for a, b in zip(losses, fx["adam_losses"]))
    upd = lambda d: {k: d[k].double() - fx["sd"][k].double() for k in names}
    assert grad_dev(upd(final), upd(fx["adam"]), names)[0] < 5e-4
    for k, v in fx["adam"].items():
        if not k in names:
            assert (int(final[k]) == int(v) == 2) if k.endswith("num_batches_tracked") else rel(final[k], v) < 2e-5, k


@pytest.mark.parametrize("tag", TAGS)
def test_bf16_storage_deviation(tag):
    """what bf16 storage alone does to the fixtures: printed, and sane (the GPU chain bound is 2 x these, computed there in the same way)"""
    fx = fixture(tag)
    taps = {}
    gs, ests = R.fixed_g_grads(fx["sd"], fx["mix"], fx["G"], sim=R.Bf16Sim, taps=taps, **model_kw(tag))
    dev = rel(ests, fx["est"])
    glob, worst = grad_dev(gs, fx["gradG"], list(gs))
    print(f"UNet {tag} bf16-storage restatement: est {dev:.3e}, gradients of <est, G> {glob:.4f} global / {worst:.4f} worst large tensor; taps "
          + ", ".join(f"{k} {rel(v.detach(), fx['tap'][k]):.2e}" for k, v in sorted(taps.items())))
    assert 1e-4 < dev < 5e-2 and 1e-3 < glob < 0.3
    # every tap is stored bf16 except the mask: a value that is not representable would mean a storage point was missed
    for k, v in taps.items():
        if k != "head":
            assert torch.equal(v.detach().bfloat16().float(), v.detach().float()), k


def test_pool_tie_rule_and_floor():
    """the restatement's pool against F.max_pool2d(return_indices=True) on tensors with planted ties: first maximum in the scan order
    (F offset outer, T offset inner), odd sizes floored"""
    g = torch.Generator().manual_seed(0)
    for (f, t) in ((2, 2), (5, 4), (4, 5), (9, 7), (6, 6)):
        z = torch.randint(-2, 3, (2, 3, f, t), generator=g).double()           # five distinct values: most windows hold a tie
        z[0, 0, :2, :2] = 1.0                                                   # a window of four equal values
        z[1, 2, :2, :2] = torch.tensor([[0.0, 3.0], [3.0, 3.0]])               # the maximum first met at (F 0, T 1)
        want, idx = F.max_pool2d(z, 2, return_indices=True)
        codes = []
        got = R.max_pool2(z, codes)
        assert tuple(got.shape) == (2, 3, f // 2, t // 2) and torch.equal(got, want)
        ff, tt = idx // t, idx % t
        assert torch.equal(codes[0], 2 * (ff % 2) + (tt % 2))
        assert int(codes[0][0, 0, 0, 0]) == 0 and int(codes[0][1, 2, 0, 0]) == 1
        zz = z.clone().requires_grad_(True)                                     # the gradient goes to the coded element only
        R.max_pool2(zz).sum().backward()
        z2 = z.clone().requires_grad_(True)
        F.max_pool2d(z2, 2).sum().backward()
        assert torch.equal(zz.grad, z2.grad)
        if f % 2:
            assert bool((zz.grad[:, :, -1] == 0).all())
        if t % 2:
            assert bool((zz.grad[:, :, :, -1] == 0).all())


def test_dropout_twin():
    from sehip.plan_rnnmask import drop_keep_mask, drop_threshold
    n = 1 << 16
    for p in (0.5, 0.25):
        m = R.drop_keep_mask(1234567890123, 3, R.DROP_MIDDLE, n, p)
        assert np.array_equal(m, drop_keep_mask(1234567890123, 3, R.DROP_MIDDLE, n, p))       # the plan's twin is the same generator
        assert abs(m.mean() - (1 - p)) < 4 * (p * (1 - p) / n) ** 0.5
        assert drop_threshold(p)[1] == pytest.approx(1 / (1 - p))
    a, b = R.drop_keep_mask(1, 0, 0, n, 0.5), R.drop_keep_mask(1, 0, 1, n, 0.5)
    assert 0.4 < (a == b).mean() < 0.6 and not np.array_equal(a, R.drop_keep_mask(1, 1, 0, n, 0.5)) and not np.array_equal(a, R.drop_keep_mask(2, 0, 0, n, 0.5))
    # the restatement scales what it keeps and indexes the tensor channels-last
    z = torch.ones(2, 16, 3, 5, dtype=torch.float64)
    d = R.dropout(z, dict(seed=9, counter=0, p=0.5), R.DROP_ENCODER)
    keep = R.drop_keep_mask(9, 0, R.DROP_ENCODER, z.numel(), 0.5).reshape(2, 5, 3, 16)
    assert set(d.unique().tolist()) == {0.0, 2.0} and np.array_equal(d.permute(0, 3, 2, 1).numpy() == 2.0, keep)
    assert torch.equal(R.dropout(z, dict(seed=9, counter=0, p=0.0), 0), z) and float(R.dropout(z, dict(seed=9, counter=0, p=1.0), 0).abs().sum()) == 0


def _unet_symbols():
    text = open(os.path.join(ROOT, "include", "sehip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sehip_unet_[a-z0-9_]+)\s*\(", text)))


def test_library_symbols_and_argument_validation():
    from sehip import _lib
    lib = _lib.lib()
    names = _unet_symbols()
    assert {"sehip_unet_features", "sehip_unet_bn_act", "sehip_unet_bn_act_pool", "sehip_unet_bn_bwd_reduce", "sehip_unet_bn_bwd_apply",
            "sehip_unet_mask_fwd", "sehip_unet_mask_bwd", "sehip_unet_bn_finalize"} == set(names)
    for n in names:
        assert hasattr(lib, n), n                                     # exported
        assert n in _lib._PROTOS, n                                   # prototyped
    assert sorted(n for n in _lib._PROTOS if n.startswith("sehip_unet_")) == names     # ... and nothing prototyped that is not declared
    # argument validation happens before any launch: safe without a GPU
    nod = (0, 0, None, 0, 0, 1.0)
    assert lib.sehip_unet_bn_act(None, None, 100, 16, *nod, None, None) != 0 and b"null pointer" in lib.sehip_last_error()
    assert lib.sehip_unet_bn_act(None, None, 100, 24, *nod, None, None) != 0 and b"power of two" in lib.sehip_last_error()
    assert lib.sehip_unet_bn_act(None, None, 1 << 29, 16, *nod, None, None) != 0 and b"2^32 elements" in lib.sehip_last_error()
    assert lib.sehip_unet_bn_act(None, None, 100, 16, 0, 0, None, 0, 1 << 23, 2.0, None, None) != 0 and b"step counter" in lib.sehip_last_error()
    assert lib.sehip_unet_bn_act_pool(None, None, 2, 1, 8, 16, *nod, None, None, None) != 0 and b"one pooling window" in lib.sehip_last_error()
    assert lib.sehip_unet_bn_bwd_reduce(None, None, None, None, 2, 4, 4, 16, *nod, None, None) != 0 and b"null pointer" in lib.sehip_last_error()
    assert lib.sehip_unet_bn_bwd_apply(None, None, None, None, None, 2, 4, 4, 12, *nod, None, None) != 0
    assert lib.sehip_unet_features(None, 2, 3, 5, 5, 16, None, None) != 0 and b"rounded up" in lib.sehip_last_error()
    assert lib.sehip_unet_mask_fwd(None, None, None, 2, 3, 5, 5, 8, None, None) != 0 and b"null pointer" in lib.sehip_last_error()
    assert lib.sehip_unet_bn_finalize(None, None, None, None, None, None, None, 100, 8, 9, 1e-5, 0.1, 1, None, None) != 0 and b"Cr=9" in lib.sehip_last_error()
    with pytest.raises(_lib.SehipError):
        _lib.call("sehip_unet_mask_bwd", None, None, 2, 1, 5, 5, 8, None, None)


def _emulate(st, p, flat, srcs, T, Fq):
    """the engine's product p on one item, from the plan's own tables: srcs [T_s][F_s][C] per source -> one array per destination.
    Chunk table: (source, frame offset, row offset, channel offset) per 8 columns of K, source position (t tmul + frame offset,
    f fmul + row offset), zero outside the source; column table: (destination, first column, valid columns) per 4 outputs; a scatter
    product writes row (t, f) to (2 t + toff, 2 f + fadd)."""
    kt = st.ktab[p.kt_off:p.kt_off + p.K // 8]
    A = np.zeros((T, Fq, p.K))
    for c, (s, toff, foff, coff) in enumerate(kt):
        if s < 0:
            continue
        for t in range(T):
            for f in range(Fq):
                tt, ff = t * p.stride[0] + toff, f * p.stride[1] + foff
                if 0 <= tt < srcs[s].shape[0] and 0 <= ff < srcs[s].shape[1]:
                    A[t, f, 8 * c:8 * c + 8] = srcs[s][tt, ff, coff:coff + 8]
    w = st.wtab[p.w_off:p.w_off + p.Npad * p.K].reshape(p.Npad, p.K)
    out = A @ np.where(w >= 0, flat[np.maximum(w, 0) >> 1], 0.0).T
    if p.b_off is not None:
        b = st.btab[p.b_off:p.b_off + p.Npad, 0]
        out = out + np.where(b >= 0, flat[np.maximum(b, 0) >> 1], 0.0)
    dsts = [np.zeros((T, Fq, c)) for _, c in p.dsts]
    for g, (d, coff, nvalid, _) in enumerate(st.ntab[p.nt_off:p.nt_off + p.Npad // 4]):
        dsts[d][:, :, coff:coff + nvalid] = out[:, :, 4 * g:4 * g + nvalid]
    return dsts


def test_products_reproduce_the_convolutions():
    """every kind of product of the plan, emulated on the host from its packing / chunk / column tables, against F.conv2d and
    F.conv_transpose2d: the 3x3 convolution with padded input channels, the two-source decoder convolution and its two-destination input
    gradient, the four parity classes of the transposed convolution and the product that gathers them back"""
    from sehip import plan_unet as P
    st = P.UNetStatic(P.UNetConfig(unet_channels=2, unet_layer=2))
    L = st.layout
    rng = np.random.default_rng(0)
    flat = rng.standard_normal(L.n_params)
    get = lambda n: torch.from_numpy(flat[L.param_off[n][0]:L.param_off[n][0] + int(np.prod(L.param_off[n][1]))].reshape(L.param_off[n][1]))
    T, Fq = 5, 4
    rnd = lambda c: torch.from_numpy(rng.standard_normal((1, c, Fq, T)))             # [1, C, F, T] as the reference lays it out
    cl = lambda x: x[0].permute(2, 1, 0).numpy()                                    # -> [T][F][C]
    ncl = lambda a: torch.from_numpy(a).permute(2, 1, 0)[None]
    # the first convolution: 2 real channels stored 8 wide
    amp = rnd(2)
    amp8 = np.concatenate([cl(amp), np.zeros((T, Fq, 6))], -1)
    got, = _emulate(st, st.prods["e0.c1"], flat, [amp8], T, Fq)
    assert np.allclose(ncl(got), F.conv2d(amp, get("encoder.0.maxpool_conv.0.double_conv.0.weight"), padding=1), atol=1e-9)
    # decoder 1: up (16 channels) | skip (16) -> 16, and its input gradient to the two halves
    pre = "decoder.1.conv.double_conv."
    up, skip = rnd(16), rnd(16)
    got, = _emulate(st, st.prods["d1.c1"], flat, [cl(up), cl(skip)], T, Fq)
    assert np.allclose(ncl(got), F.conv2d(torch.cat([up, skip], 1), get(pre + "0.weight"), padding=1), atol=1e-9)
    dy = rnd(16)
    want = F.conv_transpose2d(dy, get(pre + "0.weight"), padding=1)
    d_up, d_skip = _emulate(st, st.prods["d1.c1.dg"], flat, [cl(dy)], T, Fq)
    assert np.allclose(ncl(d_up), want[:, :16], atol=1e-9) and np.allclose(ncl(d_skip), want[:, 16:], atol=1e-9)
    assert [b for b, _ in st.prods["d1.c1.dg"].dsts] == ["d1.dup", "ds0"] and st.prods["d1.c1"].srcs == ["d1.up", "p0"]
    assert st.prods["e1.c1.dg"].res == "ds0" and st.prods["m.c1.dg"].res == "ds1" and "e0.c1.dg" not in st.prods
    # the second convolution of a block and its input gradient
    z1 = rnd(16)
    got, = _emulate(st, st.prods["d1.c2"], flat, [cl(z1)], T, Fq)
    assert np.allclose(ncl(got), F.conv2d(z1, get(pre + "3.weight"), padding=1), atol=1e-9)
    got, = _emulate(st, st.prods["d1.c2.dg"], flat, [cl(dy)], T, Fq)
    assert np.allclose(ncl(got), F.conv_transpose2d(dy, get(pre + "3.weight"), padding=1), atol=1e-9)
    # the transposed convolution of decoder 1 (32 -> 16): four parity classes, scattered
    x = rnd(32)
    want = F.conv_transpose2d(x, get("decoder.1.up.weight"), get("decoder.1.up.bias"), stride=2)       # [1, 16, 2 F, 2 T]
    for a in range(2):
        for b in range(2):
            p = st.prods[f"d1.up{a}{b}"]
            got, = _emulate(st, p, flat, [cl(x)], T, Fq)
            assert p.scatter == (a, b) and np.allclose(ncl(got), want[:, :, b::2, a::2], atol=1e-9)
    dup = torch.from_numpy(rng.standard_normal((1, 16, 2 * Fq + 1, 2 * T + 1)))      # a buffer with a pad row and a pad column
    got, = _emulate(st, st.prods["d1.up.dg"], flat, [cl(dup)], T, Fq)
    want = F.conv2d(dup[:, :, :2 * Fq, :2 * T], get("decoder.1.up.weight"), stride=2)
    assert np.allclose(ncl(got), want, atol=1e-9)
    # the head: [up (8) | amp (2 of 8)] -> 2 of 8; its input gradient goes to the up half only
    pre = "outconv.conv.double_conv."
    u8 = rnd(8)
    got, = _emulate(st, st.prods["o.c1"], flat, [cl(u8), amp8], T, Fq)
    want = F.conv2d(torch.cat([u8, amp], 1), get(pre + "0.weight"), padding=1)
    assert np.allclose(ncl(got)[:, :2], want, atol=1e-9) and not got[:, :, 2:].any()
    dy2 = np.concatenate([cl(rnd(2)), np.zeros((T, Fq, 6))], -1)
    got, = _emulate(st, st.prods["o.c1.dg"], flat, [dy2], T, Fq)
    want = F.conv_transpose2d(ncl(dy2)[:, :2], get(pre + "0.weight"), padding=1)
    assert np.allclose(ncl(got), want[:, :8], atol=1e-9) and [b for b, _ in st.prods["o.c1.dg"].dsts] == ["o.dup"]


@pytest.mark.parametrize("tag", TAGS)
def test_plan_on_the_emulated_c_abi(tag, monkeypatch):
    """the plan's own forward() / backward() on the CPU, every library call answered by tests/unet_cabi_emulator.py (numpy on the raw
    pointers, from the documented semantics): buffer wiring, pointer offsets, bound tables and launch order against the reference's
    vectors, with the bound the GPU chain test uses (2 x the deviation of the bf16-storage restatement)"""
    from sehip import plan_unet as P, workspace as W, SehipError
    from sehip.model import UNet
    from unet_cabi_emulator import Emulator
    fx = fixture(tag)
    emu = Emulator()
    for mod in (P, W):            # (gemm() and wgrad() launch from the workspace base)
        monkeypatch.setattr(mod, "call", emu)
        monkeypatch.setattr(mod, "stream", lambda: None)
    model = UNet(**model_kw(tag), unet_dropout=0.0)
    model.load_state_dict(fx["sd"])
    cpu = torch.device("cpu")
    R_, _, Fq, T, _ = fx["mix"].shape
    ws = P.UNetWorkspace(model.static, P.UNetDeviceTables(model.static, cpu), R_, Fq, T, cpu, guard=64)
    est = ws.forward(fx["mix"].contiguous(), model._flat, model._bflat, model._nbt, training=True).clone()
    grads = torch.zeros_like(model._flat)
    ws.backward(fx["G"].contiguous(), model._flat, grads)
    assert ws.guards_intact() == []
    L = model.static.layout
    got = {k: grads[L.param_off[k][0]:L.param_off[k][0] + fx["sd"][k].numel()].view(fx["sd"][k].shape) for k in L.param_names}
    gs, ests = R.fixed_g_grads(fx["sd"], fx["mix"], fx["G"], sim=R.Bf16Sim, **model_kw(tag))
    dev, sim_dev = rel(est, fx["est"]), rel(ests, fx["est"])
    (glob, _), (sglob, _) = grad_dev(got, fx["gradG"], list(got)), grad_dev(gs, fx["gradG"], list(gs))
    print(f"UNet {tag} plan on the emulated C ABI: est {dev:.3e} (restatement {sim_dev:.3e}), gradients {glob:.4f} (restatement {sglob:.4f})")
    assert dev < 2 * sim_dev and glob < 2 * sglob
    # running statistics, all layers together (the head's layers have unet_channels values: too few for two draws of the rounding noise
    # to agree within 2 x), with the same bound
    after, run_sim = model.state_dict(), {}
    R.unet_forward(fx["sd"], fx["mix"], sim=R.Bf16Sim, running=run_sim, **model_kw(tag))
    assert all(int(after[k]) == 1 for k in fx["run"] if k.endswith("num_batches_tracked"))
    for kind in ("running_mean", "running_var"):
        cat = lambda d: torch.cat([d[k].double().reshape(-1) for k in fx["run"] if k.endswith(kind)])
        assert rel(cat(after), cat(fx["run"])) < 2 * rel(cat(run_sim), cat(fx["run"])), kind
    n = model.cfg.L
    nconv, nup = 2 * (2 * n + 2), n                                   # double convolutions: n encoders, middle, n decoders, head; transposed: n - 1 + head
    assert emu.calls.count("sehip_gemm") == nconv + 4 * nup + (nconv - 1) + nup      # forward + input gradients (none from the first block: amp is data)
    assert emu.calls.count("sehip_wgrad") == nconv + 4 * nup and emu.calls.count("sehip_unet_bn_act_pool") == n
    assert emu.calls[-1] == "sehip_unpack_grad1" and "sehip_rsm_counter_next" not in emu.calls
    # eval mode: running statistics, forward only
    ev = ws.forward(fx["mix"].contiguous(), model._flat, model._bflat, model._nbt, training=False).clone()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    assert rel(ev, R.unet_forward(sd, fx["mix"], training=False, **model_kw(tag))) < 2 * sim_dev
    with pytest.raises(SehipError, match="eval mode"):
        ws.backward(fx["G"].contiguous(), model._flat, grads)


def test_plan_dropout_on_the_emulated_c_abi(monkeypatch):
    """dropout at 0.5 through the plan on the emulated C ABI against the restatement under the twin's masks: the two sites' keys, the
    channels-last index, the pooled backward under dropout and the counter's hand-over"""
    from sehip import plan_unet as P, workspace as W
    from sehip.model import UNet
    from unet_cabi_emulator import Emulator
    tag = "unet_l2_c2"
    fx = fixture(tag)
    emu = Emulator()
    for mod in (P, W):
        monkeypatch.setattr(mod, "call", emu)
        monkeypatch.setattr(mod, "stream", lambda: None)
    model = UNet(**model_kw(tag))
    model.load_state_dict(fx["sd"])
    cpu = torch.device("cpu")
    R_, _, Fq, T, _ = fx["mix"].shape
    ws = P.UNetWorkspace(model.static, P.UNetDeviceTables(model.static, cpu), R_, Fq, T, cpu)
    counter = torch.tensor([5], dtype=torch.int64)
    est = ws.forward(fx["mix"].contiguous(), model._flat, model._bflat, model._nbt, seed=model.dropout_seed, counter=counter).clone()
    grads = torch.zeros_like(model._flat)
    ws.backward(fx["G"].contiguous(), model._flat, grads)
    assert int(counter) == 6 and int(ws.ctr_used[0]) == 5
    L = model.static.layout
    got = {k: grads[L.param_off[k][0]:L.param_off[k][0] + fx["sd"][k].numel()].view(fx["sd"][k].shape) for k in L.param_names}
    drop = dict(seed=model.dropout_seed, counter=5, p=0.5)
    g32, e32 = R.fixed_g_grads(fx["sd"], fx["mix"], fx["G"], drop=drop, **model_kw(tag))
    gs, ests = R.fixed_g_grads(fx["sd"], fx["mix"], fx["G"], sim=R.Bf16Sim, drop=drop, **model_kw(tag))
    dev, sim_dev = rel(est, e32), rel(ests, e32)
    (glob, _), (sglob, _) = grad_dev(got, g32, list(got)), grad_dev(gs, g32, list(gs))
    print(f"UNet {tag} dropout 0.5 on the emulated C ABI: est {dev:.3e} (restatement {sim_dev:.3e}), gradients {glob:.4f} (restatement {sglob:.4f})")
    assert dev < 2 * sim_dev and glob < 2 * sglob
    assert rel(e32, fx["est"]) > 10 * sim_dev                         # ... and the masks did something
