"""GPU: the U-Net on the power spectrogram (`unet`) on the HIP path (csrc/unet.hip + the implicit-GEMM engine, sehip/plan_unet.py).

1. op-local: after one forward + backward pass of each fixture, every layer keeping its buffers, the workspace is copied back and EVERY
   launch of the plan is recomputed in float64 from the operands the kernel itself read (tests/unet_cabi_emulator.py in check mode: the
   plan's own launch list, so nothing is skipped): stored tensors, fp32 sums against the sum of the absolute addends, argmax codes;
2. the whole chain against vectors of the imported reference (tests/golden/unet_*.npz): the bound is 2 x the deviation of the
   bf16-storage restatement (tests/unet_ref.py under Bf16Sim) from the same vectors, computed on the CPU in the same test: est, every
   tap the HIP path stores (the mask itself is applied on the fly and covered through est), loss, gradients of <est, G>, two Adam
   steps, running statistics;
3. dropout at 0.5: the device's mask against the twin at both sites, est and gradients against the restatement under the twin's masks,
   op-local under dropout, seeds, eval;
4. edges with guard bands around every output of the new kernels, the smallest legal network input, the forward-time refusals;
5. the shipped width once; 6. three Solver steps through the registry and evaluate().
Gradient parity is gated on the fixtures only (Wave-U-Net's reason: the deep levels normalise over few values per channel).

Measured on an MI355X (every test prints what it gates), fixtures l1_c1 / l2_c2:
  op-local   39 / 61 stored tensors worst rms 2.00e-3 / 1.81e-3 (gate 1.8e-3, or its margin over the rms of the float64 result rounded once:
             the 2.00e-3 tensor has 36 rows and is correctly rounded), worst element 0.992 / 0.995 of a bf16 rounding step; 28 / 40 fp32 sums
             2.0e-6 / 1.1e-6 of the absolute addends (gate 2e-5); argmax codes and coefficient records equal to the float64 oracle's
  chain      est 6.221e-3 / 5.370e-3 against the restatement's 6.221e-3 / 5.392e-3; taps on the restatement's deviation to three digits
             (1.5e-3 .. 1.9e-2); mse loss 3.66e-5 / 4.26e-5 off (restatement 3.66e-5 / 4.55e-5); gradients of <est, G> 0.1468 / 0.2128 global
             (restatement 0.1470 / 0.2675); running statistics 2.0e-3 / 1.9e-3 and 1.1e-4 / 5.4e-5, the restatement's
  Adam x 2   second loss 1.48e-3 / 1.14e-4 off (restatement 1.18e-3 / 8.3e-5); parameter updates 0.484 / 0.486 (restatement 0.488 / 0.504)
  dropout    l2_c2 at 0.5 under the twin's masks: est 5.169e-3 (restatement 5.177e-3), gradients 0.1354 (0.1356); op-local 1.77e-3 / 0.995 /
             1.1e-6; eval 5.551e-3 (the restatement's); eval against the reference's eval vectors 3.00e-3 / 5.64e-3 (the restatement's)
  edges      spectrum kernels 1.66e-3 rms, 0.990 of a rounding step, out 1.5e-7; pool kernels 1.57e-3 .. 1.89e-3 (12 .. 189 rows), 0.98;
             the smallest legal input [2, 1, 4, 4, 2] at unet_layer=2: 2.77e-3 on an 8-row tensor that is correctly rounded, 0.993
  shipped    [2, 1, 257, 65, 2], dropout 0.5: est 1.024e-2 (restatement 1.038e-2, gate 3 x); gradients, not gated: 0.257 global / 0.486 worst
             large tensor (restatement 0.259 / 0.491)
  Solver     3.98e-6 -> 3.59e-6 -> 3.45e-6 in three steps at batch 4; the step at [32, 1, 16384] takes 3.10 ms (profiles/unet_step.json)
The same plan on an emulated C ABI and the restatement are gated on the CPU in tests/test_unet_host.py.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import unet_ref as R
from ctn_variants_ref import grad_dev
from util import rel_err

pytestmark = pytest.mark.gpu

OUT_TOL = 1.8e-3              # rms of ONE round-to-nearest bf16 rounding is 1.65e-3 (tests/test_gpu_convtasnet_variants.py)
ONE_ROUNDING_RMS = 1.65e-3
ULP_TOL = 2.0 ** -8 * 1.02
SUM_TOL = 2e-5                # fp32 sums, relative to the sum of the absolute addends
GUARD = 256
TAGS = sorted(R.FIXTURES)
fixture, model_kw = R.fixture, R.model_kw
_RUN, _SIM = {}, {}


def nchw(buf, c=None):
    """workspace buffer [R][T][F][C] bf16 -> float64 [R, C, F, T] on the host (the first c channels)"""
    t = buf.t.double().permute(0, 3, 2, 1).cpu()
    return t if c is None else t[:, :c]


def run_model(kw, sd, mix, G, seed=None):
    """one forward + backward pass under the upstream gradient G, canary bands around every workspace buffer"""
    from sehip.model import UNet
    if seed is not None:
        torch.manual_seed(seed)
    model = UNet(**kw)
    model.load_state_dict(sd)
    model._ws_guard = GUARD
    model.cuda().train()
    est = model(mix.cuda())
    (est * G.cuda()).sum().backward()
    torch.cuda.synchronize()
    ws = model.workspace(mix.shape[0], mix.shape[2], mix.shape[3])
    assert ws.guards_intact() == []
    grads = {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters()}
    return model, ws, est.detach().cpu(), grads


def run_kept(tag):
    """the fixture's pass without dropout (what the reference's vectors were taken with), shared by the tests"""
    if tag not in _RUN:
        fx = fixture(tag)
        _RUN[tag] = run_model(dict(unet_dropout=0.0, **model_kw(tag)), fx["sd"], fx["mix"], fx["G"])
    return _RUN[tag]


def sim_run(tag):
    """the restatement with bf16 round-trips at the HIP path's storage points, on the CPU: (gradients of <est, G>, est, taps, running)"""
    if tag not in _SIM:
        fx = fixture(tag)
        taps, run = {}, {}
        gs, ests = R.fixed_g_grads(fx["sd"], fx["mix"], fx["G"], sim=R.Bf16Sim, taps=taps, running=run, **model_kw(tag))
        _SIM[tag] = (gs, ests, {k: v.detach() for k, v in taps.items()}, run)
    return _SIM[tag]


# ------------------------------------------------------------------------------------------------------------------
# 1. op-local
# ------------------------------------------------------------------------------------------------------------------
def replay(model, ws, sd, mix, G):
    """the findings of the check-mode emulator over a host copy of the workspace: the plan's own forward() / backward() launch list, every
    call recomputed in float64 from what the device left in its operands"""
    from sehip import plan_unet as P, workspace as W
    from sehip.model import UNet
    from unet_cabi_emulator import Emulator
    cfg = model.cfg
    host = UNet(unet_channels=cfg.uc, unet_layer=cfg.L, unet_dropout=cfg.p)
    host.load_state_dict(sd)                                          # parameters and running statistics as they were BEFORE the pass
    cpu = torch.device("cpu")
    tables = P.UNetDeviceTables(model.static, cpu)
    tables.wpack.copy_(ws.tb.wpack.cpu()); tables.bpack.copy_(ws.tb.bpack.cpu())
    cws = P.UNetWorkspace(model.static, tables, ws.R, ws.F, ws.T, cpu)
    for k, b in ws.bufs.items():
        cws.bufs[k].t.copy_(b.t.cpu())
    for name in ("code", "coef", "bcoef", "part", "bpart"):
        for k, t in getattr(ws, name).items():
            getattr(cws, name)[k].copy_(t.cpu())
    cws.gpack.copy_(ws.gpack.cpu()); cws.out.copy_(ws.out.cpu()); cws.ctr_used.copy_(ws.ctr_used.cpu())
    emu = Emulator(check=True, gpack=(cws.gpack.data_ptr(), cws.gpack.numel()))
    saved = (P.call, P.stream, W.call, W.stream)
    P.call = W.call = emu
    P.stream = W.stream = lambda: None
    try:
        cws.forward(mix.contiguous(), host._flat, host._bflat, host._nbt, seed=model.dropout_seed, counter=torch.zeros(1, dtype=torch.int64))
        cws.backward(G.contiguous(), host._flat, model.flat_grads.detach().cpu().clone())
        emu.finish()
    finally:
        P.call, P.stream, W.call, W.stream = saved
    return emu.findings


def gate_findings(what, findings):
    """the project's gates on every finding; returns the worst of each kind.  Stored tensors: the element-wise gate is a property of one
    rounding and holds at any size; the rms gate is a statistic, so (as tests/test_gpu_wavunet.py check_small does) it keeps its margin,
    OUT_TOL / 1.65e-3, over the rms this very tensor has when the float64 result is rounded once and correctly -- a bound from the
    float64 result alone -- and is never below OUT_TOL."""
    worst = dict(rms=0.0, ulp=0.0, sum=0.0, stored=0, sums=0, exact=0)
    for f in findings:
        if f["kind"] == "stored":
            bound = OUT_TOL * max(1.0, f["ideal"] / ONE_ROUNDING_RMS)
            assert f["rms"] < bound and f["ulp"] < ULP_TOL, (what, f, bound)
            worst["rms"], worst["ulp"], worst["stored"] = max(worst["rms"], f["rms"]), max(worst["ulp"], f["ulp"]), worst["stored"] + 1
        elif f["kind"] == "sum":
            assert f["err"] < SUM_TOL, (what, f)
            worst["sum"], worst["sums"] = max(worst["sum"], f["err"]), worst["sums"] + 1
        else:
            assert f["bad"] == 0, (what, f)
            worst["exact"] += 1
    return worst


def report(w):
    return (f"{w['stored']} stored tensors worst rms {w['rms']:.2e}, worst element {w['ulp'] / 2 ** -8:.3f} bf16 roundings; {w['sums']} fp32 sums "
            f"{w['sum']:.1e} of the absolute addends; {w['exact']} exact checks (argmax codes, coefficient records)")


@pytest.mark.parametrize("tag", TAGS)
def test_op_local(tag):
    fx = fixture(tag)
    model, ws, est, _ = run_kept(tag)
    findings = replay(model, ws, fx["sd"], fx["mix"], fx["G"])
    w = gate_findings(tag, findings)
    n = model.cfg.L
    assert sum("argmax codes" in f["what"] for f in findings) == n and w["stored"] > 10 * (n + 1)
    assert torch.equal(ws.out.cpu(), est)
    print(f"UNet {tag} op-local: {report(w)}")


# ------------------------------------------------------------------------------------------------------------------
# 2. whole chain against the reference's vectors
# ------------------------------------------------------------------------------------------------------------------
def gpu_taps(model, ws):
    n, uc, b = model.cfg.L, model.cfg.uc, ws.bufs
    taps = {"amp": nchw(b["amp"], uc), "middle": nchw(b["m.z2"]), "upo": nchw(b["o.up"])}
    taps.update({f"enc{l}": nchw(b[f"p{l}"]) for l in range(n)})
    taps.update({f"dec{i}": nchw(b[f"d{i}.z2"]) for i in range(n)})
    taps.update({f"up{i}": nchw(b[f"d{i}.up"]) for i in range(1, n)})
    return taps


@pytest.mark.parametrize("tag", TAGS)
def test_whole_chain_vs_reference_vectors(tag):
    fx = fixture(tag)
    model, ws, est, grads = run_kept(tag)
    gs, ests, taps, _ = sim_run(tag)
    got = gpu_taps(model, ws)
    assert sorted(got) == sorted(k for k in fx["tap"] if k != "head")     # the mask is never stored: covered through est
    for k in sorted(got):
        dev, sim_dev = rel_err(got[k], fx["tap"][k]), rel_err(taps[k], fx["tap"][k])
        print(f"UNet {tag} tap.{k}: HIP {dev:.3e}, bf16-storage restatement {sim_dev:.3e}")
        assert dev < 2 * sim_dev, (k, dev, sim_dev)
    dev, sim_dev = rel_err(est, fx["est"]), rel_err(ests, fx["est"])
    print(f"UNet {tag} est: HIP {dev:.3e}, bf16-storage restatement {sim_dev:.3e}")
    assert dev < 2 * sim_dev, (dev, sim_dev)
    loss, loss_sim = float(F.mse_loss(est, fx["target"])), float(F.mse_loss(ests, fx["target"]))
    print(f"UNet {tag} mse loss: HIP {loss:.6e}, reference {fx['loss']:.6e}, restatement {loss_sim:.6e}")
    assert abs(loss - fx["loss"]) < 2 * abs(loss_sim - fx["loss"]), (loss, loss_sim, fx["loss"])
    names = list(grads)
    (glob, worst), (sglob, sworst) = grad_dev(grads, fx["gradG"], names), grad_dev(gs, fx["gradG"], names)
    print(f"UNet {tag} gradients of <est, G>: HIP global {glob:.4f} (worst large tensor {worst:.4f}), bf16-storage restatement {sglob:.4f} ({sworst:.4f})")
    assert glob < 2 * sglob, (glob, sglob)
    # running statistics after the one pass, all layers together (the head's layers hold unet_channels values each)
    after = {k: v.cpu() for k, v in model.state_dict().items()}
    run_sim = sim_run(tag)[3]
    assert all(int(after[k]) == 1 for k in fx["run"] if k.endswith("num_batches_tracked"))
    for kind in ("running_mean", "running_var"):
        cat = lambda d: torch.cat([d[k].double().reshape(-1) for k in fx["run"] if k.endswith(kind)])
        dev, sim_dev = rel_err(cat(after), cat(fx["run"])), rel_err(cat(run_sim), cat(fx["run"]))
        print(f"UNet {tag} {kind}: HIP {dev:.3e}, bf16-storage restatement {sim_dev:.3e}")
        assert dev < 2 * sim_dev, (kind, dev, sim_dev)


@pytest.mark.parametrize("tag", TAGS)
def test_two_adam_steps_vs_reference_vectors(tag):
    from sehip import distrib, utils
    from sehip.loss import mse_loss
    from sehip.model import UNet
    fx = fixture(tag)
    names = R.param_names(fx["sd"])
    sim_losses, p = R.adam_steps(fx["sd"], fx["mix"], fx["target"], sim=R.Bf16Sim, **model_kw(tag))
    model = UNet(unet_dropout=0.0, **model_kw(tag))
    model.load_state_dict(fx["sd"])
    model.cuda().train()
    hopt = distrib.get_optimizer(utils.dict2obj({"optim": "adam", "lr": 3e-4, "beta1": 0.9, "beta2": 0.999}), model)
    mix, tgt = fx["mix"].cuda(), fx["target"].cuda()
    losses = []
    for _ in range(2):
        loss = mse_loss(model(mix), tgt)
        hopt.zero_grad()
        loss.backward()
        hopt.clip_grad_norm_(5.0)
        hopt.step()
        losses.append(float(loss.detach()))
    torch.cuda.synchronize()
    sd = {k: v.cpu() for k, v in model.state_dict().items()}
    for i in range(2):
        ref = float(fx["adam_losses"][i])
        print(f"UNet {tag} two Adam steps, loss {i + 1}: HIP {losses[i]:.6e}, reference {ref:.6e}, restatement {sim_losses[i]:.6e}")
        assert abs(losses[i] - ref) < 2 * abs(sim_losses[i] - ref), (i, losses[i], sim_losses[i], ref)
    # the parameter UPDATES of the two steps (the parameters themselves agree to 1e-3 whatever the steps did)
    upd = lambda d: {k: d[k].detach().double() - fx["sd"][k].double() for k in names}
    (glob, _), (sglob, _) = grad_dev(upd(sd), upd(fx["adam"]), names), grad_dev(upd(p), upd(fx["adam"]), names)
    print(f"UNet {tag} two Adam steps: parameter updates HIP {glob:.4f}, bf16-storage restatement {sglob:.4f}")
    assert glob < 2 * sglob, (glob, sglob)
    assert all(int(sd[k]) == int(fx["adam"][k]) == 2 for k in fx["adam"] if k.endswith("num_batches_tracked"))
    for kind in ("running_mean", "running_var"):
        keys = [k for k in fx["adam"] if k.endswith(kind)]
        cat = lambda d: torch.cat([d[k].detach().double().reshape(-1) for k in keys])
        dev, sim_dev = rel_err(cat(sd), cat(fx["adam"])), rel_err(cat(p), cat(fx["adam"]))
        print(f"UNet {tag} two Adam steps: {kind} HIP {dev:.3e}, bf16-storage restatement {sim_dev:.3e}")
        assert dev < 2 * sim_dev, (kind, dev, sim_dev)


# ------------------------------------------------------------------------------------------------------------------
# 3. dropout
# ------------------------------------------------------------------------------------------------------------------
class Banded:
    """an output buffer of n elements between two sentinel-filled bands"""

    def __init__(self, n, dtype, fill=0):
        self.sentinel = 512 if dtype in (torch.int16, torch.int64) else 512.0
        self.full = torch.full((n + 2 * GUARD,), self.sentinel, dtype=dtype, device="cuda")
        self.view = self.full[GUARD:GUARD + n]
        self.view.fill_(fill)

    @property
    def ptr(self):
        return self.view.data_ptr()

    def intact(self):
        return bool((self.full[:GUARD] == self.sentinel).all()) and bool((self.full[-GUARD:] == self.sentinel).all())


class Both:
    """runs a library call on the device and then the check-mode emulator on host copies of the same arguments"""

    def __init__(self):
        from unet_cabi_emulator import Emulator
        self.host = {}
        self.emu = Emulator(check=True, gpack=(0, 0))
        self.outs = []

    def _host(self, a):
        t = a.view if isinstance(a, Banded) else a
        if id(a) not in self.host:
            self.host[id(a)] = t.cpu().clone()
        return self.host[id(a)]

    def __call__(self, name, *args):
        from sehip import _lib
        dev = [a.ptr if isinstance(a, Banded) else (a.data_ptr() if torch.is_tensor(a) else a) for a in args]
        _lib.call(name, *dev, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        self.outs += [a for a in args if isinstance(a, Banded)]
        for a in args:                                                 # what the call wrote has to reach the host copies
            if isinstance(a, Banded):
                self.host[id(a)] = a.view.cpu().clone()
        host = [self._host(a).data_ptr() if (isinstance(a, Banded) or torch.is_tensor(a)) else a for a in args]
        self.emu(name, *host, None)

    def finish(self, what):
        for o in self.outs:
            assert o.intact(), what
            assert bool(torch.isfinite(o.view.float()).all()), what         # (outputs start as NaN: every element was written)
        return gate_findings(what, self.emu.findings)


def device_counter(value):
    return torch.tensor([value, 0], dtype=torch.int32, device="cuda")


def test_device_mask_equals_twin_at_both_sites():
    """scale 0 / shift 1 turns the activation into the mask itself: bn_act (the middle block's site) writes 2 where it keeps and 0 where it
    drops; bn_act_pool (the last encoder block's site) writes 2 where any of the window's four is kept and codes the first kept one"""
    from sehip import _lib
    from sehip.plan_rnnmask import drop_threshold
    seed, counter, p = 0x1234567890ABCDEF, 7, 0.5
    thresh, scale = drop_threshold(p)
    st = torch.cuda.current_stream().cuda_stream
    R_, T, Fq, C = 3, 9, 7, 32
    rows = R_ * T * Fq
    y = torch.randn(rows, C).bfloat16().cuda()
    coef = torch.tensor([0.0, 1.0, 0.0, 1.0]).repeat(C, 1).cuda()
    ctr = device_counter(counter)
    args = (seed & 0xFFFFFFFF, seed >> 32, ctr.data_ptr())
    z = Banded(rows * C, torch.bfloat16)
    _lib.call("sehip_unet_bn_act", y.data_ptr(), coef.data_ptr(), rows, C, *args, R.DROP_MIDDLE, thresh, scale, z.ptr, st)
    zp, code = Banded(R_ * (T // 2) * (Fq // 2) * C, torch.bfloat16), Banded(R_ * (T // 2) * (Fq // 2) * C // 8, torch.int16)
    _lib.call("sehip_unet_bn_act_pool", y.data_ptr(), coef.data_ptr(), R_, T, Fq, C, *args, R.DROP_ENCODER, thresh, scale, zp.ptr, code.ptr, st)
    torch.cuda.synchronize()
    assert z.intact() and zp.intact() and code.intact()
    keep = R.drop_keep_mask(seed, counter, R.DROP_MIDDLE, rows * C, p)
    got = z.view.float().cpu().numpy()
    assert set(np.unique(got)) == {0.0, 2.0} and np.array_equal(got == 2.0, keep)
    keep = R.drop_keep_mask(seed, counter, R.DROP_ENCODER, rows * C, p).reshape(R_, T, Fq, C)[:, :T // 2 * 2, :Fq // 2 * 2]
    cand = np.stack([keep[:, dt::2, df::2] for df in (0, 1) for dt in (0, 1)], 0)       # code = 2 (F offset) + (T offset)
    want_code = np.where(cand.any(0), cand.argmax(0), 0)
    words = code.view.cpu().numpy().view(np.uint16).astype(np.int64).reshape(R_, T // 2, Fq // 2, C // 8, 1)
    got_code = ((words >> (2 * np.arange(8))) & 3).reshape(R_, T // 2, Fq // 2, C)
    assert np.array_equal(zp.view.float().cpu().numpy().reshape(want_code.shape) == 2.0, cand.any(0)) and np.array_equal(got_code, want_code)
    assert 0.4 < keep.mean() < 0.6 and (want_code > 0).mean() > 0.3


def test_dropout_half():
    from sehip.model import UNet
    tag = "unet_l2_c2"
    fx = fixture(tag)
    kw = dict(unet_dropout=0.5, **model_kw(tag))
    model, ws, est, grads = run_model(kw, fx["sd"], fx["mix"], fx["G"], seed=11)
    assert int(ws.ctr_used[0]) == 0 and int(model._drop_counter) == 1
    drop = dict(seed=model.dropout_seed, counter=0, p=0.5)
    # the middle block's output holds the mask: dropped elements are exact zeros (and LeakyReLU leaves no zero of its own here)
    keep = R.keep_nchw(drop, R.DROP_MIDDLE, tuple(nchw(ws.bufs["m.z2"]).shape))
    assert torch.equal(nchw(ws.bufs["m.z2"]) != 0, keep)
    g32, e32 = R.fixed_g_grads(fx["sd"], fx["mix"], fx["G"], drop=drop, **model_kw(tag))
    gs, ests = R.fixed_g_grads(fx["sd"], fx["mix"], fx["G"], sim=R.Bf16Sim, drop=drop, **model_kw(tag))
    dev, sim_dev = rel_err(est, e32), rel_err(ests, e32)
    (glob, worst), (sglob, sworst) = grad_dev(grads, g32, list(grads)), grad_dev(gs, g32, list(gs))
    print(f"UNet {tag} dropout 0.5 against the fp32 restatement under the twin's masks: est HIP {dev:.3e}, bf16-storage restatement {sim_dev:.3e}; "
          f"gradients HIP {glob:.4f} ({worst:.4f}), restatement {sglob:.4f} ({sworst:.4f})")
    assert dev < 2 * sim_dev and glob < 2 * sglob
    assert rel_err(e32, fx["est"]) > 10 * sim_dev                      # ... and the masks did something
    w = gate_findings(tag, replay(model, ws, fx["sd"], fx["mix"], fx["G"]))
    print(f"UNet {tag} dropout 0.5 op-local: {report(w)}")
    # the same seed gives the same bits, another seed gives others
    model2, _, est2, grads2 = run_model(kw, fx["sd"], fx["mix"], fx["G"], seed=11)
    assert model2.dropout_seed == model.dropout_seed and torch.equal(est2, est)
    assert grad_dev(grads2, grads, list(grads))[0] < 1e-4              # (the engine's weight gradients add with fp32 atomics)
    model3, _, est3, _ = run_model(kw, fx["sd"], fx["mix"], fx["G"], seed=12)
    assert model3.dropout_seed != model.dropout_seed and not torch.equal(est3, est)
    second = model(fx["mix"].cuda()).detach().cpu()                    # the next step draws new masks
    assert int(model._drop_counter) == 2 and not torch.equal(second, est)
    # eval drops nothing: the running statistics, no masks, the same bits at any counter
    sd = {k: v.cpu() for k, v in model.state_dict().items()}
    model.eval()
    with torch.no_grad():
        ev, ev2 = model(fx["mix"].cuda()).cpu(), model(fx["mix"].cuda()).cpu()
        ref = R.unet_forward(sd, fx["mix"], training=False, **model_kw(tag))
        sim = R.unet_forward(sd, fx["mix"], training=False, sim=R.Bf16Sim, **model_kw(tag))
    dev, sim_dev = rel_err(ev, ref), rel_err(sim, ref)
    print(f"UNet {tag} eval: HIP {dev:.3e}, bf16-storage restatement {sim_dev:.3e}")
    assert dev < 2 * sim_dev and torch.equal(ev, ev2) and int(model._drop_counter) == 2
    after = {k: v.cpu() for k, v in model.state_dict().items()}
    assert all(torch.equal(after[k], sd[k]) for k in sd)               # eval touches neither statistics nor counters
    from sehip import SehipError
    out = model(fx["mix"].cuda())
    with pytest.raises(SehipError, match="eval mode"):
        out.sum().backward()


@pytest.mark.parametrize("tag", TAGS)
def test_eval_against_reference_vector(tag):
    from sehip.model import UNet
    fx = fixture(tag)
    sd = dict(fx["sd"])
    sd.update(fx["run"])
    model = UNet(**model_kw(tag))
    model.load_state_dict(sd)
    model.cuda().eval()
    with torch.no_grad():
        ev = model(fx["mix"].cuda()).cpu()
        sim = R.unet_forward(sd, fx["mix"], training=False, sim=R.Bf16Sim, **model_kw(tag))
    dev, sim_dev = rel_err(ev, fx["est_eval"]), rel_err(sim, fx["est_eval"])
    print(f"UNet {tag} eval against the reference's eval output: HIP {dev:.3e}, bf16-storage restatement {sim_dev:.3e}")
    assert dev < 2 * sim_dev


# ------------------------------------------------------------------------------------------------------------------
# 4. edges
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 5, 3, 2), (2, 3, 37, 34, 2)])
def test_spectrum_kernels_at_the_edges(shape):
    """features / mask_fwd / mask_bwd one past a tile in both axes and below one tile, one and three channels: guard bands, padding
    channels exact zeros, values op-local"""
    R_, uc, Fq, T, _ = shape
    Cp = 8
    g = torch.Generator().manual_seed(Fq * 100 + T)
    spec, dout = torch.randn(*shape, generator=g).cuda(), torch.randn(*shape, generator=g).cuda()
    y = torch.randn(R_, T, Fq, Cp, generator=g).bfloat16().cuda()
    coef = torch.randn(Cp, 4, generator=g).cuda()
    n = R_ * T * Fq * Cp
    both = Both()
    amp, dm, out = Banded(n, torch.bfloat16, fill=float("nan")), Banded(n, torch.bfloat16, fill=float("nan")), Banded(spec.numel(), torch.float32, fill=float("nan"))
    both("sehip_unet_features", spec, R_, uc, Fq, T, Cp, amp)
    both("sehip_unet_mask_bwd", dout, spec, R_, uc, Fq, T, Cp, dm)
    both("sehip_unet_mask_fwd", y, coef, spec, R_, uc, Fq, T, Cp, out)
    w = both.finish(f"spectrum kernels {shape}")
    for o in (amp, dm):
        assert not bool(o.view.reshape(-1, Cp)[:, uc:].float().abs().sum())         # padding channels: written, exact zeros
    print(f"UNet spectrum kernels {shape}: guard bands intact; {report(w)}")


@pytest.mark.parametrize("C", [16, 32])
@pytest.mark.parametrize("Fq,T", [(2, 2), (5, 4), (4, 5), (9, 7)])
def test_pool_kernels_at_the_edges(Fq, T, C):
    """bn_act_pool and the pooled BatchNorm backward with planted ties and odd sizes: the codes follow the tie rule, an odd last row /
    column takes exact zero, guard bands; plain bn_act and its backward on the same tensor"""
    from sehip import _lib
    R_ = 3
    rows, rows2 = R_ * T * Fq, R_ * (T // 2) * (Fq // 2)
    g = torch.Generator().manual_seed(Fq * 1000 + T * 10 + C)
    y = torch.randint(-3, 4, (R_, T, Fq, C), generator=g).float()                    # seven distinct values: most windows hold a tie
    y[0, :2, :2, 0] = 1.0                                                           # four equal values: the first, code 0
    y[0, :2, :2, 1] = torch.tensor([[0.0, 2.0], [2.0, 2.0]])                        # [T offset][F offset]: first maximum at T 1, F 0 -> code 1
    y[0, :2, :2, 2] = torch.tensor([[0.0, 2.0], [0.0, 2.0]])                        # first maximum at T 0, F 1 -> code 2
    y = y.bfloat16().cuda()
    coef = torch.stack([torch.tensor([1.5, 0.25, 0.1, 0.8]), torch.tensor([-0.5, 0.0, -0.2, 1.1])] * (C // 2)).cuda()
    coef[0] = coef[1] = coef[2] = torch.tensor([1.0, 0.0, 0.0, 1.0])
    nod = (0, 0, None, 0, 0, 1.0)
    both = Both()
    zp, code = Banded(rows2 * C, torch.bfloat16, fill=float("nan")), Banded(rows2 * C // 8, torch.int16, fill=-1)
    both("sehip_unet_bn_act_pool", y, coef, R_, T, Fq, C, *nod, zp, code)
    z = Banded(rows * C, torch.bfloat16, fill=float("nan"))
    both("sehip_unet_bn_act", y, coef, rows, C, *nod, z)
    words = code.view.cpu().numpy().view(np.uint16).astype(np.int64).reshape(R_, T // 2, Fq // 2, C // 8, 1)
    cd = ((words >> (2 * np.arange(8))) & 3).reshape(R_, T // 2, Fq // 2, C)
    assert tuple(cd[0, 0, 0, :3]) == (0, 1, 2)
    # against F.max_pool2d on the activated tensor (channels with a negative scale order the values the other way round)
    to_nchw = lambda t, tt, ff: t.double().reshape(R_, tt, ff, C).permute(0, 3, 2, 1).cpu()
    want, idx = F.max_pool2d(to_nchw(z.view, T, Fq), 2, return_indices=True)
    assert torch.equal(to_nchw(zp.view, T // 2, Fq // 2), want)
    ff, tt = idx // T, idx % T
    assert torch.equal(torch.from_numpy(cd).permute(0, 3, 2, 1), 2 * (ff % 2) + (tt % 2))
    # backward: pooled form, then plain
    lib = _lib.lib()
    nfl = int(lib.sehip_wun_bn_scratch_floats(rows, C))
    dpool, dz = torch.randn(rows2, C, generator=g).bfloat16().cuda(), torch.randn(rows, C, generator=g).bfloat16().cuda()
    for k, (grad, cdbuf) in enumerate(((dpool, code.view), (dz, None))):
        part, bcoef, dy = Banded(nfl, torch.float32), Banded(4 * C, torch.float32), Banded(rows * C, torch.bfloat16, fill=float("nan"))
        sums = Banded(2 * C, torch.float32)
        both.emu.shadow, both.emu.shadow_abs = np.zeros(2 * C), np.zeros(2 * C)
        both("sehip_unet_bn_bwd_reduce", grad, cdbuf, y, coef, R_, T, Fq, C, *nod, part)
        _lib.call("sehip_wun_bn_bwd_finalize", part.ptr, coef.data_ptr(), rows, C, sums.ptr, sums.ptr + 4 * C, bcoef.ptr,
                  torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        hs, hb, hc = sums.view.cpu().clone(), bcoef.view.cpu().clone(), coef.cpu().clone()
        both.emu.gp_ptr, both.emu.gp_n = hs.data_ptr(), 2 * C
        both.emu("sehip_wun_bn_bwd_finalize", None, hc.data_ptr(), rows, C, hs.data_ptr(), hs.data_ptr() + 4 * C, hb.data_ptr(), None)
        both.emu.finish()
        both("sehip_unet_bn_bwd_apply", grad, cdbuf, y, coef, bcoef, R_, T, Fq, C, *nod, dy)
        assert sums.intact()
        if k == 0:
            # an odd last frame / row belongs to no window: its g is exact zero, so dy there is -gamma rstd (mean(g) + xhat mean(g xhat))
            d = dy.view.float().reshape(R_, T, Fq, C).cpu().double()
            kb, kc = bcoef.view.reshape(C, 4).cpu().double(), coef.cpu().double()
            xh = (y.double().cpu() - kc[:, 2]) * kc[:, 3]
            lone = kb[:, 0] * (0.0 - kb[:, 1] - xh * kb[:, 2])
            if T % 2:
                assert rel_err(d[:, -1], lone[:, -1]) < 4e-3
            if Fq % 2:
                assert rel_err(d[:, :, -1], lone[:, :, -1]) < 4e-3
    w = both.finish(f"pool kernels F={Fq} T={T} C={C}")
    print(f"UNet pool kernels F={Fq} T={T} C={C}: guard bands intact, ties as the rule says; {report(w)}")


def test_smallest_legal_input_and_refusals():
    from sehip import SehipError, plan_unet
    from sehip.model import UNet
    torch.manual_seed(2)
    model = UNet(1, unet_layer=2, unet_dropout=0.0)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    g = torch.Generator().manual_seed(3)
    mix = torch.randn(2, 1, 4, 4, 2, generator=g)
    G = torch.randn(2, 1, 4, 4, 2, generator=g)
    model, ws, est, grads = run_model(dict(unet_channels=1, unet_layer=2, unet_dropout=0.0), sd, mix, G)      # guard bands: run_model
    assert tuple(est.shape) == (2, 1, 4, 4, 2) and bool(torch.isfinite(est).all()) and all(bool(torch.isfinite(v).all()) for v in grads.values())
    assert ws.Tl == [4, 2, 1] and ws.Fl == [4, 2, 1]
    w = gate_findings("smallest input", replay(model, ws, sd, mix, G))
    print(f"UNet smallest legal input [2, 1, 4, 4, 2] at unet_layer=2 op-local: {report(w)}")
    calls, real = [], plan_unet.call
    plan_unet.call = lambda name, *a: (calls.append(name), real(name, *a))[1]
    try:
        for bad, msg in (((2, 1, 3, 4, 2), r"at least 2\^2 = 4"), ((2, 1, 4, 3, 2), r"at least 2\^2 = 4"), ((2, 2, 4, 4, 2), "unet_channels=1"),
                         ((2, 1, 4, 4), "expected")):
            with pytest.raises(SehipError, match=msg):
                model(torch.zeros(*bad).cuda())
    finally:
        plan_unet.call = real
    assert calls == []                                                # refused before any launch
    model.eval()
    out = model(mix.cuda())
    with pytest.raises(SehipError, match="eval mode"):
        out.sum().backward()


# ------------------------------------------------------------------------------------------------------------------
# 5. the shipped width
# ------------------------------------------------------------------------------------------------------------------
def test_shipped_width():
    from sehip.model import UNet
    kw = dict(unet_channels=1, unet_layer=4)
    torch.manual_seed(5)
    sd = {k: v.clone() for k, v in UNet(**kw).state_dict().items()}
    g = torch.Generator().manual_seed(6)
    mix = torch.randn(2, 1, 257, 65, 2, generator=g)
    G = torch.randn(2, 1, 257, 65, 2, generator=g) / mix.numel() ** 0.5
    model, ws, est, grads = run_model(kw, sd, mix, G, seed=5)
    assert bool(torch.isfinite(est).all()) and all(bool(torch.isfinite(v).all()) and float(v.norm()) > 0 for v in grads.values())
    assert all(int(v) == 1 for k, v in model.state_dict().items() if k.endswith("num_batches_tracked"))
    drop = dict(seed=model.dropout_seed, counter=0, p=0.5)
    g32, ref = R.fixed_g_grads(sd, mix, G, drop=drop, **kw)
    gs, sim = R.fixed_g_grads(sd, mix, G, sim=R.Bf16Sim, drop=drop, **kw)
    dev, sim_dev = rel_err(est, ref), rel_err(sim, ref)
    names = list(grads)
    gd, sgd = grad_dev(grads, g32, names), grad_dev(gs, g32, names)
    print(f"UNet shipped width [2, 1, 257, 65, 2], dropout 0.5 under the twin's masks: est HIP {dev:.3e}, bf16-storage restatement {sim_dev:.3e}; "
          f"gradients of <est, G> (not gated) HIP {gd[0]:.4f} / {gd[1]:.4f}, restatement {sgd[0]:.4f} / {sgd[1]:.4f}")
    assert dev < 3 * sim_dev, (dev, sim_dev)


# ------------------------------------------------------------------------------------------------------------------
# 6. Solver
# ------------------------------------------------------------------------------------------------------------------
def test_three_solver_steps_and_evaluate(tmp_path):
    """a `unet` config through the registry, as a user writes it: n_fft 512, hop 128, 1.024 s at 16 kHz, batch 4, mse, Adam, clip_grad 5"""
    from sehip.evaluate import evaluate
    from sehip.train import main
    from sehip.solver import ScalarLog
    from sehip.model import UNet
    from sehip.utils import dict2obj
    cfg = dict2obj({
        "seed": 10, "root": None, "ha": None,
        "model": {"name": "unet", "audio_channels": 1, "num_spk": 1, "sample_rate": 16000, "segment": 1.024, "n_fft": 512, "hop_length": 128,
                  "win_length": 512, "center": True, "unet_channels": 1, "unet_layer": 4, "bilinear": False, "drop_out": 0.5},
        "optim": {"optim": "adam", "lr": 3e-4, "beta1": 0.9, "beta2": 0.999, "loss": "mse", "clip_grad": 5, "pit": False, "load": False},
        "dset": {"name": "synthetic", "norm": None, "sample_rate": 16000},
        "solver": {"epochs": 1, "save_checkpoint_interval": 1000, "all_steps": True, "total_steps": 0, "patience": 0,
                   "root": str(tmp_path), "resume": None, "preloaded_model": None,
                   "validation": {"interval": 1000, "metric": "loss", "total_steps": 0}, "test": {"interval": 1000}},
    })
    g = torch.Generator().manual_seed(0)
    clean = 0.1 * torch.randn(4, 1, 1, 16384, generator=g)
    noisy = clean[:, 0] + 0.05 * torch.randn(4, 1, 16384, generator=g)
    batches = [(noisy, clean, [None], [None], ["x"], [0])] * 3
    log = ScalarLog()
    solver = main(cfg, return_solver=True, device="gpu", train_dataloader=batches, validation_dataloader=[batches[0]], writer=log)
    assert isinstance(solver.model, UNet) and solver.model.cfg.key() == (1, 4, 0.5)
    solver._run_one_epoch(0, 1, train=True)
    losses = [v for (t, v, _s) in log.scalars if t == "Train/Loss_step"]
    print("UNet Solver losses", losses)
    assert len(losses) == 3 and all(np.isfinite(losses)) and losses[2] < losses[0], losses
    assert solver.model.workspace(4, 257, 129).T == 129
    assert all(int(v) == 3 for k, v in solver.model.state_dict().items() if k.endswith("num_batches_tracked"))
    wav = 0.1 * torch.randn(2, 1, 16384 + 700, generator=g)
    y = evaluate(wav, solver.model, torch.device("cuda:0"), cfg)
    assert y.is_cuda and tuple(y.shape) == tuple(wav.shape) and bool(torch.isfinite(y).all())
