"""GPU: mel-rnn (sehip.model.MelRNN at n_mels = 0) on the HIP path (csrc/rnnmask.hip, sehip/plan_melrnn.py).  The sections and the gates
are those of tests/test_gpu_rnnmask.py.

1. op-local: after one forward + backward pass EVERY launch is recomputed in float64 from the operands the kernel itself read, taken back
   from the workspace -- for the recurrence every step from the device's own h(l - 1) and, backward, the device's own dG of the
   neighbouring step.  Gates: stored bf16 tensors <= 1.8e-3 rms and <= 2^-8 1.02 per element, fp32 sums <= 2e-5 of the sum of the
   absolute addends.
2. the whole chain against vectors of the imported reference (tests/golden/melrnn_*.npz): every bound is 2 x the deviation of the
   bf16-storage restatement (tests/melrnn_ref.py under Bf16Sim) from the same vectors, computed on the CPU in the same test; losses
   through loss_gate.
3. eval mode; 4. sehip_rsm_elman_fwd / _bwd called directly with two directions; 5. edges with guard bands; 6. three Solver steps through
   the registry and evaluate(); 7. the shipped width.
"""
import pytest
import torch

import melrnn_ref as R
from ctn_variants_ref import grad_dev
from test_gpu_rnnmask import Worst, all_zero, d64, shifted
from util import rel_err

pytestmark = pytest.mark.gpu

TAGS = sorted(R.FIXTURES)
_FX, _RUN, _SIM = {}, {}, {}


def fixture(tag):
    if tag not in _FX:
        _FX[tag] = R.load_fixture(tag)
    return _FX[tag]


def kw(tag, **over):
    d = dict(R.FIXTURES[tag]["kw"])
    d.update(over)
    return d


def run_model(model_kw, sd, x, G, guard=0, seed=None):
    """one training-mode forward + backward pass under the upstream gradient G: (model, workspace, est, gradients)"""
    from sehip.model import MelRNN
    if seed is not None:
        torch.manual_seed(seed)
    model = MelRNN(**model_kw)
    if sd is not None:
        model.load_state_dict(sd)
    model._ws_guard = guard
    model.cuda().train()
    est = model(x.cuda())
    (est * G.cuda()).sum().backward()
    torch.cuda.synchronize()
    ws = model.workspace(x.shape[0], x.shape[3])
    grads = {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters()}
    return model, ws, est.detach().cpu(), grads


def run_kept(tag):
    if tag not in _RUN:
        fx = fixture(tag)
        _RUN[tag] = run_model(kw(tag), fx["sd"], fx["input"], fx["G"])
    return _RUN[tag]


def sim_run(tag):
    """the restatement with bf16 round-trips at the HIP path's storage points, on the CPU: (gradients of <est, G>, est, taps, running)"""
    if tag not in _SIM:
        fx = fixture(tag)
        taps, run = {}, {}
        names = R.param_names(fx["sd"])
        p = {k: (v.clone().requires_grad_(True) if k in names else v.clone()) for k, v in fx["sd"].items()}
        est = R.melrnn_forward(p, fx["input"], sim=R.Bf16Sim, taps=taps, running=run, **kw(tag))
        (est * fx["G"]).sum().backward()
        _SIM[tag] = ({k: p[k].grad for k in names}, est.detach(), {k: v.detach() for k, v in taps.items()}, run)
    return _SIM[tag]


# ------------------------------------------------------------------------------------------------------------------
# 1. op-local: every launch from the operands it read
# ------------------------------------------------------------------------------------------------------------------
RNN_T = ("feat", "steps", "mask", "dpre", "bsteps")        # the recurrence and the transposing kernels (test 5)


def elman_fwd_local(w, what, pre, hs, st, whh, reverse=False):
    """pre, hs, st [T, L, H] float64 from the device, whh [H, H] (bf16 values): state against tanh(pre + h(l-1) W_hh^T) as an fp32 sum, hs
    against state as a stored bf16 tensor"""
    hp = shifted(hs, 1 if reverse else 0)
    w.fsum(f"state {what}", st, torch.tanh(pre + hp @ whh.t()), pre.abs() + hp.abs() @ whh.abs().t() + 1)
    w.stored(f"hs {what}", hs, st)


def elman_bwd_local(w, what, dG, dout, st, whh, reverse=False):
    """dG, dout, st [T, L, H]: dG against (dout + dG(l+1) W_hh)(1 - state^2) from the device's own neighbouring dG"""
    nxt = torch.zeros_like(dG)                              # dG of the step after l in forward order
    if reverse:
        nxt[:, 1:] = dG[:, :-1]
    else:
        nxt[:, :-1] = dG[:, 1:]
    w.stored(f"dG {what}", dG, (dout + nxt @ whh) * (1 - st * st))


def op_local(model, ws, sd_before, x, G, grads, after=None, only=None):
    """only: None = every launch; otherwise the names to check"""
    cfg, b = model.cfg, ws.bufs
    T, L, H, G4, GB, F = ws.T, ws.L, cfg.H, cfg.G, cfg.GB, cfg.F
    cell = cfg.rnn_type
    w = Worst()
    do = lambda name: only is None or name in only
    wb = lambda k: sd_before[k].bfloat16().double()
    x64, G64 = x.double(), G.double()
    buf = lambda name: d64(b[name]).reshape(T, L, -1)
    n = T * L
    # ---- features
    feat = buf("feat")
    if do("feat"):
        amp = (x64[..., 0] ** 2 - x64[..., 1] ** 2).abs().reshape(L, F, T).permute(2, 0, 1)
        w.stored("feat", feat[..., :F], amp)
        assert all_zero(feat[..., F:])
    # ---- layers
    xin = feat[..., :F]
    xins = []
    for k in range(cfg.rnn_layer):
        xins.append(xin)
        pre = d64(b[f"pre{k}"]).reshape(T, L, G4, H)
        hs, st = buf(f"hs{k}"), buf(f"state{k}")
        wih, whh = wb(f"rnn.weight_ih_l{k}"), wb(f"rnn.weight_hh_l{k}")
        if do("ih"):
            w.fsum(f"pre{k}", pre.reshape(T, L, G4 * H), xin @ wih.t(), xin.abs() @ wih.abs().t())
        if do("steps"):
            if cell == "rnn":
                elman_fwd_local(w, f"layer {k}", pre[:, :, 0], hs, st, whh)
            else:
                g = d64(b[f"gates{k}"]).reshape(T, L, 4, H)
                hp, sp = shifted(hs, 0), shifted(st, 0)
                a = (hp @ whh.t()).reshape(T, L, G4, H)
                aa = (hp.abs() @ whh.abs().t()).reshape(T, L, G4, H)
                if cell == "lstm":
                    z = pre + a
                    act = torch.stack([torch.sigmoid(z[:, :, 0]), torch.sigmoid(z[:, :, 1]), torch.tanh(z[:, :, 2]), torch.sigmoid(z[:, :, 3])], dim=2)
                    w.fsum(f"gates{k}", g, act, pre.abs() + aa + 1)
                    w.fsum(f"c{k}", st, g[:, :, 1] * sp + g[:, :, 0] * g[:, :, 2], (g[:, :, 1] * sp).abs() + (g[:, :, 0] * g[:, :, 2]).abs() + 1e-3)
                    w.stored(f"hs{k}", hs, g[:, :, 3] * torch.tanh(st))
                else:
                    w.fsum(f"r{k}", g[:, :, 0], torch.sigmoid(pre[:, :, 0] + a[:, :, 0]), pre[:, :, 0].abs() + aa[:, :, 0] + 1)
                    w.fsum(f"z{k}", g[:, :, 1], torch.sigmoid(pre[:, :, 1] + a[:, :, 1]), pre[:, :, 1].abs() + aa[:, :, 1] + 1)
                    w.fsum(f"an{k}", g[:, :, 3], a[:, :, 2], aa[:, :, 2] + 1e-3)
                    w.fsum(f"n{k}", g[:, :, 2], torch.tanh(pre[:, :, 2] + g[:, :, 0] * g[:, :, 3]), pre[:, :, 2].abs() + (g[:, :, 0] * g[:, :, 3]).abs() + 1)
                    w.fsum(f"h{k}", st, (1 - g[:, :, 1]) * g[:, :, 2] + g[:, :, 1] * sp, ((1 - g[:, :, 1]) * g[:, :, 2]).abs() + (g[:, :, 1] * sp).abs() + 1e-3)
                    w.stored(f"hs{k}", hs, st)
        xin = hs
    # ---- BatchNorm1d
    y, z = xin, buf("z")
    coef = d64(ws.coef)
    if do("bn"):
        mean, var = y.mean(dim=(0, 1)), y.var(dim=(0, 1), unbiased=False)
        w.fsum("bn mean", coef[:, 2] * n, mean * n, y.abs().sum(dim=(0, 1)))
        assert rel_err(coef[:, 3], 1 / torch.sqrt(var + R.EPS)) < 1e-5
        gam, bet = sd_before["batchnorm.weight"].double(), sd_before["batchnorm.bias"].double()
        assert rel_err(coef[:, 0], gam * coef[:, 3]) < 1e-6 and float((coef[:, 1] - (bet - coef[:, 2] * coef[:, 0])).abs().max()) < 1e-5
        if after is not None:
            assert rel_err(after["batchnorm.running_mean"], 0.9 * sd_before["batchnorm.running_mean"].double() + 0.1 * mean) < 1e-5
            assert rel_err(after["batchnorm.running_var"], 0.9 * sd_before["batchnorm.running_var"].double() + 0.1 * var * n / (n - 1)) < 1e-5
            assert int(after["batchnorm.num_batches_tracked"]) == int(sd_before["batchnorm.num_batches_tracked"]) + 1
        w.stored("bn z", z, y * coef[:, 0] + coef[:, 1])
    # ---- head: Linear + ReLU, Linear + Sigmoid, and the mask application
    a1, mk = buf("a1"), buf("mask")
    w0, w2 = wb("fc_layers.0.weight"), wb("fc_layers.2.weight")
    if do("head"):
        w.stored("relu", a1[..., :F], torch.relu(z @ w0.t() + sd_before["fc_layers.0.bias"].double()))
        w.stored("sigmoid", mk[..., :F], torch.sigmoid(a1[..., :F] @ w2.t() + sd_before["fc_layers.2.bias"].double()))
        assert all_zero(a1[..., F:]) and all_zero(mk[..., F:])
    m5 = mk[..., :F].permute(1, 2, 0).reshape(L, 1, F, T)                                # [B, 1, F, T]
    if do("mask"):
        out = d64(ws.out)
        want = m5.unsqueeze(-1) * x64
        assert tuple(out.shape) == tuple(x.shape) and float(((out - want).abs() / (want.abs() + 1e-30)).max()) < 1e-6, "mask application"
    # ---- backward
    dpre2, dpre1 = buf("dpre2"), buf("dpre1")
    if do("dpre"):
        dm = (G64 * x64).sum(-1).reshape(L, F, T).permute(2, 0, 1)                       # [T, L, F]
        w.stored("dpre2", dpre2[..., :F], mk[..., :F] * (1 - mk[..., :F]) * dm)
        assert all_zero(dpre2[..., F:])
    dp2, dp1 = dpre2[..., :F].reshape(n, F), dpre1[..., :F].reshape(n, F)
    dz = buf("dz")
    if do("head_bwd"):
        a2, z2 = a1[..., :F].reshape(n, F), z.reshape(n, H)
        w.fsum("g fc2.weight", grads["fc_layers.2.weight"], dp2.t() @ a2, dp2.abs().t() @ a2.abs() + 1e-30)
        w.fsum("g fc2.bias", grads["fc_layers.2.bias"], dp2.sum(0), dp2.abs().sum(0))
        w.stored("dpre1", dp1, torch.where(a2 > 0, dp2 @ w2, torch.zeros_like(a2)))
        assert all_zero(dpre1[..., F:])
        w.fsum("g fc0.weight", grads["fc_layers.0.weight"], dp1.t() @ z2, dp1.abs().t() @ z2.abs())
        w.fsum("g fc0.bias", grads["fc_layers.0.bias"], dp1.sum(0), dp1.abs().sum(0) + 1e-30)
        w.stored("dz", dz.reshape(n, H), dp1 @ w0)
    dy = buf("dy")
    if do("bn_bwd"):
        xh = (y - coef[:, 2]) * coef[:, 3]
        w.fsum("g bn.bias", grads["batchnorm.bias"], dz.sum(dim=(0, 1)), dz.abs().sum(dim=(0, 1)))
        w.fsum("g bn.weight", grads["batchnorm.weight"], (dz * xh).sum(dim=(0, 1)), (dz * xh).abs().sum(dim=(0, 1)))
        w.stored("dy", dy, coef[:, 0] * (dz - dz.mean(dim=(0, 1)) - xh * (dz * xh).mean(dim=(0, 1))))
    dh = dy
    for k in range(cfg.rnn_layer - 1, -1, -1):
        hs, st = buf(f"hs{k}"), buf(f"state{k}")
        dG = d64(b[f"dG{k}"]).reshape(T, L, GB, H)
        wih, whh = wb(f"rnn.weight_ih_l{k}"), wb(f"rnn.weight_hh_l{k}")
        if do("bsteps"):
            if cell == "rnn":
                elman_bwd_local(w, f"layer {k}", dG[:, :, 0], dh, st, whh)
            else:
                gates = d64(b[f"gates{k}"]).reshape(T, L, 4, H)
                want = torch.zeros_like(dG)
                carry = torch.zeros(T, H, dtype=torch.float64)
                for s, l in enumerate(range(L - 1, -1, -1)):
                    g = gates[:, l]
                    if s > 0:
                        gh = dG[:, l + 1]
                        rec = (torch.cat([gh[:, 0], gh[:, 1], gh[:, 3]], dim=1) if cell == "gru" else gh.reshape(T, 4 * H)) @ whh
                    else:
                        rec = torch.zeros(T, H, dtype=torch.float64)
                    prev = st[:, l - 1] if l > 0 else torch.zeros(T, H, dtype=torch.float64)
                    if cell == "lstm":
                        dhh = dh[:, l] + rec
                        tc = torch.tanh(st[:, l])
                        dcc = dhh * g[:, 3] * (1 - tc * tc) + carry
                        carry = dcc * g[:, 1]
                        want[:, l, 0] = dcc * g[:, 2] * g[:, 0] * (1 - g[:, 0])
                        want[:, l, 1] = dcc * prev * g[:, 1] * (1 - g[:, 1])
                        want[:, l, 2] = dcc * g[:, 0] * (1 - g[:, 2] ** 2)
                        want[:, l, 3] = dhh * tc * g[:, 3] * (1 - g[:, 3])
                    else:
                        dhh = dh[:, l] + rec + carry
                        carry = dhh * g[:, 1]
                        dpn = dhh * (1 - g[:, 1]) * (1 - g[:, 2] ** 2)
                        want[:, l, 0] = dpn * g[:, 3] * g[:, 0] * (1 - g[:, 0])
                        want[:, l, 1] = dhh * (prev - g[:, 2]) * g[:, 1] * (1 - g[:, 1])
                        want[:, l, 2] = dpn
                        want[:, l, 3] = dpn * g[:, 0]
                w.stored(f"dG{k}", dG, want)
        gi = dG[:, :, :G4].reshape(n, G4 * H)
        if do("rnn_wgrad"):
            x2 = xins[k].reshape(n, -1)
            w.fsum(f"g ih{k}", grads[f"rnn.weight_ih_l{k}"], gi.t() @ x2, gi.abs().t() @ x2.abs() + 1e-30)
            gh = (torch.cat([dG[:, :, 0], dG[:, :, 1], dG[:, :, 3]], dim=-1) if cell == "gru" else dG.reshape(T, L, GB * H)).reshape(n, G4 * H)
            hp = shifted(hs, 0).reshape(n, H)
            w.fsum(f"g hh{k}", grads[f"rnn.weight_hh_l{k}"], gh.t() @ hp, gh.abs().t() @ hp.abs() + 1e-6)
        if k > 0:
            dx = buf(f"dx{k}")
            if do("rnn_dgrad"):
                w.stored(f"dx{k}", dx.reshape(n, H), gi @ wih)
            dh = dx
    return w


@pytest.mark.parametrize("tag", TAGS)
def test_op_local(tag):
    fx = fixture(tag)
    model, ws, est, grads = run_kept(tag)
    after = {k: v.double().cpu() for k, v in model.state_dict().items()}
    w = op_local(model, ws, fx["sd"], fx["input"], fx["G"], grads, after=after)
    print(f"MelRNN {tag} op-local: {w}")


# ------------------------------------------------------------------------------------------------------------------
# 2. whole chain against the reference's vectors
# ------------------------------------------------------------------------------------------------------------------
def loss_gate(what, loss, loss_sim, loss_ref, est_sim, fx):
    """|loss - reference| < 2 x the deviation of the bf16-storage restatement's loss; where that one draw is below 2 sigma of the scalar's
    noise (sigma = ||dloss/dest|| ||est_sim - est|| / sqrt(N): a perturbation of the restatement's norm in a random direction), 2 sigma
    takes its place (tests/test_gpu_rnnmask.py::loss_gate)."""
    e = fx["est"].double().clone().requires_grad_(True)
    torch.nn.functional.mse_loss(e, fx["target"].double()).backward()
    sigma = float(e.grad.norm()) * float((est_sim.double() - fx["est"].double()).norm()) / e.numel() ** 0.5
    bound = 2 * max(abs(loss_sim - loss_ref), 2 * sigma)
    print(f"MelRNN {what}: HIP {loss:.6e}, reference {loss_ref:.6e}, restatement {loss_sim:.6e}; deviation HIP {abs(loss - loss_ref):.3e}, "
          f"restatement {abs(loss_sim - loss_ref):.3e}, sigma {sigma:.3e}, bound {bound:.3e}")
    assert abs(loss - loss_ref) < bound, (what, loss, loss_ref, bound)


def gpu_taps(model, ws):
    T, L = ws.T, ws.L
    t = lambda name, n: d64(ws.bufs[name]).reshape(T, L, -1).permute(1, 0, 2)[..., :n]
    taps = {f"rnn{k}": t(f"hs{k}", model.cfg.H) for k in range(model.cfg.rnn_layer)}
    taps.update(bn=t("z", model.cfg.H), relu=t("a1", model.cfg.F), head=t("mask", model.cfg.F))
    return taps


@pytest.mark.parametrize("tag", TAGS)
def test_whole_chain_vs_reference_vectors(tag):
    fx = fixture(tag)
    model, ws, est, grads = run_kept(tag)
    gs, ests, taps, run = sim_run(tag)
    got = gpu_taps(model, ws)
    assert set(got) == set(fx["tap"])
    for k in sorted(got):
        dev, sim_dev = rel_err(got[k], fx["tap"][k]), rel_err(taps[k], fx["tap"][k])
        print(f"MelRNN {tag} tap.{k}: HIP {dev:.3e}, bf16-storage restatement {sim_dev:.3e}")
        assert dev < 2 * sim_dev, (k, dev, sim_dev)
    dev, sim_dev = rel_err(est, fx["est"]), rel_err(ests, fx["est"])
    print(f"MelRNN {tag} est: HIP {dev:.3e}, bf16-storage restatement {sim_dev:.3e}")
    assert dev < 2 * sim_dev, (dev, sim_dev)
    sd = {k: v.cpu() for k, v in model.state_dict().items()}
    for k in ("batchnorm.running_mean", "batchnorm.running_var"):
        dev, sim_dev = rel_err(sd[k], fx["run"][k]), rel_err(run[k], fx["run"][k])
        print(f"MelRNN {tag} {k}: HIP {dev:.3e}, bf16-storage restatement {sim_dev:.3e}")
        assert dev < 2 * sim_dev, (k, dev, sim_dev)
    assert int(sd["batchnorm.num_batches_tracked"]) == int(fx["run"]["batchnorm.num_batches_tracked"]) == 1
    mse = torch.nn.functional.mse_loss
    loss_gate(f"{tag} loss", float(mse(est, fx["target"])), float(mse(ests, fx["target"])), float(fx["loss"]), ests, fx)
    names = list(grads)
    (glob, worst), (sglob, sworst) = grad_dev(grads, fx["gradG"], names), grad_dev(gs, fx["gradG"], names)
    print(f"MelRNN {tag} gradients of <est, G>: HIP global {glob:.4f} (worst large tensor {worst:.4f}), bf16-storage restatement "
          f"{sglob:.4f} ({sworst:.4f})")
    assert glob < 2 * sglob, (glob, sglob)


def sim_adam(tag, steps=2):
    """`steps` Adam steps of the bf16-storage restatement: (losses, final parameters and statistics)"""
    fx = fixture(tag)
    names = R.param_names(fx["sd"])
    p = {k: (v.clone().requires_grad_(True) if k in names else v.clone()) for k, v in fx["sd"].items()}
    opt = torch.optim.Adam([p[k] for k in names], lr=3e-4, betas=(0.9, 0.999))
    losses = []
    for _ in range(steps):
        run = {}
        loss = torch.nn.functional.mse_loss(R.melrnn_forward(p, fx["input"], sim=R.Bf16Sim, running=run, **kw(tag)), fx["target"])
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_([p[k] for k in names], 5)
        opt.step()
        p.update(run)
        losses.append(loss.item())
    return losses, p


@pytest.mark.parametrize("tag", TAGS)
def test_two_adam_steps_vs_reference_vectors(tag):
    from sehip import distrib, utils
    from sehip.loss import mse_loss
    from sehip.model import MelRNN
    fx = fixture(tag)
    names = R.param_names(fx["sd"])
    sim_losses, p = sim_adam(tag)
    model = MelRNN(**kw(tag))
    model.load_state_dict(fx["sd"])
    model.cuda().train()
    hopt = distrib.get_optimizer(utils.dict2obj({"optim": "adam", "lr": 3e-4, "beta1": 0.9, "beta2": 0.999}), model)
    x, tgt = fx["input"].cuda(), fx["target"].cuda()
    losses = []
    for _ in range(2):
        loss = mse_loss(model(x), tgt)
        hopt.zero_grad()
        loss.backward()
        hopt.clip_grad_norm_(5.0)
        hopt.step()
        losses.append(float(loss))
    torch.cuda.synchronize()
    sd = {k: v.cpu() for k, v in model.state_dict().items()}
    _, ests, _, _ = sim_run(tag)
    for i in range(2):
        loss_gate(f"{tag} two Adam steps, loss {i + 1}", losses[i], sim_losses[i], float(fx["adam_losses"][i]), ests, fx)
    upd = lambda d: {k: d[k].detach().double() - fx["sd"][k].double() for k in names}
    (glob, _), (sglob, _) = grad_dev(upd(sd), upd(fx["adam"]), names), grad_dev(upd(p), upd(fx["adam"]), names)
    print(f"MelRNN {tag} two Adam steps: parameter updates HIP {glob:.4f}, bf16-storage restatement {sglob:.4f}")
    assert glob < 2 * sglob, (glob, sglob)
    assert int(sd["batchnorm.num_batches_tracked"]) == int(fx["adam"]["batchnorm.num_batches_tracked"]) == 2
    for k in ("batchnorm.running_mean", "batchnorm.running_var"):
        dev, sim_dev = rel_err(sd[k], fx["adam"][k]), rel_err(p[k], fx["adam"][k])
        print(f"MelRNN {tag} two Adam steps: {k} HIP {dev:.3e}, bf16-storage restatement {sim_dev:.3e}")
        assert dev < 2 * sim_dev, (k, dev, sim_dev)


# ------------------------------------------------------------------------------------------------------------------
# 3. eval mode
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_eval_mode(tag):
    from sehip import SehipError
    from sehip.model import MelRNN
    fx = fixture(tag)
    sd = dict(fx["sd"])
    sd.update(fx["run"])
    model = MelRNN(**kw(tag))
    model.load_state_dict(sd)
    model.cuda().eval()
    with torch.no_grad():
        est = model(fx["input"].cuda()).cpu()
        sim = R.melrnn_forward(sd, fx["input"], training=False, sim=R.Bf16Sim, **kw(tag))
    dev, sim_dev = rel_err(est, fx["est_eval"]), rel_err(sim, fx["est_eval"])
    print(f"MelRNN {tag} eval: HIP {dev:.3e}, bf16-storage restatement {sim_dev:.3e}")
    assert dev < 2 * sim_dev, (dev, sim_dev)
    after = model.state_dict()
    assert all(torch.equal(after[k].cpu(), sd[k]) for k in fx["run"])                   # eval leaves the statistics alone
    out = model(fx["input"].cuda())
    with pytest.raises(SehipError, match="eval mode"):
        out.sum().backward()


# ------------------------------------------------------------------------------------------------------------------
# 4. the Elman entry points called directly, two directions
# ------------------------------------------------------------------------------------------------------------------
def test_elman_kernels_two_directions():
    from sehip._lib import call, ptr, stream
    Bn, L, H, D, PAD = 17, 3, 32, 2, 64
    g = torch.Generator().manual_seed(13)
    pre = torch.randn(Bn, L, D, H, generator=g).cuda()
    whh = (torch.rand(D, H, H, generator=g) * 2 - 1).mul(H ** -0.5).bfloat16().cuda()
    whhT = whh.transpose(1, 2).contiguous()
    dhs = torch.randn(Bn, L, D * H, generator=g).bfloat16().cuda()

    def padded(n, dtype):
        raw = torch.full((n + 2 * PAD,), 7.0, dtype=dtype, device="cuda")
        raw[PAD:PAD + n] = 0
        return raw, raw[PAD:PAD + n]

    def run():
        bufs = [padded(Bn * L * D * H, dt) for dt in (torch.bfloat16, torch.float32, torch.bfloat16)]
        (hs, state, dG) = (v for _, v in bufs)
        call("sehip_rsm_elman_fwd", ptr(pre), ptr(whh), hs.data_ptr(), state.data_ptr(), Bn, L, H, D, stream())
        call("sehip_rsm_elman_bwd", ptr(whhT), state.data_ptr(), ptr(dhs), dG.data_ptr(), Bn, L, H, D, stream())
        torch.cuda.synchronize()
        for raw, v in bufs:
            assert bool((raw[:PAD] == 7.0).all()) and bool((raw[PAD + v.numel():] == 7.0).all()), "a guard band was written"
        return hs.clone(), state.clone(), dG.clone()

    hs, state, dG = run()
    w = Worst()
    v = lambda t: d64(t).reshape(Bn, L, D, H)
    for d in range(D):
        elman_fwd_local(w, f"direction {d}", d64(pre)[:, :, d], v(hs)[:, :, d], v(state)[:, :, d], whh[d].double().cpu(), reverse=bool(d))
        elman_bwd_local(w, f"direction {d}", v(dG)[:, :, d], v(dhs)[:, :, d], v(state)[:, :, d], whh[d].double().cpu(), reverse=bool(d))
    assert float(hs.float().abs().min()) > 0 and float(dG.float().abs().max()) > 0            # every row, the ragged tile's too, was written
    again = run()
    assert all(torch.equal(a, b_) for a, b_ in zip((hs, state, dG), again)), "two runs differ"
    print(f"sehip_rsm_elman_fwd / _bwd, D = 2, 17 rows x 3 steps, H = 32: {w}; a second run is bit-identical")


# ------------------------------------------------------------------------------------------------------------------
# 5. edges, with guard bands around every buffer
# ------------------------------------------------------------------------------------------------------------------
EDGES = {
    "L1":       (dict(rnn_type="rnn", rnn_hidden=32, rnn_layer=2, n_fft=64), (1, 1, 33, 40, 2)),       # no recurrent product
    "T1":       (dict(rnn_type="rnn", rnn_hidden=64, rnn_layer=2, n_fft=64), (4, 1, 33, 1, 2)),
    "T16":      (dict(rnn_type="rnn", rnn_hidden=32, rnn_layer=2, n_fft=30), (2, 1, 16, 16, 2)),       # T = 16, F = 16: no padding
    "T17_h96":  (dict(rnn_type="rnn", rnn_hidden=96, rnn_layer=1, n_fft=64), (3, 1, 33, 17, 2)),       # ragged 64-unit block
    "rnn_3":    (dict(rnn_type="rnn", rnn_hidden=96, rnn_layer=3, n_fft=30), (2, 1, 16, 17, 2)),
    "lstm_3":   (dict(rnn_type="lstm", rnn_hidden=32, rnn_layer=3, n_fft=64), (5, 1, 33, 35, 2)),      # lstm through the new head
}


@pytest.mark.parametrize("name", sorted(EDGES))
def test_edges_with_guard_bands(name):
    from sehip.model import MelRNN
    args, shape = EDGES[name]
    args = dict(args, n_mels=0)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(*shape, generator=g)
    torch.manual_seed(31)
    sd = MelRNN(**args).state_dict()
    G = torch.randn(*shape, generator=g) / x.numel() ** 0.5
    model, ws, est, grads = run_model(args, sd, x, G, guard=64, seed=31)
    assert ws.guard == 64 and ws.guards_intact() == [], ws.guards_intact()
    assert len(ws._alloc) == len(ws.bufs) + 5                                            # every buffer, the arena and the scratch are banded
    assert tuple(est.shape) == shape and bool(torch.isfinite(est).all()) and all(bool(torch.isfinite(v).all()) for v in grads.values())
    if ws.L == 1:
        assert all(float(grads[k].abs().max()) == 0.0 for k in grads if "weight_hh" in k)  # no recurrent product at all
    else:
        assert all(float(grads[k].abs().max()) > 0.0 for k in grads if "weight_hh" in k)
    w = op_local(model, ws, sd, x, G, grads, only=RNN_T)
    print(f"MelRNN edge {name} {shape}: guard bands intact; recurrence and transposing kernels op-local: {w}")


# ------------------------------------------------------------------------------------------------------------------
# 6. Solver
# ------------------------------------------------------------------------------------------------------------------
def _solver_config(tag, deterministic, tmp):
    from sehip.utils import dict2obj
    return dict2obj({
        "seed": 10, "root": None, "ha": None,
        "model": dict(name="mel-rnn", audio_channels=1, num_spk=1, win_length=64, center=True, segment=0.02, **kw(tag)),
        "optim": {"optim": "adam", "lr": 3e-4, "beta1": 0.9, "beta2": 0.999, "loss": "mse", "clip_grad": 5, "pit": True, "load": True},
        "dset": {"name": "fixture", "norm": "z-score", "sample_rate": 16000},
        "solver": {"epochs": 1, "save_checkpoint_interval": 1, "all_steps": True, "total_steps": 0, "patience": 0, "root": str(tmp),
                   "resume": None, "preloaded_model": None, "cudnn_deterministic": deterministic, "use_graph": False,
                   "validation": {"interval": 1, "metric": "loss", "total_steps": 0}, "test": {"interval": 1}},
    })


def test_solver_three_steps_and_evaluate(tmp_path):
    from sehip import distrib
    from sehip.evaluate import evaluate
    from sehip.model import MelRNN
    from sehip.solver import Solver, ScalarLog
    from sehip.utils import set_deterministic
    tag = "melrnn_rnn2"
    fx = fixture(tag)
    _, ests, _, _ = sim_run(tag)
    sim_losses, _ = sim_adam(tag)
    runs = []
    try:
        for deterministic in (False, True):
            cfg = _solver_config(tag, deterministic, tmp_path)
            model = distrib.get_model(cfg.model)
            assert isinstance(model, MelRNN)
            model.load_state_dict(fx["sd"])
            hopt = distrib.get_optimizer(cfg.optim, model)
            solver = Solver(cfg, model, hopt, distrib.get_loss_function(cfg.optim), device="gpu", writer=ScalarLog())
            x, tgt = fx["input"].cuda(), fx["target"].cuda()
            losses = [float(solver.train_step(x, tgt)[0]) for _ in range(3)]
            runs.append((losses, model.flat_params.detach().cpu().clone()))
            for i in range(2):
                loss_gate(f"Solver (cudnn_deterministic={deterministic}) loss {i + 1}", losses[i], sim_losses[i], float(fx["adam_losses"][i]), ests, fx)
            assert losses[2] < losses[0]
    finally:
        set_deterministic(False)
    # no atomics in the model: the switch changes no bit of the three updates.  (The reported loss is the library's plain mse reduction,
    # sehip_pointwise_loss_fwd, which sums in one workgroup under the switch and in several without it: the scalar may differ in its
    # last fp32 bits, its gradient does not depend on it.)
    assert torch.equal(runs[0][1], runs[1][1])
    print(f"MelRNN Solver: losses {runs[0][0]} / with cudnn_deterministic {runs[1][0]}; parameters after three steps bit-identical")
    assert all(abs(a - b) <= 1e-6 * abs(a) for a, b in zip(runs[0][0], runs[1][0]))
    wav = 0.1 * torch.randn(2, 1, 320 + 2 * 64 + 9, generator=torch.Generator().manual_seed(1))
    y = evaluate(wav, model, torch.device("cuda:0"), cfg)
    assert y.is_cuda and tuple(y.shape) == tuple(wav.shape) and bool(torch.isfinite(y).all())


# ------------------------------------------------------------------------------------------------------------------
# 7. the shipped width
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell, layers", [("lstm", 1), ("rnn", 2)])
def test_shipped_width(cell, layers):
    from sehip.model import MelRNN
    args = dict(rnn_type=cell, rnn_hidden=1024, rnn_layer=layers, n_mels=0, n_fft=512, hop_length=128)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(4, 1, 257, 33, 2, generator=g)
    G = torch.randn(4, 1, 257, 33, 2, generator=g) / x.numel() ** 0.5
    torch.manual_seed(41)
    sd = MelRNN(**args).state_dict()
    model, ws, est, grads = run_model(args, sd, x, G, seed=41)
    assert bool(torch.isfinite(est).all()) and all(bool(torch.isfinite(v).all()) for v in grads.values())
    w = op_local(model, ws, sd, x, G, grads, only={"steps", "bsteps", "head", "head_bwd"})
    print(f"MelRNN shipped width ({cell}, K = 1024 recurrent steps, heads of 264 columns) op-local: {w}")
    with torch.no_grad():
        want = R.melrnn_forward(sd, x, **args)
    print(f"MelRNN shipped width ({cell}): est deviates {rel_err(est, want):.3e} from the fp32 restatement (not gated)")
