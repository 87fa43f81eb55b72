"""GPU: rnn-stft-mask (sehip.model.RNNBaseSTFTMask) on the HIP path (csrc/rnnmask.hip, sehip/plan_rnnmask.py).

1. op-local: after one forward + backward pass EVERY launch is recomputed in float64 from the operands the kernel itself read, taken back
   from the workspace -- for the recurrence every step from the device's own h(l -+ 1) / c(l -+ 1) and, backward, the device's own dG of
   the neighbouring step.  (The carried cell / hidden gradient is fp32 scratch that only holds its last value: the float64 chain
   carries its own, which differs from the device's by fp32 rounding only.)  Gates: stored bf16 tensors <= 1.8e-3 rms and <= 2^-8 1.02
   per element, fp32 sums <= 2e-5 of the sum of the absolute addends (tests/test_gpu_wavunet.py:37-39).
2. the whole chain against vectors of the imported reference (tests/golden/rnnmask_*.npz): every bound is 2 x the deviation of the
   bf16-storage restatement (tests/rnnmask_ref.py under Bf16Sim) from the same vectors, computed on the CPU in the same test; a loss is
   one number, so its gate follows tests/test_gpu_wavunet.py::loss_gate (2 sigma of the scalar's noise where the restatement's one
   draw happens to be smaller).
3. dropout; 4. eval mode; 5. edges with guard bands; 6. three Solver steps through the registry and evaluate(); 7. the shipped width.

Measured on an MI355X (every test prints what it gates), fixtures gru_uni / lstm_bi:
  op-local   stored tensors worst rms 1.76e-3 / 1.70e-3 (gate 1.8e-3), worst element 0.993 / 0.995 of a bf16 rounding step; fp32 sums
             1.4e-7 / 1.6e-7 of the absolute addends (gate 2e-5); with drop_out 0.5 (lstm_bi): 1.76e-3, 0.994, 1.4e-7, mask == twin
  chain      est 5.066e-3 / 5.795e-3, the restatement's deviation to all four digits; taps rnn0 2.849e-3 / 3.164e-3, rnn1 3.480e-3 /
             3.852e-3, bn 4.393e-3 / 5.348e-3, head 4.872e-3 / 5.736e-3 (restatement: the same); running_mean 2.212e-3 / 2.739e-3 (same),
             running_var 1.626e-6 / 5.452e-7 (restatement 1.613e-6 / 5.476e-7); loss deviation 9.47e-6 / 7.56e-6 (bound 5.0e-5 / 2.1e-5);
             gradients of <est, G> 0.0054 / 0.0384 global (restatement 0.0053 / 0.0383)
  Adam x 2   second loss 7.9e-6 / 2.37e-5 off (bound 5.0e-5 / 4.7e-5); parameter updates 0.1888 / 0.2221 (restatement 0.1771 / 0.2223)
  eval       3.065e-3 / 2.893e-3 (restatement: the same)
  edges      guard bands intact in all six; worst rms 1.96e-3 at T = 1 (1024-element tensors: the gate is scaled by the correctly rounded
             reference's own rms there), 1.70e-3 .. 1.81e-3 elsewhere; worst element 0.995
  Solver     losses 1.769408e-2, 1.725442e-2 (reference 1.768652e-2, 1.723076e-2), the same bits with cudnn_deterministic
  shipped    [2, 2, 257, 33, 2], H = 896 x 3 bidirectional: K = 896 steps and the 514-column head 1.67e-3 rms, 0.995; est deviates 5.41e-3
             from the fp32 restatement under the same dropout masks (not gated)
"""
import pytest
import torch

import rnnmask_ref as R
from ctn_variants_ref import grad_dev
from util import rel_err

pytestmark = pytest.mark.gpu

OUT_TOL = 1.8e-3              # rms of ONE round-to-nearest bf16 rounding is 1.65e-3 (tests/test_gpu_convtasnet_variants.py)
ULP_TOL = 2.0 ** -8 * 1.02
SUM_TOL = 2e-5                # fp32 sums, relative to the sum of the absolute addends
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


def out_err(got, want):
    got, want = got.double(), want.double()
    floor = 1e-3 * float(want.pow(2).mean().sqrt())
    return rel_err(got, want), float(((got - want).abs() / (want.abs() + floor)).max())


class Worst:
    def __init__(self):
        self.rms = self.ulp = self.sum = 0.0

    def stored(self, what, got, want):
        """the rms of one rounding over n elements is a sample statistic (1.65e-3 only in the limit): below 4096 elements the gate is scaled
        by the correctly rounded reference's own rms where that lies above 1.65e-3 (as the guard-band test of tests/test_gpu_wavunet.py)"""
        rms, ulp = out_err(got, want)
        tol = OUT_TOL
        if want.numel() < 4096:
            tol *= max(1.0, rel_err(want.bfloat16().double(), want) / 1.65e-3)
        assert rms < tol and ulp < ULP_TOL, (what, rms, ulp, tol)
        self.rms, self.ulp = max(self.rms, rms), max(self.ulp, ulp)

    def fsum(self, what, got, want, addends):
        """got / want: fp32 sums (or smooth functions of one); addends: the sum of the absolute addends, same shape"""
        err = float(((got.double() - want.double()).abs() / (addends.double() + 1e-30)).max())
        assert err < SUM_TOL, (what, err)
        self.sum = max(self.sum, err)

    def __str__(self):
        return (f"stored tensors worst rms {self.rms:.2e}, worst element {self.ulp / 2 ** -8:.3f} bf16 roundings; fp32 sums {self.sum:.1e} "
                "of the absolute addends")


def run_model(model_kw, sd, x, G, guard=0, seed=None):
    """one training-mode forward + backward pass under the upstream gradient G: (model, workspace, est, gradients)"""
    from sehip.model import RNNBaseSTFTMask
    if seed is not None:
        torch.manual_seed(seed)
    model = RNNBaseSTFTMask(**model_kw)
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
        est = R.rnnmask_forward(p, fx["input"], sim=R.Bf16Sim, taps=taps, running=run, **kw(tag))
        (est * fx["G"]).sum().backward()
        _SIM[tag] = ({k: p[k].grad for k in names}, est.detach(), {k: v.detach() for k, v in taps.items()}, run)
    return _SIM[tag]


def d64(t):
    return t.detach().double().cpu()


def all_zero(t):
    return t.numel() == 0 or float(t.abs().max()) == 0.0


def shifted(t, d):
    """t [T, L, ...] -> the tensor of the step BEFORE each step in direction d's forward order (zeros at the start)"""
    z = torch.zeros_like(t)
    if d == 0:
        z[:, 1:] = t[:, :-1]
    else:
        z[:, :-1] = t[:, 1:]
    return z


# ------------------------------------------------------------------------------------------------------------------
# 1. op-local: every launch from the operands it read
# ------------------------------------------------------------------------------------------------------------------
def op_local(model, ws, sd_before, x, G, grads, after=None, only=None):
    """only: None = every launch; "rnn_t" = the recurrence and the two transposing kernels (test 5); a set of names otherwise"""
    cfg, b = model.cfg, ws.bufs
    T, L, H, D, G4, Ho, F, S = ws.T, ws.L, cfg.H, cfg.D, cfg.G, cfg.Hout, cfg.F, cfg.num_spk
    gru = cfg.gru
    w = Worst()
    want_all = only is None
    do = lambda name: want_all or (only == "rnn_t" and name in ("feat", "steps", "mask", "dpre", "bsteps")) or (not isinstance(only, str) and only is not None and name in only)
    wb = lambda k: sd_before[k].bfloat16().double()
    x64, G64 = x.double(), G.double()
    buf = lambda name: d64(b[name]).reshape(T, L, -1)
    seed = model.dropout_seed
    ctr = int(ws.ctr_used[0].item()) & 0xFFFFFFFF
    masks = {}
    if ws.dropping:
        for k in range(cfg.rnn_layer - 1):
            masks[k] = R.device_mask(seed, ctr, k, L, T, Ho, cfg.drop_out, torch.float64).permute(1, 0, 2)     # [T, L, Ho]
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
        sfxs = ("", "_reverse")[:D]
        pre = d64(b[f"pre{k}"]).reshape(T, L, D, G4, H)
        gates = d64(b[f"gates{k}"]).reshape(T, L, D, 4, H)
        hs = buf(f"hs{k}").reshape(T, L, D, H)
        st = buf(f"state{k}").reshape(T, L, D, H)
        if do("ih"):
            for d, sfx in enumerate(sfxs):
                wih = wb(f"rnn.weight_ih_l{k}{sfx}")
                w.fsum(f"pre{k}.{d}", pre[:, :, d].reshape(T, L, G4 * H), xin @ wih.t(), xin.abs() @ wih.abs().t())
        if do("steps"):
            want_h = torch.zeros_like(hs)
            for d, sfx in enumerate(sfxs):
                whh = wb(f"rnn.weight_hh_l{k}{sfx}")
                hp, sp = shifted(hs[:, :, d], d), shifted(st[:, :, d], d)
                a = (hp @ whh.t()).reshape(T, L, G4, H)
                aa = (hp.abs() @ whh.abs().t()).reshape(T, L, G4, H)
                p_ = pre[:, :, d]
                g = gates[:, :, d]
                if not gru:
                    z = p_ + a
                    act = torch.stack([torch.sigmoid(z[:, :, 0]), torch.sigmoid(z[:, :, 1]), torch.tanh(z[:, :, 2]), torch.sigmoid(z[:, :, 3])], dim=2)
                    w.fsum(f"gates{k}.{d}", g, act, p_.abs() + aa + 1)
                    c = g[:, :, 1] * sp + g[:, :, 0] * g[:, :, 2]
                    w.fsum(f"c{k}.{d}", st[:, :, d], c, (g[:, :, 1] * sp).abs() + (g[:, :, 0] * g[:, :, 2]).abs() + 1e-3)
                    want_h[:, :, d] = g[:, :, 3] * torch.tanh(st[:, :, d])
                else:
                    r = torch.sigmoid(p_[:, :, 0] + a[:, :, 0])
                    zt = torch.sigmoid(p_[:, :, 1] + a[:, :, 1])
                    w.fsum(f"r{k}.{d}", g[:, :, 0], r, p_[:, :, 0].abs() + aa[:, :, 0] + 1)
                    w.fsum(f"z{k}.{d}", g[:, :, 1], zt, p_[:, :, 1].abs() + aa[:, :, 1] + 1)
                    w.fsum(f"an{k}.{d}", g[:, :, 3], a[:, :, 2], aa[:, :, 2] + 1e-3)
                    n = torch.tanh(p_[:, :, 2] + g[:, :, 0] * g[:, :, 3])
                    w.fsum(f"n{k}.{d}", g[:, :, 2], n, p_[:, :, 2].abs() + (g[:, :, 0] * g[:, :, 3]).abs() + 1)
                    h = (1 - g[:, :, 1]) * g[:, :, 2] + g[:, :, 1] * sp
                    w.fsum(f"h{k}.{d}", st[:, :, d], h, ((1 - g[:, :, 1]) * g[:, :, 2]).abs() + (g[:, :, 1] * sp).abs() + 1e-3)
                    want_h[:, :, d] = st[:, :, d]
            w.stored(f"hs{k}", hs, want_h)
        xin = hs.reshape(T, L, Ho)
        if k in masks:
            hd = buf(f"hd{k}")
            if do("steps"):
                w.stored(f"hd{k}", hd, xin * masks[k])
                assert torch.equal(hd != 0, (xin != 0) & (masks[k] != 0)), f"layer {k}: the device's dropout mask is not the twin's"
            xin = hd
    # ---- BatchNorm1d
    y, z = xin, buf("z")
    coef = d64(ws.coef)
    n = T * L
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
    # ---- head and mask application
    mk = buf("mask")
    wfc = wb("fc_layers.0.weight")
    if do("head"):
        bias = sd_before["fc_layers.0.bias"].double()
        w.stored("head", mk[..., :S * F], torch.relu(z @ wfc.t() + bias))
        assert all_zero(mk[..., S * F:])
    B, C = ws.B, cfg.audio_channels
    m5 = mk[..., :S * F].reshape(T, B, C, S, F).permute(1, 3, 2, 4, 0)               # [B, S, C, F, T]
    if do("mask"):
        out = d64(ws.out)
        want = m5.unsqueeze(-1) * x64.unsqueeze(1)
        assert float(((out - want).abs() / (want.abs() + 1e-30)).max()) < 1e-6, "mask application"
    # ---- backward
    dpre = buf("dpre")
    if do("dpre"):
        dm = (G64 * x64.unsqueeze(1)).sum(-1)                                         # [B, S, C, F, T]
        dm = torch.where(m5 > 0, dm, torch.zeros_like(dm)).permute(4, 0, 2, 1, 3).reshape(T, L, S * F)
        w.stored("dpre", dpre[..., :S * F], dm)
        assert all_zero(dpre[..., S * F:])
    dp = dpre[..., :S * F].reshape(n, S * F)
    dz = buf("dz")
    if do("head_bwd"):
        z2 = z.reshape(n, Ho)
        w.fsum("g fc.weight", grads["fc_layers.0.weight"], dp.t() @ z2, dp.abs().t() @ z2.abs())
        w.fsum("g fc.bias", grads["fc_layers.0.bias"], dp.sum(0), dp.abs().sum(0))
        w.stored("dz", dz.reshape(n, Ho), dp @ wfc)
    dy = buf("dy")
    if do("bn_bwd"):
        xh = (y - coef[:, 2]) * coef[:, 3]
        w.fsum("g bn.bias", grads["batchnorm.bias"], dz.sum(dim=(0, 1)), dz.abs().sum(dim=(0, 1)))
        w.fsum("g bn.weight", grads["batchnorm.weight"], (dz * xh).sum(dim=(0, 1)), (dz * xh).abs().sum(dim=(0, 1)))
        w.stored("dy", dy, coef[:, 0] * (dz - dz.mean(dim=(0, 1)) - xh * (dz * xh).mean(dim=(0, 1))))
    dh = dy
    for k in range(cfg.rnn_layer - 1, -1, -1):
        sfxs = ("", "_reverse")[:D]
        gates = d64(b[f"gates{k}"]).reshape(T, L, D, 4, H)
        hs = buf(f"hs{k}").reshape(T, L, D, H)
        st = buf(f"state{k}").reshape(T, L, D, H)
        dG = d64(b[f"dG{k}"]).reshape(T, L, D, 4, H)
        dout = (dh * masks[k] if k in masks else dh).reshape(T, L, D, H)
        xk = xins[k]
        if do("bsteps"):
            want = torch.zeros_like(dG)
            for d, sfx in enumerate(sfxs):
                whh = wb(f"rnn.weight_hh_l{k}{sfx}")                                  # [G H][H]
                carry = torch.zeros(T, H, dtype=torch.float64)
                order = range(L - 1, -1, -1) if d == 0 else range(L)
                for s, l in enumerate(order):
                    ln = l + 1 if d == 0 else l - 1                                  # the step after l in forward order
                    lp = l - 1 if d == 0 else l + 1
                    g = gates[:, l, d]
                    if s > 0:
                        gh = dG[:, ln, d]
                        gh = torch.cat([gh[:, 0], gh[:, 1], gh[:, 3]], dim=1) if gru else gh.reshape(T, 4 * H)
                        rec = gh @ whh
                    else:
                        rec = torch.zeros(T, H, dtype=torch.float64)
                    prev = st[:, lp, d] if 0 <= lp < L else torch.zeros(T, H, dtype=torch.float64)
                    if not gru:
                        dhh = dout[:, l, d] + rec
                        tc = torch.tanh(st[:, l, d])
                        dcc = dhh * g[:, 3] * (1 - tc * tc) + carry
                        carry = dcc * g[:, 1]
                        want[:, l, d, 0] = dcc * g[:, 2] * g[:, 0] * (1 - g[:, 0])
                        want[:, l, d, 1] = dcc * prev * g[:, 1] * (1 - g[:, 1])
                        want[:, l, d, 2] = dcc * g[:, 0] * (1 - g[:, 2] ** 2)
                        want[:, l, d, 3] = dhh * tc * g[:, 3] * (1 - g[:, 3])
                    else:
                        dhh = dout[:, l, d] + rec + carry
                        carry = dhh * g[:, 1]
                        dpn = dhh * (1 - g[:, 1]) * (1 - g[:, 2] ** 2)
                        want[:, l, d, 0] = dpn * g[:, 3] * g[:, 0] * (1 - g[:, 0])
                        want[:, l, d, 1] = dhh * (prev - g[:, 2]) * g[:, 1] * (1 - g[:, 1])
                        want[:, l, d, 2] = dpn
                        want[:, l, d, 3] = dpn * g[:, 0]
            w.stored(f"dG{k}", dG, want)
        if do("rnn_wgrad"):
            for d, sfx in enumerate(sfxs):
                gi = dG[:, :, d, :G4].reshape(n, G4 * H)
                x2 = xk.reshape(n, -1)
                w.fsum(f"g ih{k}.{d}", grads[f"rnn.weight_ih_l{k}{sfx}"], gi.t() @ x2, gi.abs().t() @ x2.abs() + 1e-30)
                gh = dG[:, :, d]
                gh = (torch.cat([gh[:, :, 0], gh[:, :, 1], gh[:, :, 3]], dim=-1) if gru else gh.reshape(T, L, 4 * H)).reshape(n, G4 * H)
                hp = shifted(hs[:, :, d], d).reshape(n, H)
                w.fsum(f"g hh{k}.{d}", grads[f"rnn.weight_hh_l{k}{sfx}"], gh.t() @ hp, gh.abs().t() @ hp.abs() + 1e-6)
        if k > 0:
            dx = buf(f"dx{k}")
            if do("rnn_dgrad"):
                tot = torch.zeros(n, Ho, dtype=torch.float64)
                for d, sfx in enumerate(sfxs):
                    tot += dG[:, :, d, :G4].reshape(n, G4 * H) @ wb(f"rnn.weight_ih_l{k}{sfx}")
                w.stored(f"dx{k}", dx.reshape(n, Ho), tot)
            dh = dx
    return w


@pytest.mark.parametrize("tag", TAGS)
def test_op_local(tag):
    fx = fixture(tag)
    model, ws, est, grads = run_kept(tag)
    after = {k: v.double().cpu() for k, v in model.state_dict().items()}
    w = op_local(model, ws, fx["sd"], fx["input"], fx["G"], grads, after=after)
    print(f"RNNBaseSTFTMask {tag} op-local: {w}")


# ------------------------------------------------------------------------------------------------------------------
# 2. whole chain against the reference's vectors
# ------------------------------------------------------------------------------------------------------------------
def loss_gate(what, loss, loss_sim, loss_ref, est_sim, fx):
    """|loss - reference| < 2 x the deviation of the bf16-storage restatement's loss; where that one draw is below 2 sigma of the scalar's
    noise (sigma = ||dloss/dest|| ||est_sim - est|| / sqrt(N): a perturbation of the restatement's norm in a random direction), 2 sigma
    takes its place (tests/test_gpu_wavunet.py::loss_gate)."""
    e = fx["est"].double().clone().requires_grad_(True)
    torch.nn.functional.mse_loss(e, fx["target"].double()).backward()
    sigma = float(e.grad.norm()) * float((est_sim.double() - fx["est"].double()).norm()) / e.numel() ** 0.5
    bound = 2 * max(abs(loss_sim - loss_ref), 2 * sigma)
    print(f"RNNBaseSTFTMask {what}: HIP {loss:.6e}, reference {loss_ref:.6e}, restatement {loss_sim:.6e}; deviation HIP {abs(loss - loss_ref):.3e}, "
          f"restatement {abs(loss_sim - loss_ref):.3e}, sigma {sigma:.3e}, bound {bound:.3e}")
    assert abs(loss - loss_ref) < bound, (what, loss, loss_ref, bound)


def gpu_taps(model, ws):
    T, L = ws.T, ws.L
    t = lambda name, n: d64(ws.bufs[name]).reshape(T, L, -1).permute(1, 0, 2)[..., :n]
    taps = {f"rnn{k}": t(f"hs{k}", model.cfg.Hout) for k in range(model.cfg.rnn_layer)}
    taps["bn"] = t("z", model.cfg.Hout)
    taps["head"] = t("mask", model.cfg.SF)
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
        print(f"RNNBaseSTFTMask {tag} tap.{k}: HIP {dev:.3e}, bf16-storage restatement {sim_dev:.3e}")
        assert dev < 2 * sim_dev, (k, dev, sim_dev)
    dev, sim_dev = rel_err(est, fx["est"]), rel_err(ests, fx["est"])
    print(f"RNNBaseSTFTMask {tag} est: HIP {dev:.3e}, bf16-storage restatement {sim_dev:.3e}")
    assert dev < 2 * sim_dev, (dev, sim_dev)
    sd = {k: v.cpu() for k, v in model.state_dict().items()}
    for k in ("batchnorm.running_mean", "batchnorm.running_var"):
        dev, sim_dev = rel_err(sd[k], fx["run"][k]), rel_err(run[k], fx["run"][k])
        print(f"RNNBaseSTFTMask {tag} {k}: HIP {dev:.3e}, bf16-storage restatement {sim_dev:.3e}")
        assert dev < 2 * sim_dev, (k, dev, sim_dev)
    assert int(sd["batchnorm.num_batches_tracked"]) == int(fx["run"]["batchnorm.num_batches_tracked"]) == 1
    mse = torch.nn.functional.mse_loss
    loss_gate(f"{tag} loss", float(mse(est, fx["target"])), float(mse(ests, fx["target"])), float(fx["loss"]), ests, fx)
    names = list(grads)
    (glob, worst), (sglob, sworst) = grad_dev(grads, fx["gradG"], names), grad_dev(gs, fx["gradG"], names)
    print(f"RNNBaseSTFTMask {tag} gradients of <est, G>: HIP global {glob:.4f} (worst large tensor {worst:.4f}), bf16-storage restatement "
          f"{sglob:.4f} ({sworst:.4f})")
    assert glob < 2 * sglob, (glob, sglob)


@pytest.mark.parametrize("tag", TAGS)
def test_two_adam_steps_vs_reference_vectors(tag):
    from sehip import distrib, utils
    from sehip.loss import mse_loss
    from sehip.model import RNNBaseSTFTMask
    fx = fixture(tag)
    names = R.param_names(fx["sd"])
    p = {k: (v.clone().requires_grad_(True) if k in names else v.clone()) for k, v in fx["sd"].items()}
    opt = torch.optim.Adam([p[k] for k in names], lr=3e-4, betas=(0.9, 0.999))
    sim_losses = []
    for _ in range(2):
        run = {}
        loss = torch.nn.functional.mse_loss(R.rnnmask_forward(p, fx["input"], sim=R.Bf16Sim, running=run, **kw(tag)), fx["target"])
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_([p[k] for k in names], 5)
        opt.step()
        p.update(run)
        sim_losses.append(loss.item())
    model = RNNBaseSTFTMask(**kw(tag))
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
    print(f"RNNBaseSTFTMask {tag} two Adam steps: parameter updates HIP {glob:.4f}, bf16-storage restatement {sglob:.4f}")
    assert glob < 2 * sglob, (glob, sglob)
    assert int(sd["batchnorm.num_batches_tracked"]) == int(fx["adam"]["batchnorm.num_batches_tracked"]) == 2
    for k in ("batchnorm.running_mean", "batchnorm.running_var"):
        dev, sim_dev = rel_err(sd[k], fx["adam"][k]), rel_err(p[k], fx["adam"][k])
        print(f"RNNBaseSTFTMask {tag} two Adam steps: {k} HIP {dev:.3e}, bf16-storage restatement {sim_dev:.3e}")
        assert dev < 2 * sim_dev, (k, dev, sim_dev)


# ------------------------------------------------------------------------------------------------------------------
# 3. dropout
# ------------------------------------------------------------------------------------------------------------------
def test_dropout():
    tag = "rnnmask_lstm_bi"
    fx = fixture(tag)
    args = kw(tag, drop_out=0.5)
    model, ws, est, grads = run_model(args, fx["sd"], fx["input"], fx["G"], seed=21)
    assert ws.dropping and int(ws.ctr_used[0]) == 0
    after = {k: v.double().cpu() for k, v in model.state_dict().items()}
    w = op_local(model, ws, fx["sd"], fx["input"], fx["G"], grads, after=after)          # includes: the device's mask == the twin's, bit for bit
    print(f"RNNBaseSTFTMask dropout 0.5 op-local (mask = the twin's): {w}")
    hd0 = ws.bufs["hd0"].clone()
    kept = float((hd0 != 0).float().mean())
    assert abs(kept - 0.5) < 4 * (0.25 / hd0.numel()) ** 0.5 + 0.01, kept             # (+ the few exact zeros of h itself)
    # the next step uses another mask
    est2 = model(fx["input"].cuda())
    torch.cuda.synchronize()
    assert int(ws.ctr_used[0]) == 1
    hd1 = ws.bufs["hd0"]
    m1 = R.device_mask(model.dropout_seed, 1, 0, ws.L, ws.T, model.cfg.Hout, 0.5).permute(1, 0, 2).cuda()
    assert torch.equal(hd1.view_as(m1) != 0, (ws.bufs["hs0"].view_as(m1) != 0) & (m1 != 0)) and not torch.equal(hd1 != 0, hd0 != 0)
    assert not torch.equal(est2.detach().cpu(), est)
    # two models built after the same torch.manual_seed: bit-identical outputs and gradients
    model_b, _, est_b, grads_b = run_model(args, fx["sd"], fx["input"], fx["G"], seed=21)
    assert model_b.dropout_seed == model.dropout_seed and torch.equal(est_b, est) and all(torch.equal(grads[k], grads_b[k]) for k in grads)
    model_c, _, est_c, _ = run_model(args, fx["sd"], fx["input"], fx["G"], seed=22)
    assert model_c.dropout_seed != model.dropout_seed and not torch.equal(est_c, est)
    # eval mode: no dropout
    from sehip.model import RNNBaseSTFTMask
    plain = RNNBaseSTFTMask(**kw(tag))
    plain.load_state_dict(model.state_dict())
    plain.cuda()
    with torch.no_grad():
        assert torch.equal(model.eval()(fx["input"].cuda()), plain.eval()(fx["input"].cuda()))
    # p = 1: zeros, not NaN
    _, ws1, est1, g1 = run_model(kw(tag, drop_out=1.0), fx["sd"], fx["input"], fx["G"])
    assert float(ws1.bufs["hd0"].abs().max()) == 0.0 and bool(torch.isfinite(est1).all()) and all(bool(torch.isfinite(v).all()) for v in g1.values())
    # nothing reaches layer 1, whose h then stays 0: only the head and BatchNorm's shift see a gradient
    assert float(g1["rnn.weight_ih_l0"].abs().max()) == 0.0 and float(g1["fc_layers.0.bias"].abs().max()) > 0.0


# ------------------------------------------------------------------------------------------------------------------
# 4. eval mode
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_eval_mode(tag):
    from sehip import SehipError
    from sehip.model import RNNBaseSTFTMask
    fx = fixture(tag)
    sd = dict(fx["sd"])
    sd.update(fx["run"])
    model = RNNBaseSTFTMask(**kw(tag))
    model.load_state_dict(sd)
    model.cuda().eval()
    with torch.no_grad():
        est = model(fx["input"].cuda()).cpu()
        sim = R.rnnmask_forward(sd, fx["input"], training=False, sim=R.Bf16Sim, **kw(tag))
    dev, sim_dev = rel_err(est, fx["est_eval"]), rel_err(sim, fx["est_eval"])
    print(f"RNNBaseSTFTMask {tag} eval: HIP {dev:.3e}, bf16-storage restatement {sim_dev:.3e}")
    assert dev < 2 * sim_dev, (dev, sim_dev)
    after = model.state_dict()
    assert all(torch.equal(after[k].cpu(), sd[k]) for k in fx["run"])                   # eval leaves the statistics alone
    out = model(fx["input"].cuda())
    with pytest.raises(SehipError, match="eval mode"):
        out.sum().backward()


# ------------------------------------------------------------------------------------------------------------------
# 5. edges, with guard bands around every buffer
# ------------------------------------------------------------------------------------------------------------------
EDGES = {
    "L1":         (dict(rnn_type="lstm", bidirectional=True, rnn_hidden=32, rnn_layer=2, num_spk=2, audio_channels=1, n_fft=64), (1, 1, 33, 40, 2)),
    "T1":         (dict(rnn_type="gru", bidirectional=True, rnn_hidden=64, rnn_layer=2, num_spk=1, audio_channels=2, n_fft=64), (4, 2, 33, 1, 2)),
    "T16":        (dict(rnn_type="lstm", bidirectional=False, rnn_hidden=32, rnn_layer=2, num_spk=2, audio_channels=2, n_fft=30), (2, 2, 16, 16, 2)),
    "T17_h96":    (dict(rnn_type="gru", bidirectional=True, rnn_hidden=96, rnn_layer=1, num_spk=3, audio_channels=1, n_fft=64), (3, 1, 33, 17, 2)),
    "lstm_uni_3": (dict(rnn_type="lstm", bidirectional=False, rnn_hidden=96, rnn_layer=3, num_spk=3, audio_channels=2, n_fft=30), (2, 2, 16, 17, 2)),
    "gru_bi_3":   (dict(rnn_type="gru", bidirectional=True, rnn_hidden=32, rnn_layer=3, num_spk=1, audio_channels=1, n_fft=64), (5, 1, 33, 35, 2)),
}


@pytest.mark.parametrize("name", sorted(EDGES))
def test_edges_with_guard_bands(name):
    args, shape = EDGES[name]
    args = dict(args, drop_out=0.25)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(*shape, generator=g)
    torch.manual_seed(31)
    from sehip.model import RNNBaseSTFTMask
    sd = RNNBaseSTFTMask(**args).state_dict()
    B, C, F, T, _ = shape
    G = torch.randn(B, args["num_spk"], C, F, T, 2, generator=g) / (x.numel() * args["num_spk"]) ** 0.5
    model, ws, est, grads = run_model(args, sd, x, G, guard=64, seed=31)
    assert ws.guard == 64 and ws.guards_intact() == [], ws.guards_intact()
    assert bool(torch.isfinite(est).all()) and all(bool(torch.isfinite(v).all()) for v in grads.values())
    if ws.L == 1:
        assert all(float(grads[k].abs().max()) == 0.0 for k in grads if "weight_hh" in k)  # no recurrent product at all
    w = op_local(model, ws, sd, x, G, grads, only="rnn_t")
    print(f"RNNBaseSTFTMask edge {name} {shape}: guard bands intact; recurrence and transposing kernels op-local: {w}")


# ------------------------------------------------------------------------------------------------------------------
# 6. Solver
# ------------------------------------------------------------------------------------------------------------------
def _solver_config(tag, deterministic, tmp):
    from sehip.utils import dict2obj
    return dict2obj({
        "seed": 10, "root": None, "ha": None,
        "model": dict(name="rnn-stft-mask", sources=["s1", "s2"], win_length=64, center=True, segment=0.02, **kw(tag)),
        "optim": {"optim": "adam", "lr": 3e-4, "beta1": 0.9, "beta2": 0.999, "loss": "mse", "clip_grad": 5, "pit": True, "pit_apply": True,
                  "load": True},
        "dset": {"name": "fixture", "norm": "z-score", "sample_rate": 16000},
        "solver": {"epochs": 1, "save_checkpoint_interval": 1, "all_steps": True, "total_steps": 0, "patience": 0, "root": str(tmp),
                   "resume": None, "preloaded_model": None, "cudnn_deterministic": deterministic, "use_graph": False,
                   "validation": {"interval": 1, "metric": "loss", "total_steps": 0}, "test": {"interval": 1}},
    })


def test_solver_three_steps_and_evaluate(tmp_path):
    from sehip import distrib
    from sehip.evaluate import evaluate
    from sehip.model import RNNBaseSTFTMask
    from sehip.solver import Solver, ScalarLog
    from sehip.utils import set_deterministic
    tag = "rnnmask_lstm_bi"
    fx = fixture(tag)
    _, ests, _, _ = sim_run(tag)
    names = R.param_names(fx["sd"])
    p = {k: (v.clone().requires_grad_(True) if k in names else v.clone()) for k, v in fx["sd"].items()}
    opt = torch.optim.Adam([p[k] for k in names], lr=3e-4, betas=(0.9, 0.999))
    sim_losses = []
    for _ in range(2):
        run = {}
        loss = torch.nn.functional.mse_loss(R.rnnmask_forward(p, fx["input"], sim=R.Bf16Sim, running=run, **kw(tag)), fx["target"])
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_([p[k] for k in names], 5)
        opt.step()
        p.update(run)
        sim_losses.append(loss.item())
    runs = []
    try:
        for deterministic in (False, True):
            cfg = _solver_config(tag, deterministic, tmp_path)
            model = distrib.get_model(cfg.model)
            assert isinstance(model, RNNBaseSTFTMask)
            model.load_state_dict(fx["sd"])
            hopt = distrib.get_optimizer(cfg.optim, model)
            solver = Solver(cfg, model, hopt, distrib.get_loss_function(cfg.optim), device="gpu", writer=ScalarLog())
            x, tgt = fx["input"].cuda(), fx["target"].cuda()
            assert solver._pit_applies(tgt)
            losses = [float(solver.train_step(x, tgt)[0]) for _ in range(3)]
            runs.append((losses, model.flat_params.detach().cpu().clone()))
            for i in range(2):
                loss_gate(f"Solver (cudnn_deterministic={deterministic}) loss {i + 1}", losses[i], sim_losses[i], float(fx["adam_losses"][i]), ests, fx)
            assert losses[2] < losses[0]
    finally:
        set_deterministic(False)
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])                # no atomics: the switch changes nothing
    wav = 0.1 * torch.randn(2, 2, 320 + 2 * 64 + 9, generator=torch.Generator().manual_seed(1))
    y = evaluate(wav, model, torch.device("cuda:0"), cfg)
    assert y.is_cuda and tuple(y.shape) == (2, 2, 2, wav.shape[-1]) and bool(torch.isfinite(y).all())


def test_pit_mse_at_stft_domain_row_counts():
    """optim.pit_apply on an STFT-domain estimate with more than 2^20 (batch x row) pairs of 2 samples, as the shipped step has: the value,
    the permutation and the gradient of the batch-level PIT (src/loss.py:58-100) against torch in float64"""
    from sehip.loss import mse_loss, pit_loss
    g = torch.Generator().manual_seed(3)
    shape = (4, 2, 2, 257, 520, 2)
    tgt = torch.randn(*shape, generator=g)
    est = (tgt.flip(1) + 0.3 * torch.randn(*shape, generator=g)).cuda().requires_grad_(True)      # the speakers come out swapped
    loss = pit_loss(est, tgt.cuda(), mse_loss)
    loss.backward()
    e64 = est.detach().double().cpu().requires_grad_(True)
    pair = lambda i, j: ((e64[:, i] - tgt[:, j].double()) ** 2).mean()
    want = torch.minimum((pair(0, 0) + pair(1, 1)) / 2, (pair(0, 1) + pair(1, 0)) / 2)
    want.backward()
    assert float(pair(0, 1) + pair(1, 0)) < float(pair(0, 0) + pair(1, 1))
    assert abs(float(loss) - float(want)) < 1e-5 * float(want) and rel_err(est.grad.cpu(), e64.grad) < 1e-5


# ------------------------------------------------------------------------------------------------------------------
# 7. the shipped width
# ------------------------------------------------------------------------------------------------------------------
def test_shipped_width():
    args = dict(rnn_type="lstm", bidirectional=True, rnn_hidden=896, rnn_layer=3, num_spk=2, audio_channels=2, n_fft=512, hop_length=128, drop_out=0.5)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 2, 257, 33, 2, generator=g)
    G = torch.randn(2, 2, 2, 257, 33, 2, generator=g) / (2 * x.numel()) ** 0.5
    torch.manual_seed(41)
    from sehip.model import RNNBaseSTFTMask
    sd = RNNBaseSTFTMask(**args).state_dict()
    model, ws, est, grads = run_model(args, sd, x, G, seed=41)
    assert bool(torch.isfinite(est).all()) and all(bool(torch.isfinite(v).all()) for v in grads.values())
    w = op_local(model, ws, sd, x, G, grads, only={"steps", "bsteps", "head"})
    print(f"RNNBaseSTFTMask shipped width (K = 896 recurrent steps, head of 514 columns) op-local: {w}")
    masks = [R.device_mask(model.dropout_seed, 0, k, ws.L, ws.T, 1792, 0.5) for k in range(2)]
    with torch.no_grad():
        want = R.rnnmask_forward(sd, x, drop_masks=masks, **args)
    print(f"RNNBaseSTFTMask shipped width: est deviates {rel_err(est, want):.3e} from the fp32 restatement under the same masks (not gated)")
