"""fp32 / float64 restatement of Wave-U-Net, training and eval -- TEST INFRASTRUCTURE ONLY (reference: src/model/wav_unet.py:8-110).

Written from the math: Conv1d(k = 15, pad 7) + BatchNorm1d + LeakyReLU(0.1) per encoder layer, `[::2]` between them, a middle block of the
same form, then per decoder layer the align-corners x2 linear interpolation, the concatenation with the encoder's tensor of that
length, Conv1d(k = 5, pad 2) + BatchNorm1d + LeakyReLU(0.1); the head is a 1x1 convolution of cat([o, input]) and tanh.
Hooks: taps= (dict: "enc{l}", "middle", "up{i}", "dec{i}"), running= (dict that receives the running statistics and counters after a
training forward), sim= (oracle.convtasnet_oracle.Bf16Sim / NoSim: bf16 round-trips exactly where the HIP path stores bf16 -- every
convolution output y, every encoder z, every upsampled tensor, the last decoder layer's z, and every packed weight, i.e. every
convolution weight but the first layer's and the head's, which the HIP path reads in fp32).
Pinned against vectors of the imported reference by tests/test_wavunet_host.py (tests/golden/wavunet_*.npz, tools/gen_golden_wavunet.py)."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle.convtasnet_oracle import Bf16Sim, NoSim   # noqa: F401  (re-exported for the tests)

EPS, MOMENTUM, SLOPE = 1e-5, 0.1, 0.1
FIXTURES = {"wavunet_l3_c8": dict(unet_nlayers=3, channels_interval=8, shape=(2, 1, 200)),
            "wavunet_l2_c24": dict(unet_nlayers=2, channels_interval=24, shape=(3, 1, 132))}


def up2_table(t_in):
    """(left frame, right frame, weight of the right frame) per output position of the align-corners x2 linear interpolation:
    position p of 2 t_in sits at p (t_in - 1) / (2 t_in - 1) source frames; in integers p (t_in - 1) = i (2 t_in - 1) + r"""
    p = np.arange(2 * t_in, dtype=np.int64)
    den = 2 * t_in - 1
    i0 = p * (t_in - 1) // den
    return i0, np.minimum(i0 + 1, t_in - 1), (p * (t_in - 1) - i0 * den) / den


def upsample2(z):
    i0, i1, w = up2_table(z.shape[-1])
    w = torch.as_tensor(w, dtype=z.dtype)
    return z[..., torch.as_tensor(i0)] * (1 - w) + z[..., torch.as_tensor(i1)] * w


def bn_lrelu(y, p, pre, training, running=None):
    """BatchNorm1d over (batch, time) + LeakyReLU(0.1); training: batch moments (biased variance), running statistics as nn.BatchNorm1d"""
    if training:
        mean, var = y.mean(dim=(0, 2)), y.var(dim=(0, 2), unbiased=False)
        if running is not None:
            n = y.shape[0] * y.shape[2]
            running[pre + "running_mean"] = ((1 - MOMENTUM) * p[pre + "running_mean"] + MOMENTUM * mean).detach()
            running[pre + "running_var"] = ((1 - MOMENTUM) * p[pre + "running_var"] + MOMENTUM * var * n / (n - 1)).detach()
            running[pre + "num_batches_tracked"] = p[pre + "num_batches_tracked"] + 1
    else:
        mean, var = p[pre + "running_mean"].to(y.dtype), p[pre + "running_var"].to(y.dtype)
    o = (y - mean[None, :, None]) / torch.sqrt(var[None, :, None] + EPS) * p[pre + "weight"][None, :, None] + p[pre + "bias"][None, :, None]
    return F.leaky_relu(o, SLOPE)


def wavunet_forward(p, x, unet_nlayers=12, channels_interval=24, training=True, taps=None, running=None, sim=NoSim):
    """x [B, 1, T] -> [B, 1, T]"""
    n = unet_nlayers
    tmp, o = [], x
    for l in range(n):
        q = f"encoder.{l}.main."
        w = p[q + "0.weight"] if l == 0 else sim.weight(p[q + "0.weight"])      # the first layer runs on the fp32 waveform in fp32
        y = sim.act(F.conv1d(o, w, p[q + "0.bias"], padding=7))
        z = sim.act(bn_lrelu(y, p, q + "1.", training, running))
        if taps is not None:
            taps[f"enc{l}"] = z
        tmp.append(z)
        o = z[:, :, ::2]
    y = sim.act(F.conv1d(o, sim.weight(p["middle.0.weight"]), p["middle.0.bias"], padding=7))
    o = bn_lrelu(y, p, "middle.1.", training, running)
    if taps is not None:
        taps["middle"] = o
    for i in range(n):
        q = f"decoder.{i}.main."
        up = sim.act(upsample2(o))
        if taps is not None:
            taps[f"up{i}"] = up
        y = sim.act(F.conv1d(torch.cat([up, tmp[n - 1 - i]], dim=1), sim.weight(p[q + "0.weight"]), p[q + "0.bias"], padding=2))
        o = bn_lrelu(y, p, q + "1.", training, running)
        if taps is not None:
            taps[f"dec{i}"] = o
    o = sim.act(o)                                                               # the head reads the last layer's z from bf16 storage
    return torch.tanh(F.conv1d(torch.cat([o, x], dim=1), p["out.0.weight"], p["out.0.bias"]))


def param_names(sd):
    return [k for k in sd if not k.endswith(("running_mean", "running_var", "num_batches_tracked"))]


def fixed_g_grads(sd, x, G, sim=NoSim, **kw):
    """({name: gradient of <est, G>}, est) of the restatement"""
    names = param_names(sd)
    p = {k: (v.detach().clone().requires_grad_(True) if k in names else v.detach().clone()) for k, v in sd.items()}
    est = wavunet_forward(p, x, sim=sim, **kw)
    (est * G).sum().backward()
    return {k: p[k].grad for k in names}, est.detach()


def load_fixture(path):
    z = dict(np.load(path))
    z.update(np.load(path[:-len(".npz")] + "_train.npz"))      # the loss's gradients and the Adam steps: a file of their own (size)
    g = lambda pre: {k[len(pre):]: torch.from_numpy(z[k]) for k in z if k.startswith(pre)}
    out = dict(sd=g("sd."), tap=g("tap."), run=g("run."), grad=g("grad."), gradG=g("gradG."), adam=g("adam."))
    for k in ("mix", "target", "est", "est_eval", "G"):
        out[k] = torch.from_numpy(z[k])
    out["loss"] = float(z["loss"])
    out["adam_losses"] = [float(v) for v in z["adam_losses"]]
    return out
