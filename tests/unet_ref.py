"""fp32 / float64 restatement of the U-Net on the power spectrogram, training and eval -- TEST INFRASTRUCTURE ONLY (reference:
src/model/unet.py:9-146).

Written from the math: amp = re^2 + im^2; per encoder block (Conv3x3 pad 1 without bias, BatchNorm2d, LeakyReLU(0.01)) twice, Dropout(p)
(p > 0 in the last block only), MaxPool2d(2); the pooled tensor is the next block's input and the skip.  A middle double convolution
with Dropout.  Decoder 0 concatenates [middle | last skip]; the others ConvTranspose2d(k = 2, s = 2, bias, C -> C / 2), a zero pad at
the far end up to the skip's size, cat([up | skip]), a double convolution.  The head: ConvTranspose2d(16 -> 8), pad, cat([up | amp]), a
double convolution (8 + uc) -> uc -> uc, out = mix * x[..., None].  H = F, W = T.
Hooks: taps= (dict: "amp", "enc{i}", "middle", "up{n}", "dec{n}", "upo", "head"), running= (dict that receives the running statistics
and counters after a training forward), sim= (Bf16Sim / NoSim: bf16 round-trips exactly where the HIP path stores bf16 -- amp, every
convolution output, every first-half activation, the pooled tensors, the middle's and the decoders' outputs, every `up`, and every
packed weight; the transposed convolutions' biases stay fp32), drop= (dict(seed, counter, p): the device generator's twin at the two
dropout sites, on the element's index in the channels-last full-resolution tensor).
The pool takes the first maximum in the reference's scan order (F offset outer, T offset inner) and floors odd sizes.
Pinned against vectors of the imported reference by tests/test_unet_host.py (tests/golden/unet_*.npz, tools/gen_golden_unet.py)."""
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle.dccrn_oracle import Bf16Sim, NoSim   # noqa: F401  (re-exported for the tests)

EPS, MOMENTUM, SLOPE = 1e-5, 0.1, 0.01
DROP_ENCODER, DROP_MIDDLE = 0, 1
FIXTURES = {"unet_l1_c1": dict(unet_layer=1, unet_channels=1, shape=(3, 1, 9, 6, 2)),
            "unet_l2_c2": dict(unet_layer=2, unet_channels=2, shape=(3, 2, 21, 14, 2))}
GOLDEN_MASK = 0x9E3779B9


# ---- the dropout generator's twin (csrc/drop.h), written out here so that the restatement stands on its own ---------------------------
def _mix(x):
    x = np.asarray(x, dtype=np.uint64) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & 0xFFFFFFFF
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def drop_keep_mask(seed, counter, layer, n, p):
    """bool [n]: kept elements 0 .. n-1 of site `layer` at step counter `counter`; kept when the top 24 bits are >= round(p 2^24)"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    lo, hi = seed & 0xFFFFFFFF, seed >> 32
    key = _mix(lo ^ int(_mix(hi ^ int(_mix(((int(counter) & 0xFFFFFFFF) * GOLDEN_MASK + int(layer)) & 0xFFFFFFFF)))))
    bits = _mix((_mix(np.arange(n, dtype=np.uint64) ^ key) + GOLDEN_MASK) & 0xFFFFFFFF)
    return (bits >> 8) >= int(round(float(p) * (1 << 24)))


def keep_nchw(drop, site, shape):
    """the keep mask of a [R, C, F, T] tensor: the device indexes it channels-last, [R][T][F][C]"""
    r, c, f, t = shape
    m = drop_keep_mask(drop["seed"], drop["counter"], site, r * t * f * c, drop["p"]).reshape(r, t, f, c)
    return torch.from_numpy(np.ascontiguousarray(m.transpose(0, 3, 2, 1)))


def dropout(z, drop, site):
    if drop is None or drop["p"] <= 0.0:
        return z
    scale = 0.0 if drop["p"] >= 1.0 else 1.0 / (1.0 - drop["p"])
    return z * keep_nchw(drop, site, z.shape).to(z.dtype) * scale


# ---- MaxPool2d(2) with the tie rule -----------------------------------------------------------------------------------------------------
def pool_codes(z):
    """int64 [R, C, F // 2, T // 2]: 2 (F offset) + (T offset) of the first maximum of every window in the order (0,0), (0,1), (1,0), (1,1)
    of (F offset, T offset); a later candidate wins only when it is strictly greater"""
    f2, t2 = z.shape[2] // 2, z.shape[3] // 2
    w = z.detach()[:, :, :2 * f2, :2 * t2]
    cand = [w[:, :, df::2, dt::2] for df in (0, 1) for dt in (0, 1)]
    best, code = cand[0], torch.zeros(cand[0].shape, dtype=torch.int64)
    for k in (1, 2, 3):
        m = cand[k] > best
        best, code = torch.where(m, cand[k], best), torch.where(m, torch.full_like(code, k), code)
    return code


def max_pool2(z, codes=None):
    f2, t2 = z.shape[2] // 2, z.shape[3] // 2
    w = z[:, :, :2 * f2, :2 * t2]
    cand = torch.stack([w[:, :, df::2, dt::2] for df in (0, 1) for dt in (0, 1)], 0)
    code = pool_codes(z)
    if codes is not None:
        codes.append(code)
    return cand.gather(0, code[None])[0]


# ---- the network ---------------------------------------------------------------------------------------------------------------------------
def bn_lrelu(y, p, pre, training, running=None):
    """BatchNorm2d over (items, F, T) + LeakyReLU(0.01); training: batch moments (biased variance), running statistics as nn.BatchNorm2d"""
    if training:
        mean, var = y.mean(dim=(0, 2, 3)), y.var(dim=(0, 2, 3), unbiased=False)
        if running is not None:
            n = y.shape[0] * y.shape[2] * y.shape[3]
            running[pre + "running_mean"] = ((1 - MOMENTUM) * p[pre + "running_mean"] + MOMENTUM * mean).detach()
            running[pre + "running_var"] = ((1 - MOMENTUM) * p[pre + "running_var"] + MOMENTUM * var * n / (n - 1)).detach()
            running[pre + "num_batches_tracked"] = p[pre + "num_batches_tracked"] + 1
    else:
        mean, var = p[pre + "running_mean"].to(y.dtype), p[pre + "running_var"].to(y.dtype)
    v = lambda a: a[None, :, None, None]
    return F.leaky_relu((y - v(mean)) / torch.sqrt(v(var) + EPS) * v(p[pre + "weight"]) + v(p[pre + "bias"]), SLOPE)


def double_conv(x, p, pre, training, running, sim):
    """-> the second activation in fp32 (the caller stores it, pools it or masks with it)"""
    y1 = sim.act(F.conv2d(x, sim.weight(p[pre + "0.weight"]), padding=1))
    z1 = sim.act(bn_lrelu(y1, p, pre + "1.", training, running))
    y2 = sim.act(F.conv2d(z1, sim.weight(p[pre + "3.weight"]), padding=1))
    return bn_lrelu(y2, p, pre + "4.", training, running)


def up_pad(x, p, pre, like, sim):
    u = F.conv_transpose2d(x, sim.weight(p[pre + "weight"]), p[pre + "bias"], stride=2)
    return sim.act(F.pad(u, [0, like.shape[3] - u.shape[3], 0, like.shape[2] - u.shape[2]]))


def unet_forward(p, mix, unet_channels, unet_layer=4, training=True, taps=None, running=None, sim=NoSim, drop=None, codes=None):
    """mix [R, uc, F, T, 2] -> [R, uc, F, T, 2]"""
    L = unet_layer
    assert mix.dim() == 5 and mix.shape[1] == unet_channels
    if not training:
        drop = None
    tap = (lambda k, v: taps.__setitem__(k, v)) if taps is not None else (lambda k, v: None)
    amp = sim.act(mix[..., 0] ** 2 + mix[..., 1] ** 2)
    tap("amp", amp)
    x, skips = amp, []
    for l in range(L):
        z = double_conv(x, p, f"encoder.{l}.maxpool_conv.0.double_conv.", training, running, sim)
        if l == L - 1:
            z = dropout(z, drop, DROP_ENCODER)
        x = sim.act(max_pool2(z, codes))
        tap(f"enc{l}", x)
        skips.append(x)
    x = sim.act(dropout(double_conv(x, p, "middle.double_conv.", training, running, sim), drop, DROP_MIDDLE))
    tap("middle", x)
    for n in range(L):
        skip = skips.pop()
        if n > 0:
            x = up_pad(x, p, f"decoder.{n}.up.", skip, sim)
            tap(f"up{n}", x)
        x = sim.act(double_conv(torch.cat([x, skip], 1), p, f"decoder.{n}.conv.double_conv.", training, running, sim))
        tap(f"dec{n}", x)
    u = up_pad(x, p, "outconv.up.", amp, sim)
    tap("upo", u)
    m = double_conv(torch.cat([u, amp], 1), p, "outconv.conv.double_conv.", training, running, sim)
    tap("head", m)
    return mix * m[..., None]


def param_names(sd):
    return [k for k in sd if not k.endswith(("running_mean", "running_var", "num_batches_tracked"))]


def fixed_g_grads(sd, mix, G, sim=NoSim, **kw):
    """({name: gradient of <est, G>}, est) of the restatement"""
    names = param_names(sd)
    p = {k: (v.detach().clone().requires_grad_(True) if k in names else v.detach().clone()) for k, v in sd.items()}
    est = unet_forward(p, mix, sim=sim, **kw)
    (est * G).sum().backward()
    return {k: p[k].grad for k in names}, est.detach()


def adam_steps(sd, mix, target, steps=2, lr=3e-4, clip=5.0, sim=NoSim, **kw):
    """(losses, final state dict) of `steps` Adam steps on the mse loss with clip_grad_norm_, as src/solver.py:487-492 does them"""
    names = param_names(sd)
    p = {k: (v.detach().clone().requires_grad_(True) if k in names else v.detach().clone()) for k, v in sd.items()}
    opt = torch.optim.Adam([p[k] for k in names], lr=lr, betas=(0.9, 0.999))
    losses = []
    for _ in range(steps):
        run = {}
        loss = F.mse_loss(unet_forward(p, mix, running=run, sim=sim, **kw), target)
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_([p[k] for k in names], clip)
        opt.step()
        p.update(run)
        losses.append(loss.item())
    return losses, {k: v.detach() for k, v in p.items()}


def load_fixture(path):
    z = dict(np.load(path))
    for suffix in ("_gradG", "_train", "_adam"):      # files of their own: a committed file holds at most 1 MiB
        z.update(np.load(path[:-len(".npz")] + suffix + ".npz"))
    g = lambda pre: {k[len(pre):]: torch.from_numpy(z[k]) for k in z if k.startswith(pre)}
    out = dict(sd=g("sd."), tap=g("tap."), run=g("run."), grad=g("grad."), gradG=g("gradG."), adam=g("adam."))
    for k in ("mix", "target", "est", "est_eval", "G"):
        out[k] = torch.from_numpy(z[k])
    out["loss"] = float(z["loss"])
    out["adam_losses"] = [float(v) for v in z["adam_losses"]]
    return out


_FX = {}


def fixture(tag):
    if tag not in _FX:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        _FX[tag] = load_fixture(os.path.join(root, "tests", "golden", tag + ".npz"))
    return _FX[tag]


def model_kw(tag):
    return dict(unet_channels=FIXTURES[tag]["unet_channels"], unet_layer=FIXTURES[tag]["unet_layer"])
