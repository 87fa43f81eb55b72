#!/usr/bin/env python3
"""tests/golden/unet_{l1_c1,l2_c2}{,_gradG,_train,_adam}.npz from the IMPORTED reference (the path of a reference checkout is the
first argument or $SEHIP_REFERENCE).  Data only: nothing of the reference's program text is written.

  unet_l1_c1: unet_layer=1, unet_channels=1, input [3, 1, 9, 6, 2] -- the first-decoder form only; F is odd, so the head's far-end pad
              row is live
  unet_l2_c2: unet_layer=2, unet_channels=2, input [3, 2, 21, 14, 2] -- F 21 -> 10 -> 5 and T 14 -> 7 -> 3: an odd axis at each level,
              a middle decoder whose transposed convolution lands in a buffer with a padded column, two input channels, three items
Model seed 7, data seed 8, seeded non-trivial BatchNorm affine terms.  Every nn.Dropout of the built reference model has p = 0.0 set:
torch's dropout stream cannot be matched by a counter-based generator (the decision of the rnnmask_* fixtures).  The reference's
Up.forward prints shapes: its stdout is swallowed.

Per fixture, four files (one state dict of l2_c2 is 478 kB and a committed file holds at most 1 MiB):
  *.npz        the state dict before any forward pass (sd.*), the input (mix), a target (the untrained output + 30 % noise), the
               taps of one training-mode forward pass (tap.amp, tap.enc{i}: the pooled skips, tap.middle, tap.up{n}: the transposed
               convolution's output after its pad, n >= 1, tap.dec{n}, tap.upo, tap.head: the mask), est, the running statistics and
               counters after that pass (run.*), the eval-mode output with those statistics (est_eval), a fixed upstream gradient G
  *_gradG.npz  the gradients of <est, G> (gradG.*)
  *_train.npz  the mse loss against the target and its gradients (loss, grad.*)
  *_adam.npz   the losses and the final state dict of two Adam steps (lr 3e-4, clip_grad_norm_ 5 as src/solver.py:487-492)
Run:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_unet.py /path/to/reference"""
import contextlib
import copy
import io
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.dont_write_bytecode = True
REFERENCE = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SEHIP_REFERENCE")
if not REFERENCE:
    sys.exit("usage: gen_golden_unet.py /path/to/reference")
sys.path.insert(0, REFERENCE)
GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
FIXTURES = {"unet_l1_c1": dict(unet_layer=1, unet_channels=1, shape=(3, 1, 9, 6, 2)),
            "unet_l2_c2": dict(unet_layer=2, unet_channels=2, shape=(3, 2, 21, 14, 2))}

from src.model.unet import UNet  # noqa: E402


def quiet(fn, *a):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a)


def make(unet_layer, unet_channels):
    m = UNet(unet_channels=unet_channels, unet_layer=unet_layer, bilinear=False).train()
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    return m


def build(out_path, unet_layer, unet_channels, shape):
    torch.manual_seed(7)
    model = make(unet_layer, unet_channels)
    g = torch.Generator().manual_seed(8)
    with torch.no_grad():   # non-trivial BatchNorm affine terms
        for name, prm in model.named_parameters():
            if prm.dim() == 1 and name.endswith((".1.weight", ".4.weight")):
                prm.copy_(1 + 0.2 * torch.randn(prm.shape, generator=g))
            if prm.dim() == 1 and name.endswith((".1.bias", ".4.bias")):
                prm.copy_(0.1 * torch.randn(prm.shape, generator=g))
    mix = torch.randn(*shape, generator=g)
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    with torch.no_grad():   # (on a copy: the fixture's model has seen no batch before its first forward pass)
        e0 = quiet(copy.deepcopy(model), mix)
    tgt = e0 + 0.3 * e0.std() * torch.randn(e0.shape, generator=g)
    G = torch.randn(e0.shape, generator=g) / e0.numel() ** 0.5
    out = {"sd." + k: v.numpy() for k, v in sd0.items()}
    taps, ups = {}, {}
    keep = lambda d, k: (lambda m, a, o: d.__setitem__(k, o.detach().clone()))
    hooks = [model.middle.register_forward_hook(keep(taps, "middle")), model.outconv.register_forward_hook(keep(taps, "head")),
             model.outconv.up.register_forward_hook(keep(ups, "upo"))]
    for i in range(unet_layer):
        hooks.append(model.encoder[i].register_forward_hook(keep(taps, f"enc{i}")))
        hooks.append(model.decoder[i].register_forward_hook(keep(taps, f"dec{i}")))
        if i > 0:
            hooks.append(model.decoder[i].up.register_forward_hook(keep(ups, f"up{i}")))
    est = quiet(model, mix)
    for h in hooks:
        h.remove()
    taps["amp"] = mix[..., 0] ** 2 + mix[..., 1] ** 2
    for k, u in ups.items():          # the far-end pad up to the skip's (the input's) size
        like = taps["amp"] if k == "upo" else taps[f"enc{unet_layer - 1 - int(k[2:])}"]
        taps[k] = F.pad(u, [0, like.shape[3] - u.shape[3], 0, like.shape[2] - u.shape[2]])
    for k, v in model.state_dict().items():
        if k.endswith(("running_mean", "running_var", "num_batches_tracked")):
            out["run." + k] = v.detach().clone().numpy()
    with torch.no_grad():
        est_eval = quiet(copy.deepcopy(model).eval(), mix)
    loss = F.mse_loss(est, tgt)
    loss.backward()
    for k, v in taps.items():
        out["tap." + k] = v.numpy()
    out.update(mix=mix.numpy(), target=tgt.numpy(), est=est.detach().numpy(), est_eval=est_eval.numpy(), loss=np.float32(loss.item()),
               G=G.numpy())
    for k, prm in model.named_parameters():
        out["grad." + k] = prm.grad.clone().numpy()
    m2 = make(unet_layer, unet_channels)
    m2.load_state_dict(sd0)
    (quiet(m2, mix) * G).sum().backward()
    for k, prm in m2.named_parameters():
        out["gradG." + k] = prm.grad.clone().numpy()
    m3 = make(unet_layer, unet_channels)
    m3.load_state_dict(sd0)
    opt = torch.optim.Adam(m3.parameters(), lr=3e-4, betas=(0.9, 0.999))
    losses = []
    for _ in range(2):
        l3 = F.mse_loss(quiet(m3, mix), tgt)
        opt.zero_grad()
        l3.backward()
        torch.nn.utils.clip_grad_norm_(m3.parameters(), 5)
        opt.step()
        losses.append(l3.item())
    out["adam_losses"] = np.asarray(losses, dtype=np.float32)
    for k, v in m3.state_dict().items():
        out["adam." + k] = v.detach().clone().numpy()
    parts = {"_gradG": {k: out.pop(k) for k in list(out) if k.startswith("gradG.")},
             "_train": {k: out.pop(k) for k in list(out) if k.startswith("grad.") or k == "loss"},
             "_adam": {k: out.pop(k) for k in list(out) if k.startswith("adam.") or k == "adam_losses"}, "": out}
    sizes = []
    for suffix, d in parts.items():
        path = out_path[:-len(".npz")] + suffix + ".npz"
        np.savez_compressed(path, **d)
        sizes.append(os.path.getsize(path))
    print(os.path.basename(out_path), "est", tuple(est.shape), "loss", loss.item(), "adam", losses,
          sum(p.numel() for p in model.parameters()), "parameters", sizes, "bytes")


if __name__ == "__main__":
    for tag, kw in FIXTURES.items():
        build(os.path.join(GOLDEN, tag + ".npz"), **kw)
