#!/usr/bin/env python3
"""tests/golden/wavunet_{l3_c8,l2_c24}{,_train}.npz from the IMPORTED reference (the path of a reference checkout is
the first argument or $SEHIP_REFERENCE).  Data only: nothing of the reference's program text is written.

  wavunet_l3_c8 : unet_nlayers=3, channels_interval=8, input [2, 1, 200] -- levels of 200 / 100 / 50 frames and a middle block of 25,
                  an odd length: the interpolation's clamped last neighbour and non-trivial weights
  wavunet_l2_c24: unet_nlayers=2, channels_interval=24, input [3, 1, 132] -- the default's 24-wide first layer, 72- / 48-channel
                  concatenations, a middle block of 33 frames, three utterances
Model seed 7, data seed 8, seeded non-trivial BatchNorm affine terms.  Per file: the state dict before any forward pass (sd.*), the
input (mix), a target (the untrained network's own output + 30 % noise, as in the ConvTasNet fixtures), every layer's output of one
training-mode forward pass (tap.enc{l} / tap.middle / tap.dec{i}, and tap.up{i}: F.interpolate of the tensor in front of decoder i),
its output (est), the running statistics and counters after that pass (run.*), the eval-mode output with those statistics
(est_eval), a fixed upstream gradient G and the gradients of <est, G>
(gradG.*); in the companion file *_train.npz (a state dict four times over does not fit one committed file): the SI-SNR loss and its
gradients (loss, grad.*), the losses and the final state dict (adam_losses, adam.*) of two Adam steps (lr 3e-4, clip_grad_norm_ 5 as
src/solver.py:487-492).
Run:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_wavunet.py /path/to/reference"""
import copy
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.dont_write_bytecode = True
REFERENCE = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SEHIP_REFERENCE")
if not REFERENCE:
    sys.exit("usage: gen_golden_wavunet.py /path/to/reference")
sys.path.insert(0, REFERENCE)
GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
FIXTURES = {"wavunet_l3_c8": dict(unet_nlayers=3, channels_interval=8, shape=(2, 1, 200)),
            "wavunet_l2_c24": dict(unet_nlayers=2, channels_interval=24, shape=(3, 1, 132))}

from src.model.wav_unet import WavUnet  # noqa: E402
from src.loss import loss_sisdr  # noqa: E402


def build(out_path, unet_nlayers, channels_interval, shape):
    torch.manual_seed(7)
    model = WavUnet(unet_nlayers=unet_nlayers, channels_interval=channels_interval).train()
    g = torch.Generator().manual_seed(8)
    with torch.no_grad():   # non-trivial BatchNorm affine terms
        for name, prm in model.named_parameters():
            if name.endswith("1.weight"):
                prm.copy_(1 + 0.2 * torch.randn(prm.shape, generator=g))
            if name.endswith("1.bias"):
                prm.copy_(0.1 * torch.randn(prm.shape, generator=g))
    mix = 0.3 * torch.randn(*shape, generator=g)
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    with torch.no_grad():   # (on a copy: the fixture's model has seen no batch before its first forward pass)
        e0 = copy.deepcopy(model)(mix)
    tgt = e0 + 0.3 * e0.std() * torch.randn(e0.shape, generator=g)
    G = torch.randn(e0.shape, generator=g) / e0.numel() ** 0.5
    out = {"sd." + k: v.numpy() for k, v in sd0.items()}
    taps = {}
    hooks = [model.middle.register_forward_hook(lambda m, a, o: taps.__setitem__("middle", o.detach().clone()))]
    for i in range(unet_nlayers):
        hooks.append(model.encoder[i].register_forward_hook(lambda m, a, o, i=i: taps.__setitem__(f"enc{i}", o.detach().clone())))
        hooks.append(model.decoder[i].register_forward_hook(lambda m, a, o, i=i: taps.__setitem__(f"dec{i}", o.detach().clone())))
    est = model(mix)
    for h in hooks:
        h.remove()
    prev = taps["middle"]
    for i in range(unet_nlayers):
        taps[f"up{i}"] = F.interpolate(prev, scale_factor=2, mode="linear", align_corners=True)
        prev = taps[f"dec{i}"]
    for k, v in model.state_dict().items():
        if k.endswith(("running_mean", "running_var", "num_batches_tracked")):
            out["run." + k] = v.detach().clone().numpy()
    with torch.no_grad():
        est_eval = copy.deepcopy(model).eval()(mix)
    loss = loss_sisdr(est, tgt)
    loss.backward()
    for k, v in taps.items():
        out["tap." + k] = v.numpy()
    out.update(mix=mix.numpy(), target=tgt.numpy(), est=est.detach().numpy(), est_eval=est_eval.numpy(), loss=np.float32(loss.item()),
               G=G.numpy())
    for k, prm in model.named_parameters():
        out["grad." + k] = prm.grad.clone().numpy()
    m2 = WavUnet(unet_nlayers=unet_nlayers, channels_interval=channels_interval).train()
    m2.load_state_dict(sd0)
    (m2(mix) * G).sum().backward()
    for k, prm in m2.named_parameters():
        out["gradG." + k] = prm.grad.clone().numpy()
    m3 = WavUnet(unet_nlayers=unet_nlayers, channels_interval=channels_interval).train()
    m3.load_state_dict(sd0)
    opt = torch.optim.Adam(m3.parameters(), lr=3e-4, betas=(0.9, 0.999))
    losses = []
    for _ in range(2):
        l3 = loss_sisdr(m3(mix), tgt)
        opt.zero_grad()
        l3.backward()
        torch.nn.utils.clip_grad_norm_(m3.parameters(), 5)
        opt.step()
        losses.append(l3.item())
    out["adam_losses"] = np.asarray(losses, dtype=np.float32)
    for k, v in m3.state_dict().items():
        out["adam." + k] = v.detach().clone().numpy()
    # two files per fixture, each below the 1 MiB a committed file may have: the forward pass and <est, G> | the loss's gradients and Adam
    train = {k: out.pop(k) for k in list(out) if k.startswith(("grad.", "adam.")) or k in ("loss", "adam_losses")}
    train_path = out_path[:-len(".npz")] + "_train.npz"
    np.savez_compressed(out_path, **out)
    np.savez_compressed(train_path, **train)
    print(os.path.basename(out_path), len(out), "+", len(train), "entries; est", tuple(est.shape), "loss", loss.item(), "adam", losses,
          sum(v.numel() for v in sd0.values()), "state elements", os.path.getsize(out_path), "+", os.path.getsize(train_path), "bytes")


if __name__ == "__main__":
    for tag, kw in FIXTURES.items():
        build(os.path.join(GOLDEN, tag + ".npz"), **kw)
