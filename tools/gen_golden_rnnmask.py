#!/usr/bin/env python3
"""tests/golden/rnnmask_{lstm_bi,gru_uni}{,_train}.npz from the IMPORTED reference (the path of a reference checkout is the first
argument or $SEHIP_REFERENCE).  Data only: nothing of the reference's program text is written.

  rnnmask_lstm_bi: rnn_type='lstm', bidirectional, rnn_hidden=32, rnn_layer=2, num_spk=2, audio_channels=2, n_fft=64, input
                   [3, 2, 33, 21, 2] -- six recurrence steps over 21 rows (one full 16-row tile and a ragged one), F = 33 (padding)
  rnnmask_gru_uni: rnn_type='gru', unidirectional, rnn_hidden=64, rnn_layer=2, num_spk=1, audio_channels=1, n_fft=64, input
                   [2, 1, 33, 17, 2] -- two steps, the shortest sequence with a recurrent product; one speaker
Both with drop_out=0.0 (torch's dropout stream cannot be matched).  Model seed 7, data seed 8, seeded non-trivial BatchNorm affine terms.
Per fixture: the state dict before any forward pass (sd.*), the input, a target (the untrained output + 30 % noise), taps after every
RNN layer (tap.rnn{k} [L, N, Hout], from single-layer torch modules holding the same weights), after BatchNorm (tap.bn [L, N, Hout]) and
after the head (tap.head [L, N, S F]), est, the running statistics after one training pass (run.*), est_eval, a fixed upstream
gradient G and the gradients of <est, G> (gradG.*); in *_train.npz the mse loss and its gradients (loss, grad.*), the losses and the
final state of two Adam steps (adam_losses, adam.*; lr 3e-4, clip_grad_norm_ 5 as src/solver.py:487-492).
Run:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_rnnmask.py /path/to/reference"""
import copy
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.dont_write_bytecode = True
REFERENCE = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SEHIP_REFERENCE")
if not REFERENCE:
    sys.exit("usage: gen_golden_rnnmask.py /path/to/reference")
sys.path.insert(0, REFERENCE)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")

from src.model.stft_rnn import RNNBaseSTFTMask  # noqa: E402
from rnnmask_ref import FIXTURES  # noqa: E402  (the fixtures' configurations: one list for the generator and the tests)


def layer_taps(model, inputs, kw):
    """outputs [L, N, Hout] of every RNN layer: single-layer torch modules with the model's weights, chained (drop_out = 0)"""
    cls = torch.nn.LSTM if kw["rnn_type"] == "lstm" else torch.nn.GRU
    x = model.ampltude(inputs)
    b, c, f, t = x.shape
    x = x.reshape(b * c, f, t).transpose(1, 2)
    taps = {}
    for k in range(kw["rnn_layer"]):
        one = cls(input_size=x.shape[-1], hidden_size=kw["rnn_hidden"], num_layers=1, bias=False, bidirectional=kw["bidirectional"])
        with torch.no_grad():
            for sfx in ("", "_reverse")[:2 if kw["bidirectional"] else 1]:
                getattr(one, "weight_ih_l0" + sfx).copy_(getattr(model.rnn, f"weight_ih_l{k}{sfx}"))
                getattr(one, "weight_hh_l0" + sfx).copy_(getattr(model.rnn, f"weight_hh_l{k}{sfx}"))
            x, _ = one(x)
        taps[f"rnn{k}"] = x.clone()
    return taps


def build(out_path, kw, shape):
    torch.manual_seed(7)
    model = RNNBaseSTFTMask(**kw).train()
    g = torch.Generator().manual_seed(8)
    with torch.no_grad():
        model.batchnorm.weight.copy_(1 + 0.2 * torch.randn(model.batchnorm.weight.shape, generator=g))
        model.batchnorm.bias.copy_(0.1 * torch.randn(model.batchnorm.bias.shape, generator=g))
    inp = torch.randn(*shape, generator=g)
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    with torch.no_grad():
        e0 = copy.deepcopy(model)(inp)
    tgt = e0 + 0.3 * e0.std() * torch.randn(e0.shape, generator=g)
    G = torch.randn(e0.shape, generator=g) / e0.numel() ** 0.5
    out = {"sd." + k: v.numpy() for k, v in sd0.items()}
    taps = layer_taps(model, inp, kw)
    hooks = [model.batchnorm.register_forward_hook(lambda m, a, o: taps.__setitem__("bn", o.detach().transpose(1, 2).clone())),
             model.fc_layers.register_forward_hook(lambda m, a, o: taps.__setitem__("head", o.detach().clone()))]
    est = model(inp)
    for h in hooks:
        h.remove()
    assert torch.equal(taps[f"rnn{kw['rnn_layer'] - 1}"], model.rnn(model.ampltude(inp).reshape(-1, shape[2], shape[3]).transpose(1, 2))[0])
    for k, v in model.state_dict().items():
        if k.endswith(("running_mean", "running_var", "num_batches_tracked")):
            out["run." + k] = v.detach().clone().numpy()
    with torch.no_grad():
        est_eval = copy.deepcopy(model).eval()(inp)
    loss = F.mse_loss(est, tgt)
    loss.backward()
    for k, v in taps.items():
        out["tap." + k] = v.detach().numpy()
    out.update(input=inp.numpy(), target=tgt.numpy(), est=est.detach().numpy(), est_eval=est_eval.numpy(), loss=np.float32(loss.item()), G=G.numpy())
    for k, prm in model.named_parameters():
        out["grad." + k] = prm.grad.clone().numpy()
    m2 = RNNBaseSTFTMask(**kw).train()
    m2.load_state_dict(sd0)
    (m2(inp) * G).sum().backward()
    for k, prm in m2.named_parameters():
        out["gradG." + k] = prm.grad.clone().numpy()
    m3 = RNNBaseSTFTMask(**kw).train()
    m3.load_state_dict(sd0)
    opt = torch.optim.Adam(m3.parameters(), lr=3e-4, betas=(0.9, 0.999))
    losses = []
    for _ in range(2):
        l3 = F.mse_loss(m3(inp), tgt)
        opt.zero_grad()
        l3.backward()
        torch.nn.utils.clip_grad_norm_(m3.parameters(), 5)
        opt.step()
        losses.append(l3.item())
    out["adam_losses"] = np.asarray(losses, dtype=np.float32)
    for k, v in m3.state_dict().items():
        out["adam." + k] = v.detach().clone().numpy()
    train = {k: out.pop(k) for k in list(out) if k.startswith(("grad.", "adam.")) or k in ("loss", "adam_losses")}
    train_path = out_path[:-len(".npz")] + "_train.npz"
    np.savez_compressed(out_path, **out)
    np.savez_compressed(train_path, **train)
    zeros = float((taps["head"] == 0).float().mean())
    print(os.path.basename(out_path), len(out), "+", len(train), "entries; est", tuple(est.shape), "finite", bool(torch.isfinite(est).all()),
          "mask zeros", round(zeros, 3), "loss", loss.item(), "adam", losses, sum(p.numel() for p in model.parameters()), "parameters",
          os.path.getsize(out_path), "+", os.path.getsize(train_path), "bytes")


if __name__ == "__main__":
    for tag, fx in FIXTURES.items():
        build(os.path.join(GOLDEN, tag + ".npz"), fx["kw"], fx["shape"])
