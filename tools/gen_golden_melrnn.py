#!/usr/bin/env python3
"""tests/golden/melrnn_{rnn2,lstm1,gru2}{,_train}.npz from the IMPORTED reference (the path of a reference checkout is the first
argument or $SEHIP_REFERENCE).  Data only: nothing of the reference's program text is written.  The reference's module imports
torchaudio.transforms at its top; at n_mels = 0 nothing of it is called, so an empty stub module stands in where torchaudio is missing.

  melrnn_rnn2 : rnn_type='rnn' (Elman), rnn_hidden=32, rnn_layer=2, n_fft=64, input [3, 1, 33, 21, 2] -- three recurrence steps over 21
                rows (one full 16-row tile and a ragged one), F = 33 (padding to 40)
  melrnn_lstm1: rnn_type='lstm', rnn_hidden=64, rnn_layer=1, input [2, 1, 33, 17, 2] -- the shipped YAML's cell and layer count
  melrnn_gru2 : rnn_type='gru', rnn_hidden=32, rnn_layer=2, input [5, 1, 33, 35, 2]
All with n_mels=0.  Model seed 7, data seed 8, seeded non-trivial BatchNorm affine terms.  Per fixture: the state dict before any forward
pass (sd.*), the input, a target (the untrained output + 30 % noise), taps after every RNN layer (tap.rnn{k} [L, N, H], from single-layer
torch modules holding the same weights), after BatchNorm (tap.bn [L, N, H]), after the ReLU (tap.relu [L, N, F]) and after the sigmoid
(tap.head [L, N, F]), est, the running statistics after one training pass (run.*), est_eval, a fixed upstream gradient G and the gradients
of <est, G> (gradG.*); in *_train.npz the mse loss and its gradients (loss, grad.*), the losses and the final state of two Adam steps
(adam_losses, adam.*; lr 3e-4, clip_grad_norm_ 5 as src/solver.py:487-492).
Run:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_melrnn.py /path/to/reference"""
import copy
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

sys.dont_write_bytecode = True
REFERENCE = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SEHIP_REFERENCE")
if not REFERENCE:
    sys.exit("usage: gen_golden_melrnn.py /path/to/reference")
sys.path.insert(0, REFERENCE)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")

try:
    import torchaudio.transforms  # noqa: F401
except ImportError:
    _ta, _tr = types.ModuleType("torchaudio"), types.ModuleType("torchaudio.transforms")
    _ta.transforms = _tr
    sys.modules["torchaudio"], sys.modules["torchaudio.transforms"] = _ta, _tr

from src.model.mel_rnn import MelRNN  # noqa: E402
from melrnn_ref import FIXTURES  # noqa: E402  (the fixtures' configurations: one list for the generator and the tests)

CELLS = {"rnn": torch.nn.RNN, "lstm": torch.nn.LSTM, "gru": torch.nn.GRU}


def layer_taps(model, inputs, kw):
    """outputs [L, N, H] of every RNN layer: single-layer torch modules with the model's weights, chained"""
    x = model.amplitude(inputs).squeeze(1).transpose(1, 2)
    taps = {}
    for k in range(kw["rnn_layer"]):
        one = CELLS[kw["rnn_type"]](input_size=x.shape[-1], hidden_size=kw["rnn_hidden"], num_layers=1, bias=False)
        with torch.no_grad():
            one.weight_ih_l0.copy_(getattr(model.rnn, f"weight_ih_l{k}"))
            one.weight_hh_l0.copy_(getattr(model.rnn, f"weight_hh_l{k}"))
            x, _ = one(x)
        taps[f"rnn{k}"] = x.clone()
    return taps


def build(out_path, kw, shape):
    torch.manual_seed(7)
    model = MelRNN(**kw).train()
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
             model.fc_layers[1].register_forward_hook(lambda m, a, o: taps.__setitem__("relu", o.detach().clone())),
             model.fc_layers[3].register_forward_hook(lambda m, a, o: taps.__setitem__("head", o.detach().clone()))]
    est = model(inp)
    for h in hooks:
        h.remove()
    assert torch.equal(taps[f"rnn{kw['rnn_layer'] - 1}"], model.rnn(model.amplitude(inp).squeeze(1).transpose(1, 2))[0])
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
    m2 = MelRNN(**kw).train()
    m2.load_state_dict(sd0)
    (m2(inp) * G).sum().backward()
    for k, prm in m2.named_parameters():
        out["gradG." + k] = prm.grad.clone().numpy()
    m3 = MelRNN(**kw).train()
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
    hmax = max(float(v.abs().max()) for k, v in taps.items() if k.startswith("rnn"))
    print(os.path.basename(out_path), len(out), "+", len(train), "entries; est", tuple(est.shape), "finite", bool(torch.isfinite(est).all()),
          "max |h|", round(hmax, 3), "relu zeros", round(float((taps["relu"] == 0).float().mean()), 3), "sigmoid", round(float(taps["head"].min()), 3),
          "..", round(float(taps["head"].max()), 3), "loss", loss.item(), "adam", losses, sum(p.numel() for p in model.parameters()), "parameters",
          os.path.getsize(out_path), "+", os.path.getsize(train_path), "bytes")


if __name__ == "__main__":
    for tag, fx in FIXTURES.items():
        build(os.path.join(GOLDEN, tag + ".npz"), fx["kw"], fx["shape"])
