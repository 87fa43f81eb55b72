"""fp32 / float64 restatement of RNNBaseSTFTMask, training and eval -- TEST INFRASTRUCTURE ONLY (reference: src/model/stft_rnn.py:5-119).

Written from the description of the network, not from its text:
  * features |re^2 - im^2| of inputs [B, C, F, T, 2] (not a magnitude);
  * [B C, F, T] -> [B C, T, F] goes into a batch_first=False recurrence: L = B C steps over N = T independent rows;
  * `rnn_layer` stacked bias-free LSTM (gates i, f, g, o) or GRU (r, z, n; n = tanh(W_in x + r (W_hn h)), h' = (1 - z) n + z h) layers,
    optionally bidirectional, dropout on every layer's output but the last;
  * BatchNorm1d over all L N positions, Linear + ReLU, out[b, s, c, f, t, :] = mask[(b, c), t, s F + f] inputs[b, c, f, t, :].
Hooks: taps= (dict: "rnn{k}" [L, N, Hout], "bn" [L, N, Hout], "head" [L, N, S F]), running= (dict that receives the running statistics
after a training pass), sim= (oracle.dccrn_oracle.Bf16Sim / NoSim: bf16 round-trips where the HIP path stores bf16 -- the features, every
weight of a product, every layer's output h (which is also the next step's operand; the carried c / h stays unrounded), the dropped-out
copy, the BatchNorm output and the mask; use NoSim in float64), drop_masks= ([rnn_layer - 1] tensors [L, N, Hout] holding 0 or
1 / (1 - p), or None: no dropout).  Also the Python twin of the device's dropout generator (sehip.plan_rnnmask.drop_keep_mask is the
same arithmetic on the product side; this copy is written against the header's description and the host test compares the two).
Pinned against vectors of the imported reference by tests/test_rnnmask_host.py (tests/golden/rnnmask_*.npz, tools/gen_golden_rnnmask.py)."""
import os

import numpy as np
import torch

from oracle.dccrn_oracle import Bf16Sim, NoSim   # noqa: F401  (re-exported for the tests)

EPS, MOMENTUM = 1e-5, 0.1
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = {
    "rnnmask_lstm_bi": dict(kw=dict(rnn_type="lstm", bidirectional=True, rnn_hidden=32, rnn_layer=2, num_spk=2, audio_channels=2, n_fft=64,
                                    hop_length=16, drop_out=0.0), shape=(3, 2, 33, 21, 2)),
    "rnnmask_gru_uni": dict(kw=dict(rnn_type="gru", bidirectional=False, rnn_hidden=64, rnn_layer=2, num_spk=1, audio_channels=1, n_fft=64,
                                    hop_length=16, drop_out=0.0), shape=(2, 1, 33, 17, 2)),
}


def load_fixture(tag):
    out = {"sd": {}, "tap": {}, "run": {}, "gradG": {}, "grad": {}, "adam": {}}
    for path in (os.path.join(GOLDEN_DIR, tag + ".npz"), os.path.join(GOLDEN_DIR, tag + "_train.npz")):
        z = np.load(path)
        for k in z.files:
            v = torch.from_numpy(np.asarray(z[k]))
            head, _, rest = k.partition(".")
            if head in out and rest:
                out[head][rest] = v
            else:
                out[k] = v
    return out


def param_names(sd):
    return [k for k in sd if not k.startswith("batchnorm.running") and not k.endswith("num_batches_tracked")]


# ---- dropout generator: 32-bit murmur3 finaliser, key from (seed, step counter, layer), one draw per element index ---------------------
def _mix(x):
    x = np.asarray(x, dtype=np.uint64) & 0xFFFFFFFF
    x = x ^ (x >> 16)
    x = (x * 0x85EBCA6B) & 0xFFFFFFFF
    x = x ^ (x >> 13)
    x = (x * 0xC2B2AE35) & 0xFFFFFFFF
    return x ^ (x >> 16)


def dropout_bits(seed, counter, layer, n):
    """uint32-valued [n]: the generator's word for elements 0 .. n-1"""
    seed = int(seed) & (2 ** 64 - 1)
    k = int(_mix(((int(counter) & 0xFFFFFFFF) * 0x9E3779B9 + int(layer)) & 0xFFFFFFFF))
    k = int(_mix((seed >> 32) ^ k))
    k = int(_mix((seed & 0xFFFFFFFF) ^ k))
    idx = np.arange(n, dtype=np.uint64)
    return _mix((_mix(idx ^ np.uint64(k)) + 0x9E3779B9) & 0xFFFFFFFF)


def dropout_keep(seed, counter, layer, n, p):
    """bool [n]: kept when the word's top 24 bits reach round(p 2^24)"""
    return (dropout_bits(seed, counter, layer, n) >> 8) >= int(round(float(p) * (1 << 24)))


def device_mask(seed, counter, layer, L, N, Hout, p, dtype=torch.float32):
    """the multiplier [L, N, Hout] (0 or 1 / (1 - p)) of layer `layer`'s output; the device indexes elements as [N][L][Hout]"""
    keep = torch.from_numpy(dropout_keep(seed, counter, layer, N * L * Hout, p)).view(N, L, Hout).permute(1, 0, 2)
    return keep.to(dtype) * (0.0 if p >= 1 else 1.0 / (1.0 - p))


# ---- the network ------------------------------------------------------------------------------------------------------------------------
def _direction(x, w_ih, w_hh, kind, reverse, sim):
    """x [L, N, in] -> h [L, N, H]; one direction of one layer"""
    L, N, _ = x.shape
    H = w_hh.shape[1]
    pre = x @ sim.weight(w_ih).t()
    whh = sim.weight(w_hh)
    state = x.new_zeros(N, H)      # c (LSTM) / h (GRU), carried unrounded
    hop = x.new_zeros(N, H)        # what the recurrent product reads
    outs = [None] * L
    for s in range(L):
        l = L - 1 - s if reverse else s
        a = hop @ whh.t()
        if kind == "lstm":
            g = pre[l] + a
            i, f, gg, o = torch.sigmoid(g[:, :H]), torch.sigmoid(g[:, H:2 * H]), torch.tanh(g[:, 2 * H:3 * H]), torch.sigmoid(g[:, 3 * H:])
            state = f * state + i * gg
            hop = sim.act(o * torch.tanh(state))
        else:
            r = torch.sigmoid(pre[l][:, :H] + a[:, :H])
            z = torch.sigmoid(pre[l][:, H:2 * H] + a[:, H:2 * H])
            n = torch.tanh(pre[l][:, 2 * H:] + r * a[:, 2 * H:])
            state = (1 - z) * n + z * state
            hop = sim.act(state)
        outs[l] = hop
    return torch.stack(outs)


def rnnmask_forward(p, inputs, rnn_type="lstm", rnn_layer=2, bidirectional=False, num_spk=2, training=True, sim=NoSim, taps=None,
                    running=None, drop_masks=None, **_ignored):
    B, C, F, T, _ = inputs.shape
    amp = (inputs[..., 0] ** 2 - inputs[..., 1] ** 2).abs()
    x = sim.act(amp.reshape(B * C, F, T).transpose(1, 2))          # [L, N, F]
    for k in range(rnn_layer):
        hs = [_direction(x, p[f"rnn.weight_ih_l{k}"], p[f"rnn.weight_hh_l{k}"], rnn_type, False, sim)]
        if bidirectional:
            hs.append(_direction(x, p[f"rnn.weight_ih_l{k}_reverse"], p[f"rnn.weight_hh_l{k}_reverse"], rnn_type, True, sim))
        x = torch.cat(hs, dim=-1)
        if taps is not None:
            taps[f"rnn{k}"] = x
        if k < rnn_layer - 1 and training and drop_masks is not None and drop_masks[k] is not None:
            x = sim.act(x * drop_masks[k].to(x.dtype))
    pre = "batchnorm."
    if training:
        mean, var = x.mean(dim=(0, 1)), x.var(dim=(0, 1), unbiased=False)
        if running is not None:
            n = x.shape[0] * x.shape[1]
            running[pre + "running_mean"] = ((1 - MOMENTUM) * p[pre + "running_mean"] + MOMENTUM * mean).detach()
            running[pre + "running_var"] = ((1 - MOMENTUM) * p[pre + "running_var"] + MOMENTUM * var * n / (n - 1)).detach()
            running[pre + "num_batches_tracked"] = p[pre + "num_batches_tracked"] + 1
    else:
        mean, var = p[pre + "running_mean"].to(x.dtype), p[pre + "running_var"].to(x.dtype)
    z = sim.act((x - mean) / torch.sqrt(var + EPS) * p[pre + "weight"] + p[pre + "bias"])
    if taps is not None:
        taps["bn"] = z
    m = sim.act(torch.relu(z @ sim.weight(p["fc_layers.0.weight"]).t() + p["fc_layers.0.bias"]))     # [L, N, S F]
    if taps is not None:
        taps["head"] = m
    m = m.reshape(B, C, T, num_spk, F).permute(0, 3, 1, 4, 2)     # [B, S, C, F, T]
    return m.unsqueeze(-1) * inputs.unsqueeze(1)
