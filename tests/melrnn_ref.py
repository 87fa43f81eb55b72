"""fp32 / float64 restatement of MelRNN at n_mels = 0, training and eval -- TEST INFRASTRUCTURE ONLY (reference: src/model/mel_rnn.py:8-123).

Written from the description of the network, not from its text:
  * features |re^2 - im^2| of inputs [B, 1, F, T, 2] (not a magnitude), the channel axis squeezed;
  * [B, F, T] -> [B, T, F] goes into a batch_first=False recurrence: L = B steps over N = T independent rows;
  * `rnn_layer` stacked bias-free, unidirectional layers without dropout: the Elman cell h' = tanh(W_ih x + W_hh h) ('rnn'), or the LSTM /
    GRU of tests/rnnmask_ref.py;
  * BatchNorm1d over all L N positions, Linear + ReLU, Linear + Sigmoid, out[b, 0, f, t, :] = mask[b, t, f] inputs[b, 0, f, t, :].
Hooks: taps= (dict: "rnn{k}" [L, N, H], "bn" [L, N, H], "relu" [L, N, F], "head" [L, N, F]), running= (dict that receives the running
statistics after a training pass), sim= (oracle.dccrn_oracle.Bf16Sim / NoSim: bf16 round-trips where the HIP path stores bf16 -- the
features, every weight of a product, every layer's output h (also the next step's operand; the LSTM's c and the GRU's h are carried
unrounded, the Elman cell's only state IS its output), the BatchNorm output, a1 = ReLU(fc_layers.0) and the mask; use NoSim in float64).
Pinned against vectors of the imported reference by tests/test_melrnn_host.py (tests/golden/melrnn_*.npz, tools/gen_golden_melrnn.py)."""
import torch

from rnnmask_ref import Bf16Sim, NoSim, EPS, MOMENTUM, _direction, load_fixture, param_names   # noqa: F401  (re-exported for the tests)

FIXTURES = {
    "melrnn_rnn2": dict(kw=dict(rnn_type="rnn", rnn_hidden=32, rnn_layer=2, n_fft=64, hop_length=16, n_mels=0), shape=(3, 1, 33, 21, 2)),
    "melrnn_lstm1": dict(kw=dict(rnn_type="lstm", rnn_hidden=64, rnn_layer=1, n_fft=64, hop_length=16, n_mels=0), shape=(2, 1, 33, 17, 2)),
    "melrnn_gru2": dict(kw=dict(rnn_type="gru", rnn_hidden=32, rnn_layer=2, n_fft=64, hop_length=16, n_mels=0), shape=(5, 1, 33, 35, 2)),
}


def _elman(x, w_ih, w_hh, sim):
    """x [L, N, in] -> h [L, N, H]: h(l) = tanh(x(l) W_ih^T + h(l-1) W_hh^T), h(-1) = 0; the stored h is what the next step reads"""
    L, N, _ = x.shape
    pre = x @ sim.weight(w_ih).t()
    whh = sim.weight(w_hh)
    h = x.new_zeros(N, w_hh.shape[1])
    outs = []
    for l in range(L):
        h = sim.act(torch.tanh(pre[l] + h @ whh.t()))
        outs.append(h)
    return torch.stack(outs)


def melrnn_forward(p, inputs, rnn_type="rnn", rnn_layer=2, training=True, sim=NoSim, taps=None, running=None, **_ignored):
    B, C, F, T, _ = inputs.shape
    assert C == 1, "the reference squeezes the channel axis"
    amp = (inputs[..., 0] ** 2 - inputs[..., 1] ** 2).abs()
    x = sim.act(amp.reshape(B, F, T).transpose(1, 2))              # [L, N, F]
    for k in range(rnn_layer):
        w_ih, w_hh = p[f"rnn.weight_ih_l{k}"], p[f"rnn.weight_hh_l{k}"]
        x = _elman(x, w_ih, w_hh, sim) if rnn_type == "rnn" else _direction(x, w_ih, w_hh, rnn_type, False, sim)
        if taps is not None:
            taps[f"rnn{k}"] = x
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
    a1 = sim.act(torch.relu(z @ sim.weight(p["fc_layers.0.weight"]).t() + p["fc_layers.0.bias"]))      # [L, N, F]
    if taps is not None:
        taps["relu"] = a1
    m = sim.act(torch.sigmoid(a1 @ sim.weight(p["fc_layers.2.weight"]).t() + p["fc_layers.2.bias"]))
    if taps is not None:
        taps["head"] = m
    return m.transpose(1, 2).reshape(B, 1, F, T, 1) * inputs
