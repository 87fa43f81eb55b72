"""Drop-in MelRNN on libsehip (reference: src/model/mel_rnn.py:8-114; `mel-rnn` of the model registry), at n_mels = 0.

Same constructor arguments and defaults, same ``forward(x[B, 1, F, T, 2]) -> [B, 1, F, T, 2]`` in fp32, same state_dict keys, shapes and
order (``rnn.weight_ih_l{k}``, ``rnn.weight_hh_l{k}``, ``batchnorm.*``, ``fc_layers.0.*``, ``fc_layers.2.*``): checkpoints load both
ways.  Built: n_mels of 0 (or anything false) with rnn_type 'rnn' (the tanh Elman cell, no bias), 'lstm' and 'gru', 1 .. 8 layers,
rnn_hidden a multiple of 32 up to 1024, even n_fft up to 4096; unidirectional, no dropout, as in the reference.  n_mels > 0 -- the
constructor's default -- is refused: torchaudio's InverseMelScale(max_iter=0) returns its random starting point.

As in the reference the features are |re^2 - im^2| and the recurrence runs along the batch axis (batch_first=False on [B][T][F]): the
output of an utterance depends on the batch it is in.  The channel axis must be 1 (the reference squeezes it).
"""
import math

import torch

from .. import plan_melrnn as P
from .._lib import SehipError
from .flat import FlatModule


class MelRNN(FlatModule):
    plan_name = "MelRNN"

    def __init__(self, n_fft=512, hop_length=256, n_mels=128, f_min=100, f_max=8000, sample_rate=16000, rnn_hidden=256, rnn_layer=2,
                 rnn_type="rnn", *args, **kwarg):
        super().__init__()
        self.cfg = cfg = P.MelRnnConfig(n_fft=n_fft, hop_length=hop_length, n_mels=n_mels, f_min=f_min, f_max=f_max, sample_rate=sample_rate,
                                        rnn_hidden=rnn_hidden, rnn_layer=rnn_layer, rnn_type=rnn_type)
        self.static = self._static(cfg.key(), lambda: P.MelRnnStatic(cfg))
        self.n_fft, self.hop_length, self.n_mels, self.sample_rate, self.f_min, self.f_max = n_fft, hop_length, n_mels, sample_rate, f_min, f_max
        self._ws_guard = 0           # tests: canary bands around every buffer of workspaces created from here on
        self._build_flat()
        # gradients land in the flat buffer in the parameters' own layout: no un-pack launch could take the optimizer's sums along
        del self._tail_sink
        self.reset_parameters()

    def reset_parameters(self):
        """PyTorch's defaults: recurrent weights U(+-1/sqrt(H)), each nn.Linear weight and bias U(+-1/sqrt(fan_in)), BatchNorm 1 / 0,
        running statistics 0 / 1, counter 0."""
        with torch.no_grad():
            for name, p in self._params:
                if name.startswith("rnn."):
                    bound = 1.0 / math.sqrt(self.cfg.H)
                    p.uniform_(-bound, bound)
                elif name.startswith("fc_layers."):
                    bound = 1.0 / math.sqrt(self.cfg.H if name.startswith("fc_layers.0.") else self.cfg.F)
                    p.uniform_(-bound, bound)
                elif name == "batchnorm.weight":
                    p.fill_(1.0)
                else:
                    p.zero_()
            for name, node, leaf in self._buffers_named:
                getattr(node, leaf).fill_(1.0 if name.endswith("running_var") else 0.0)
            self._nbt.zero_()

    def set_deterministic(self, on=True):
        """Nothing to switch: no kernel of this model uses atomics, two runs from the same seed are bit-identical by construction."""
        return self

    def workspace(self, batch, nframe):
        dev = self._require_gpu()
        return self._lru_get((batch, nframe), lambda: P.MelRnnWorkspace(self.static, batch, nframe, dev, guard=self._ws_guard))

    def _run_forward(self, x):
        ws = self.workspace(x.shape[0], x.shape[3])
        ws.generation += 1
        ws.forward(x.contiguous().float(), self._flat, self._bflat, self._nbt, training=self.training)
        return ws

    def _run_backward(self, ws, grad_out):
        g = grad_out.contiguous().float()
        self._backward_into_flat(lambda dst: ws.backward(g, self._flat, dst))

    def forward(self, inputs):
        cfg = self.cfg
        if inputs.dim() != 5 or inputs.shape[1] != 1 or inputs.shape[2] != cfg.F or inputs.shape[4] != 2:
            raise SehipError(f"MelRNN.forward: [B, 1, {cfg.F}, T, 2] expected (the channel axis is squeezed: mono only), got {tuple(inputs.shape)}")
        out = self._run_plan(inputs, torch.is_grad_enabled() and self.training)
        return self._eval_guarded(out) if torch.is_grad_enabled() and not self.training else out
