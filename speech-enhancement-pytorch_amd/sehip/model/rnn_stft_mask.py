"""Drop-in RNNBaseSTFTMask on libsehip (reference: src/model/stft_rnn.py:5-110; `rnn-stft-mask` of the model registry).

Same constructor arguments and defaults, same ``forward(x[B, C, F, T, 2]) -> [B, S, C, F, T, 2]`` in fp32, same state_dict keys, shapes
and order (``rnn.weight_ih_l{k}``, ``rnn.weight_hh_l{k}``, their ``_reverse`` pair, ``batchnorm.*``, ``fc_layers.0.*``): checkpoints
load both ways.  Built: rnn_type 'lstm' and 'gru' (the Elman cell 'rnn', the constructor's default, has no HIP path yet and is
refused), 1 .. 8 layers, rnn_hidden a multiple of 32 up to 1024, either direction count, 1 .. 6 speakers, even n_fft, drop_out in
[0, 1], activation 'relu'.

As in the reference the features are |re^2 - im^2| and the recurrence runs along the batch x channel axis (batch_first=False on
[B C][T][F]): the output of an utterance depends on the batch it is in.  Dropout between the layers is counter-based: the model draws a
64-bit seed from torch's default CPU generator at construction, a step counter lives on the device and is advanced there.
"""
import math

import torch

from .. import plan_rnnmask as P
from .._lib import SehipError
from .flat import FlatModule

class RNNBaseSTFTMask(FlatModule):
    plan_name = "RNNBaseSTFTMask"

    def __init__(self, num_spk=2, audio_channels=2, n_fft=512, hop_length=256, sample_rate=16000, rnn_hidden=256, rnn_layer=2,
                 rnn_type="rnn", drop_out=0.5, activation="relu", bidirectional=False, *args, **kwarg):
        super().__init__()
        self.cfg = cfg = P.RnnMaskConfig(num_spk=num_spk, audio_channels=audio_channels, n_fft=n_fft, hop_length=hop_length,
                                         sample_rate=sample_rate, rnn_hidden=rnn_hidden, rnn_layer=rnn_layer, rnn_type=rnn_type,
                                         drop_out=drop_out, activation=activation, bidirectional=bidirectional)
        self.static = self._static(cfg.key(), lambda: P.RnnMaskStatic(cfg))
        self.audio_channels, self.num_spk, self.n_fft, self.hop_length, self.sample_rate = audio_channels, num_spk, n_fft, hop_length, sample_rate
        self._ws_guard = 0           # tests: canary bands around every buffer of workspaces created from here on
        self._build_flat()
        # gradients land in the flat buffer in the parameters' own layout: there is no un-pack launch that could take the optimizer's clip /
        # metric sums along (FlatModule._tail_sink), so the model does not offer that hook and FlatOptimizer keeps its own launches
        del self._tail_sink
        # one 64-bit dropout seed per model from torch's default CPU generator: torch.manual_seed(k) before construction reproduces a run
        self.dropout_seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
        self._drop_counter = None
        self.reset_parameters()

    def reset_parameters(self):
        """PyTorch's defaults: nn.LSTM / nn.GRU weights U(+-1/sqrt(H)), nn.Linear weight and bias U(+-1/sqrt(fan_in)), BatchNorm 1 / 0,
        running statistics 0 / 1, counter 0."""
        with torch.no_grad():
            for name, p in self._params:
                if name.startswith("rnn."):
                    bound = 1.0 / math.sqrt(self.cfg.H)
                    p.uniform_(-bound, bound)
                elif name.startswith("fc_layers."):
                    bound = 1.0 / math.sqrt(self.cfg.Hout)
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

    def _counter(self, dev):
        if self._drop_counter is None or self._drop_counter.device != dev:
            self._drop_counter = torch.zeros(1, dtype=torch.int64, device=dev)
        return self._drop_counter

    def workspace(self, batch, nframe):
        dev = self._require_gpu()
        return self._lru_get((batch, self.cfg.audio_channels, nframe),
                             lambda: P.RnnMaskWorkspace(self.static, batch, nframe, dev, guard=self._ws_guard))

    def _run_forward(self, x):
        ws = self.workspace(x.shape[0], x.shape[3])
        ws.generation += 1
        ws.forward(x.contiguous().float(), self._flat, self._bflat, self._nbt, self.dropout_seed, self._counter(x.device), training=self.training)
        return ws

    def _run_backward(self, ws, grad_out):
        g = grad_out.contiguous().float()
        self._backward_into_flat(lambda dst: ws.backward(g, self._flat, dst, self.dropout_seed))

    def forward(self, inputs):
        cfg = self.cfg
        if inputs.dim() != 5 or inputs.shape[1] != cfg.audio_channels or inputs.shape[2] != cfg.F or inputs.shape[4] != 2:
            raise SehipError(f"RNNBaseSTFTMask.forward: [B, {cfg.audio_channels}, {cfg.F}, T, 2] expected, got {tuple(inputs.shape)}")
        out = self._run_plan(inputs, torch.is_grad_enabled() and self.training)
        return self._eval_guarded(out) if torch.is_grad_enabled() and not self.training else out
