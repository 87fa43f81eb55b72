"""Drop-in Wave-U-Net on libsehip (reference: src/model/wav_unet.py:8-110; `wav-unet` of the model registry).

Same constructor arguments, same ``forward(x[B, 1, T]) -> [B, 1, T]``, same state_dict keys and order (``encoder.{i}.main.0.weight``,
``encoder.{i}.main.1.running_mean``, ``middle.0.*``, ``decoder.{i}.main.{0,1}.*``, ``out.0.*``), so the reference's checkpoints load
here and vice versa.  Parameters are views into one flat fp32 buffer; forward / backward run the HIP kernels through the C ABI; a
CPU tensor raises SehipError.  Built: 1 .. 12 layers, channels_interval a multiple of 8, clips of a multiple of 2^unet_nlayers
samples with at least two frames in the middle block (the reference fails in torch.cat on any other length).  Training uses batch
statistics and updates the running ones as nn.BatchNorm1d does; eval uses the running statistics (forward only).
"""
import math

import torch

from .. import plan_wavunet as P
from .._lib import SehipError
from .flat import FlatModule

class WavUnet(FlatModule):
    plan_name = "WavUnet"

    def __init__(self, unet_nlayers=12, channels_interval=24, *args, **kwargs):
        super().__init__()
        self.cfg = cfg = P.WavUnetConfig(unet_nlayers=unet_nlayers, channels_interval=channels_interval)
        self.static = self._static(cfg.key(), lambda: P.WavUnetStatic(cfg))
        self.n_layers, self.channels_interval = unet_nlayers, channels_interval
        self._build_flat(list_roots=("encoder", "decoder"))
        mods = dict(self._modules)             # the reference registers encoder, middle, decoder, out: state_dict() follows that order
        self._modules.clear()
        self._modules.update({k: mods[k] for k in ("encoder", "middle", "decoder", "out")})
        self.reset_parameters()

    def reset_parameters(self):
        """PyTorch's defaults, which is all the reference uses: nn.Conv1d weight and bias U(+-1/sqrt(fan_in)) (kaiming_uniform_ with
        a = sqrt(5) is that bound), BatchNorm weight 1 / bias 0, running statistics 0 / 1, counters 0."""
        with torch.no_grad():
            by_name = dict(self._params)
            for name, p in self._params:
                if name.endswith("0.weight"):
                    bound = 1.0 / math.sqrt(p.shape[1] * p.shape[2])
                    p.uniform_(-bound, bound)
                    by_name[name[:-len("weight")] + "bias"].uniform_(-bound, bound)
                elif name.endswith("1.weight"):
                    p.fill_(1.0)
                elif name.endswith("1.bias"):
                    p.zero_()
            for name, node, leaf in self._buffers_named:
                getattr(node, leaf).fill_(1.0 if name.endswith("running_var") else 0.0)
            self._nbt.zero_()

    def valid_length(self, length):
        """the shortest clip of at least `length` samples the network takes"""
        return P.valid_lengths(length, self.cfg.n)[1]

    def workspace(self, batch, nsample):
        dev = self._require_gpu()
        if self._tables is None:
            self._tables = P.WavUnetDeviceTables(self.static, dev)
        return self._lru_get((batch, nsample), lambda: P.WavUnetWorkspace(self.static, self._tables, batch, nsample, dev))

    def _run_forward(self, wav):
        ws = self.workspace(wav.shape[0], wav.shape[-1])
        ws.generation += 1
        ws.forward(wav.contiguous().float(), self._flat, self._bflat, self._nbt, training=self.training)
        return ws

    def _run_backward(self, ws, grad_out):
        g = grad_out.contiguous().float()
        tail = self._tail_for_backward()
        self._backward_into_flat(lambda dst: ws.backward(g, self._flat, dst, tail=tail))
        self._tail_mark(tail)

    def forward(self, input):
        if input.dim() != 3 or input.shape[1] != 1:
            raise SehipError(f"WavUnet.forward: [B, 1, T] expected, got {tuple(input.shape)}")
        out = self._run_plan(input, torch.is_grad_enabled() and self.training)
        return self._eval_guarded(out) if torch.is_grad_enabled() and not self.training else out

