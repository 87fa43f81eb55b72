"""Drop-in Wave-U-Net on libsehip (reference: src/model/wav_unet.py:8-110; `wav-unet` of the model registry).

Same constructor arguments, same ``forward(x[B, 1, T]) -> [B, 1, T]``, same state_dict keys and order (``encoder.{i}.main.0.weight``,
``encoder.{i}.main.1.running_mean``, ``middle.0.*``, ``decoder.{i}.main.{0,1}.*``, ``out.0.*``), so the reference's checkpoints load
here and vice versa.  Parameters are views into one flat fp32 buffer; forward / backward run the HIP kernels through the C ABI; a
CPU tensor raises SehipError.  Built: 1 .. 12 layers, channels_interval a multiple of 8, clips of a multiple of 2^unet_nlayers
samples with at least two frames in the middle block (the reference fails in torch.cat on any other length).  Training uses batch
statistics and updates the running ones as nn.BatchNorm1d does; eval uses the running statistics (forward only).
"""
import math
import os

import torch

from .. import plan_wavunet as P
from .._lib import SehipError
from .flat import FlatModule

_STATIC_CACHE = {}


class _WavUnetFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, wav, anchor):
        ctx.model = model
        ctx.ws = model._run_forward(wav)
        ctx.generation = ctx.ws.generation
        return ctx.ws.out.clone()

    @staticmethod
    def backward(ctx, grad_out):
        if ctx.generation != ctx.ws.generation or ctx.ws.closed:
            raise SehipError("WavUnet.backward: the workspace of this forward was overwritten by a later forward of the same "
                             "shape (or evicted); run backward before the next forward of that shape")
        from .._lib import stream_scope
        with stream_scope():
            ctx.model._run_backward(ctx.ws, grad_out)
        return None, None, None


class WavUnet(FlatModule):
    def __init__(self, unet_nlayers=12, channels_interval=24, *args, **kwargs):
        super().__init__()
        self.cfg = cfg = P.WavUnetConfig(unet_nlayers=unet_nlayers, channels_interval=channels_interval)
        skey = cfg.key()
        if skey not in _STATIC_CACHE:
            _STATIC_CACHE[skey] = P.WavUnetStatic(cfg)
        self.static = _STATIC_CACHE[skey]
        self.n_layers, self.channels_interval = unet_nlayers, channels_interval
        self._tables = None
        self._ws_cap = max(1, int(os.environ.get("SEHIP_WS_CACHE", "4")))
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
        dev = self._require_gpu("WavUnet")
        if self._tables is None:
            self._tables = P.WavUnetDeviceTables(self.static, dev)
        return self._lru_get((batch, nsample), self._ws_cap, lambda: P.WavUnetWorkspace(self.static, self._tables, batch, nsample, dev))

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
        if not input.is_cuda:
            raise SehipError("WavUnet.forward got a CPU tensor: the HIP path needs a gfx950 GPU (no CPU fallback)")
        if torch.is_grad_enabled():
            if not self.training:
                # forward only: a backward pass through the running statistics is not built (as for DCCRN and DCUnet)
                ws = self._run_forward(input)
                out = ws.out.clone().requires_grad_(True)
                return _EvalGuard.apply(out)
            if self._anchor is None or self._anchor.device != input.device:
                self._anchor = torch.zeros(1, device=input.device, requires_grad=True)
            return _WavUnetFunction.apply(self, input, self._anchor)
        return self._run_forward(input).out.clone()


class _EvalGuard(torch.autograd.Function):
    """Identity whose backward raises: an eval-mode output takes part in a graph (losses are computed on it) but has no gradient."""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        raise SehipError("WavUnet.backward in eval mode: the backward pass is built for batch statistics only (call model.train())")
