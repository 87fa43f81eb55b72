"""Drop-in U-Net on libsehip (reference: src/model/unet.py:9-146; `unet` of the model registry).

Same constructor arguments, same ``forward(mix[R, unet_channels, F, T, 2]) -> [R, unet_channels, F, T, 2]`` in fp32, same state_dict keys,
order, shapes and dtypes (``encoder.{i}.maxpool_conv.0.double_conv.{0,1,3,4}.*``, ``middle.double_conv.*``, ``decoder.{i}.up.*`` for
i >= 1, ``decoder.{i}.conv.double_conv.*``, ``outconv.up.*``, ``outconv.conv.double_conv.*``): checkpoints load both ways.  Parameters
are views into one flat fp32 buffer; forward / backward run the HIP kernels through the C ABI; a CPU tensor raises SehipError.

Built: the transposed-convolution decoder (bilinear=False, the shipped setting), unet_channels 1 .. 15, unet_layer 1 .. 4, inputs of
at least 2^unet_layer bins and frames.  ``unet_dropout`` (build-only, default 0.5) is the p of the two dropout sites the reference
hard-codes (the last encoder block and the middle block); the reference swallows the keyword.  Dropout is counter-based as in
rnn-stft-mask: the model draws a 64-bit seed from torch's default CPU generator at construction, a step counter lives on the device.
Training uses batch statistics and updates the running ones as nn.BatchNorm2d does; eval uses the running statistics and drops
nothing (forward only).
"""
import math

import torch

from .. import plan_unet as P
from .._lib import SehipError
from .flat import FlatModule


class UNet(FlatModule):
    plan_name = "UNet"

    def __init__(self, unet_channels=None, unet_layer=4, bilinear=False, *args, unet_dropout=0.5, **kwargs):
        super().__init__()
        self.cfg = cfg = P.UNetConfig(unet_channels=unet_channels, unet_layer=unet_layer, bilinear=bilinear, unet_dropout=unet_dropout)
        self.static = self._static(cfg.key(), lambda: P.UNetStatic(cfg))
        self.unet_channels, self.unet_layer, self.bilinear = unet_channels, unet_layer, bilinear
        self._ws_guard = 0           # tests: canary bands around every buffer of workspaces created from here on
        self._build_flat(list_roots=("encoder", "decoder"))
        mods = dict(self._modules)             # the reference registers encoder, middle, decoder, outconv: state_dict() follows that order
        self._modules.clear()
        self._modules.update({k: mods[k] for k in ("encoder", "middle", "decoder", "outconv")})
        # one 64-bit dropout seed per model from torch's default CPU generator: torch.manual_seed(k) before construction reproduces a run
        self.dropout_seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
        self._drop_counter = None
        self.reset_parameters()

    def reset_parameters(self):
        """PyTorch's defaults, which is all the reference uses: nn.Conv2d weight U(+-1/sqrt(fan_in)) (kaiming_uniform_ with a = sqrt(5) is
        that bound), nn.ConvTranspose2d weight and bias the same with torch's fan_in of a transposed weight (weight.size(1) x 4),
        BatchNorm weight 1 / bias 0, running statistics 0 / 1, counters 0."""
        with torch.no_grad():
            by_name = dict(self._params)
            for name, p in self._params:
                if p.dim() == 4:
                    bound = 1.0 / math.sqrt(p.shape[1] * p.shape[2] * p.shape[3])
                    p.uniform_(-bound, bound)
                    if name.endswith("up.weight"):
                        by_name[name[:-len("weight")] + "bias"].uniform_(-bound, bound)
                elif name.endswith("up.bias"):
                    pass
                elif name.endswith("weight"):
                    p.fill_(1.0)
                else:
                    p.zero_()
            for name, node, leaf in self._buffers_named:
                getattr(node, leaf).fill_(1.0 if name.endswith("running_var") else 0.0)
            self._nbt.zero_()

    def _counter(self, dev):
        if self._drop_counter is None or self._drop_counter.device != dev:
            self._drop_counter = torch.zeros(1, dtype=torch.int64, device=dev)
        return self._drop_counter

    def workspace(self, items, nbins, nframe):
        dev = self._require_gpu()
        if self._tables is None:
            self._tables = P.UNetDeviceTables(self.static, dev)
        return self._lru_get((items, nbins, nframe),
                             lambda: P.UNetWorkspace(self.static, self._tables, items, nbins, nframe, dev, guard=self._ws_guard))

    def _run_forward(self, x):
        ws = self.workspace(x.shape[0], x.shape[2], x.shape[3])
        ws.generation += 1
        ws.forward(x.contiguous().float(), self._flat, self._bflat, self._nbt, self.dropout_seed, self._counter(x.device), training=self.training)
        return ws

    def _run_backward(self, ws, grad_out):
        g = grad_out.contiguous().float()
        tail = self._tail_for_backward()
        self._backward_into_flat(lambda dst: ws.backward(g, self._flat, dst, tail=tail))
        self._tail_mark(tail)

    def forward(self, mix):
        cfg = self.cfg
        if mix.dim() != 5 or mix.shape[1] != cfg.uc or mix.shape[4] != 2:
            raise SehipError(f"UNet.forward: [R, unet_channels={cfg.uc}, F, T, 2] expected, got {tuple(mix.shape)}")
        if mix.shape[2] < 2 ** cfg.L or mix.shape[3] < 2 ** cfg.L:
            raise SehipError(f"UNet.forward: F={mix.shape[2]} bins x T={mix.shape[3]} frames do not fit unet_layer={cfg.L}: F and T must be "
                             f"at least 2^{cfg.L} = {2 ** cfg.L} (the reference fails inside max_pool2d below that)")
        out = self._run_plan(mix, torch.is_grad_enabled() and self.training)
        return self._eval_guarded(out) if torch.is_grad_enabled() and not self.training else out
