"""Host-side plan of the Wave-U-Net train step on libsehip (reference: src/model/wav_unet.py:8-110; `wav-unet` of the registry).

Activations are channels-last bf16 ``[B][T_l][C_l]`` with T_l = T / 2^l (level n = unet_nlayers is the middle block); the waveform
and the network output stay fp32.  Every convolution but the first is a product of the implicit-GEMM engine (csrc/gemm.hip, generic
kernels, bias / bias gradient through the descriptor):
  * encoder layers 1 .. n-1 and the middle: 15 taps.  The ``[::2]`` in front of them (:89) is not a kernel: the product binds the
    previous layer's activated tensor z as the PAIR view ``[B][T_l / 2][2 C]`` and takes channel chunks 0 .. C-1 of it, the even
    frames.  Its input gradient lands in a dense half-length buffer that the previous layer's BatchNorm backward adds on the even
    frames (``dz_even`` of sehip_wun_bn_bwd_*): no scatter-add pass, no zero fill;
  * decoder layers: 5 taps over TWO sources, the upsampled tensor and the encoder's skip tensor (the reference's torch.cat, :103);
    its input gradient has two destinations, d_up and the skip half;
  * weight gradients: the same descriptors with dOut as the second operand, on the side stream.
Everything else is csrc/wavunet.hip: the first layer straight from the fp32 waveform, BatchNorm1d + LeakyReLU(0.1) (batch statistics
forward / backward), the same fused with the align-corners x2 linear upsampling (the activated tensor of a decoder / middle layer is
never stored), the upsampling's adjoint as a gather, and the ``cat + 1x1 + tanh`` head.

The product graph itself (Prod, the arenas, the un-pack table, the bound descriptors, prologue and un-pack) is sehip/prodgraph.py, shared
with plan_unet.py; this module holds the network's own products, its shape refusals and its launch sequence.
"""
import numpy as np
import torch

from . import _lib
from ._lib import call, ptr, stream, SehipError
from .prodgraph import ProdDeviceTables, ProdStatic, ProdWorkspace

BN_EPS, BN_MOMENTUM, ENC_TAPS, DEC_TAPS = 1e-5, 0.1, 15, 5


def up2_table(t_in):
    """(left source frame, right source frame, weight of the right one) of every output position of
    F.interpolate(scale_factor=2, mode="linear", align_corners=True) over t_in frames, in integers as csrc/wavunet.hip computes them:
    p (t_in - 1) = i (2 t_in - 1) + r, weight r / (2 t_in - 1), right neighbour clamped to t_in - 1."""
    p = np.arange(2 * t_in, dtype=np.int64)
    den = 2 * t_in - 1
    num = p * (t_in - 1)
    i0 = num // den
    return i0, np.minimum(i0 + 1, t_in - 1), (num - i0 * den) / den


class WavUnetConfig:
    """Constructor arguments of the reference model (src/model/wav_unet.py:35)."""

    def __init__(self, unet_nlayers=12, channels_interval=24, **_ignored):
        if not isinstance(unet_nlayers, int) or not 1 <= unet_nlayers <= 12:
            raise SehipError(f"sehip WavUnet: unet_nlayers={unet_nlayers!r} must be an integer in 1 .. 12")
        if not isinstance(channels_interval, int) or channels_interval < 8 or channels_interval % 8:
            raise SehipError(f"sehip WavUnet: channels_interval={channels_interval!r} must be a multiple of 8 (16-byte pieces of 8 bf16 channels)")
        if 2 * unet_nlayers * channels_interval > 2048:
            raise SehipError(f"sehip WavUnet: channels_interval={channels_interval} with unet_nlayers={unet_nlayers}: more than 2048 channels "
                             "in one tensor")
        self.n, self.ci = unet_nlayers, channels_interval

    def key(self):
        return (self.n, self.ci)

    def enc_channels(self, l):
        return (1 if l == 0 else l * self.ci), (l + 1) * self.ci

    def dec_channels(self, i):
        """(upsampled channels, skip channels, output channels) of decoder layer i"""
        n, ci = self.n, self.ci
        return (n * ci if i == 0 else (n - i + 1) * ci), (n - i) * ci, (n - i) * ci

    def param_specs(self):
        """[(name, shape, kind)] in the reference's state_dict() order (named_parameters() is the same without the buffers)."""
        out = []

        def layer(pre, cout, cin, k):
            out.append((pre + "0.weight", (cout, cin, k), "param")); out.append((pre + "0.bias", (cout,), "param"))
            out.append((pre + "1.weight", (cout,), "param")); out.append((pre + "1.bias", (cout,), "param"))
            out.append((pre + "1.running_mean", (cout,), "buffer")); out.append((pre + "1.running_var", (cout,), "buffer"))
            out.append((pre + "1.num_batches_tracked", (), "nbt"))

        for l in range(self.n):
            cin, cout = self.enc_channels(l)
            layer(f"encoder.{l}.main.", cout, cin, ENC_TAPS)
        layer("middle.", self.n * self.ci, self.n * self.ci, ENC_TAPS)
        for i in range(self.n):
            cu, cs, co = self.dec_channels(i)
            layer(f"decoder.{i}.main.", co, cu + cs, DEC_TAPS)
        out.append(("out.0.weight", (1, 1 + self.ci, 1), "param")); out.append(("out.0.bias", (1,), "param"))
        return out


def _chunks(src, frame_off, cn):
    assert cn % 8 == 0
    return [(src, frame_off, 0, 8 * q) for q in range(cn // 8)]


class WavUnetStatic(ProdStatic):
    """Products, packed-weight layout and gradient un-packing table (independent of batch and clip length).  A product's sources are
    (buffer, pair view?) tuples (WavUnetWorkspace._src_view)."""
    plan_name = "WavUnet"

    def __init__(self, cfg: WavUnetConfig):
        super().__init__(cfg)
        ia = self.layout.index_array
        n, ci = cfg.n, cfg.ci
        ga, buf, prod, norm = self.ga, self.buf, self.prod, self.norm

        def conv15(key, pre, zin, cin, cout, level, y, dy, dzeven):
            """15 taps over the pair view of zin (level - 1) -> y; input gradient -> dzeven [T_level][cin]"""
            w = ia(pre + "0.weight")                                   # [cout][cin][15]
            rows = [r for p in range(ENC_TAPS) for r in _chunks(0, p - ENC_TAPS // 2, cin)]
            prod(key + ".fwd", rows, w.transpose(0, 2, 1).reshape(cout, ENC_TAPS * cin), [(zin, True)], [(y, cout)], level,
                 bias=ia(pre + "0.bias"), dout=dy)
            rows = [r for p in range(ENC_TAPS) for r in _chunks(0, ENC_TAPS // 2 - p, cout)]
            prod(key + ".dg", rows, w.transpose(1, 2, 0).reshape(cin, ENC_TAPS * cout), [(dy, False)], [(dzeven, cin)], level, kind="dgrad")

        self.enc0_goff = ga.reserve((ENC_TAPS + 1) * ci)                # dW [C0][15] | db [C0]
        for l in range(n):
            cin, cout = cfg.enc_channels(l)
            k = f"e{l}"
            buf(k + ".y", l, cout); buf(k + ".z", l, cout); buf(k + ".dy", l, cout); buf(k + ".dskip", l, cout); buf(k + ".dzeven", l + 1, cout)
            if l > 0:
                conv15(k, f"encoder.{l}.main.", f"e{l - 1}.z", cin, cout, l, k + ".y", k + ".dy", f"e{l - 1}.dzeven")
            norm(k, f"encoder.{l}.main.1.", cout, l, k + ".y")
        cm = n * ci
        buf("m.y", n, cm); buf("m.dy", n, cm); buf("m.dz", n, cm)
        conv15("m", "middle.", f"e{n - 1}.z", cm, cm, n, "m.y", "m.dy", f"e{n - 1}.dzeven")
        norm("m", "middle.1.", cm, n, "m.y")
        for i in range(n):
            cu, cs, co = cfg.dec_channels(i)
            lv = n - 1 - i
            k = f"d{i}"
            buf(k + ".up", lv, cu); buf(k + ".dup", lv, cu); buf(k + ".y", lv, co); buf(k + ".dy", lv, co); buf(k + ".dz", lv, co)
            pre = f"decoder.{i}.main."
            w = ia(pre + "0.weight")                                   # [co][cu + cs][5], input channels = cat([up, skip])
            rows = [r for p in range(DEC_TAPS) for r in _chunks(0, p - DEC_TAPS // 2, cu) + _chunks(1, p - DEC_TAPS // 2, cs)]
            prod(k + ".fwd", rows, w.transpose(0, 2, 1).reshape(co, DEC_TAPS * (cu + cs)), [(k + ".up", False), (f"e{lv}.z", False)],
                 [(k + ".y", co)], lv, bias=ia(pre + "0.bias"), dout=k + ".dy")
            rows = [r for p in range(DEC_TAPS) for r in _chunks(0, DEC_TAPS // 2 - p, co)]
            prod(k + ".dg", rows, w.transpose(1, 2, 0).reshape(cu + cs, DEC_TAPS * co), [(k + ".dy", False)],
                 [(k + ".dup", cu), (f"e{lv}.dskip", cs)], lv, kind="dgrad")
            norm(k, pre + "1.", co, lv, k + ".y")
        buf("zl", 0, ci)                                               # the last decoder layer's activated output: the head reads it
        self.out_goff = ga.reserve(ci + 2)                              # dW [C0 + 1] | db

        c0 = ci
        self._assemble(extra=[(ia("encoder.0.main.0.weight"), self.enc0_goff + np.arange(ENC_TAPS * c0)),
                              (ia("encoder.0.main.0.bias"), self.enc0_goff + ENC_TAPS * c0 + np.arange(c0)),
                              (ia("out.0.weight"), self.out_goff + np.arange(c0 + 1)),
                              (ia("out.0.bias"), self.out_goff + c0 + 1)])


WavUnetDeviceTables = ProdDeviceTables


def valid_lengths(T, n):
    """the nearest clip lengths below and above T that the n-layer network takes: multiples of 2^n with at least two middle frames"""
    m = 2 ** n
    lo = max(2 * m, T // m * m)
    hi = max(2 * m, -(-T // m) * m)
    return lo, hi


class WavUnetWorkspace(ProdWorkspace):
    def __init__(self, st: WavUnetStatic, tables: WavUnetDeviceTables, B, T, device):
        cfg = st.cfg
        n = cfg.n
        if T % 2 ** n or T // 2 ** n < 2:
            lo, hi = valid_lengths(T, n)
            raise SehipError(f"WavUnet: a clip of T={T} samples does not fit {n} layers: T must be a multiple of 2^{n} = {2 ** n} with at least "
                             f"two frames in the middle block (the reference fails in torch.cat otherwise); nearest valid lengths: {lo}"
                             + (f" and {hi}" if hi != lo else ""))
        if B < 1 or B > 65535:
            raise SehipError(f"WavUnet: batch size B={B} must be in 1 .. 65535")
        self.B, self.T = B, T
        self.lens = [T >> l for l in range(n + 1)]
        super().__init__(st, tables, B, self.lens, [1] * (n + 1), device)
        lib = _lib.lib()
        self.out = torch.zeros(B, 1, T, dtype=torch.float32, device=device)
        self.enc0_scratch = torch.zeros(int(lib.sehip_wun_enc0_wgrad_scratch_floats(B, T, cfg.ci)), dtype=torch.float32, device=device)
        self.out_scratch = torch.zeros(int(lib.sehip_wun_out_bwd_scratch_floats(B * T, cfg.ci)), dtype=torch.float32, device=device)
        self.wav = None
        self.training = True

    def _src_view(self, s):
        """a source is (buffer, pair view?): the pair view of [B][T][C] is [B][T / 2][2 C], whose channels 0 .. C-1 are the even frames"""
        name, pair = s
        b = self.bufs[name]
        if not pair:
            return b.ptr, b.Tst, 1, b.C
        assert b.Tst % 2 == 0
        return b.ptr, b.Tst // 2, 1, 2 * b.C

    # ---- launches (gemm, wgrad: GemmWorkspace) ------------------------------------------------------------------------
    def _norm_coef(self, key, params, buffers, nbt, training):
        """batch (training) or running (eval) statistics of layer `key` -> its coefficient records"""
        nm, L = self.st.norms[key], self.st.layout
        y, pre = self.bufs[nm["y"]], nm["pre"]
        rows = self.B * y.Tst
        if training:
            call("sehip_wun_bn_stats", y.ptr, rows, nm["C"], ptr(self.part[key]), stream())
        call("sehip_wun_bn_finalize", ptr(self.part[key]), y.ptr, self._pp(params, pre + "weight"), self._pp(params, pre + "bias"),
             buffers.data_ptr() + 4 * L.buffer_off[pre + "running_mean"][0], buffers.data_ptr() + 4 * L.buffer_off[pre + "running_var"][0],
             nbt.data_ptr() + 8 * L.nbt_idx[pre + "num_batches_tracked"], rows, nm["C"], BN_EPS, BN_MOMENTUM, 1 if training else 0,
             ptr(self.coef[key]), stream())
        return rows

    def _norm_bwd(self, key, dz_full, dz_even, dy):
        nm = self.st.norms[key]
        y = self.bufs[nm["y"]]
        rows = self.B * y.Tst
        ze = self.bufs[dz_even].ptr if dz_even else None
        g = self.gpack.data_ptr() + 4 * nm["goff"]
        call("sehip_wun_bn_bwd_reduce", self.bufs[dz_full].ptr, ze, y.ptr, ptr(self.coef[key]), rows, nm["C"], ptr(self.bpart[key]), stream())
        call("sehip_wun_bn_bwd_finalize", ptr(self.bpart[key]), ptr(self.coef[key]), rows, nm["C"], g, g + 4 * nm["C"], ptr(self.bcoef[key]), stream())
        call("sehip_wun_bn_bwd_apply", self.bufs[dz_full].ptr, ze, y.ptr, ptr(self.coef[key]), ptr(self.bcoef[key]), rows, nm["C"],
             self.bufs[dy].ptr, stream())
        self._chain_dirty = True

    def forward(self, wav, params, buffers, nbt, training=True):
        """wav [B, 1, T] fp32 on device -> self.out [B, 1, T]."""
        cfg, b = self.st.cfg, self.bufs
        B, T, n, c0 = self.B, self.T, cfg.n, cfg.ci
        pp = lambda nme: self._pp(params, nme)
        self.wav, self.training = wav, bool(training)
        self._prologue(params)
        call("sehip_wun_enc0_fwd", ptr(wav), pp("encoder.0.main.0.weight"), pp("encoder.0.main.0.bias"), B, T, c0, b["e0.y"].ptr, stream())
        for l in range(n):
            k = f"e{l}"
            if l > 0:
                self.gemm(k + ".fwd")
            rows = self._norm_coef(k, params, buffers, nbt, training)
            call("sehip_wun_bn_apply", b[k + ".y"].ptr, ptr(self.coef[k]), rows, (l + 1) * c0, b[k + ".z"].ptr, stream())
        self.gemm("m.fwd")
        self._norm_coef("m", params, buffers, nbt, training)
        prev, prev_key = "m.y", "m"
        for i in range(n):
            k = f"d{i}"
            cu, _, co = cfg.dec_channels(i)
            call("sehip_wun_bn_apply_up2", b[prev].ptr, ptr(self.coef[prev_key]), B, self.lens[n - i], cu, b[k + ".up"].ptr, stream())
            self.gemm(k + ".fwd")
            self._norm_coef(k, params, buffers, nbt, training)
            prev, prev_key = k + ".y", k
        call("sehip_wun_bn_apply", b[prev].ptr, ptr(self.coef[prev_key]), B * T, c0, b["zl"].ptr, stream())
        call("sehip_wun_out_fwd", b["zl"].ptr, ptr(wav), pp("out.0.weight"), pp("out.0.bias"), B * T, c0, ptr(self.out), stream())
        return self.out

    def backward(self, dout, params, grads, tail=None):
        """dout [B, 1, T] fp32 -> flat parameter gradients (overwritten)."""
        if not self.training:
            raise SehipError("WavUnet.backward in eval mode: the backward pass is built for batch statistics only (call model.train())")
        st, cfg, b = self.st, self.st.cfg, self.bufs
        B, T, n, c0 = self.B, self.T, cfg.n, cfg.ci
        pp = lambda nme: self._pp(params, nme)
        gp = lambda off: self.gpack.data_ptr() + 4 * off
        self._begin_backward()
        call("sehip_wun_out_bwd", ptr(dout), ptr(self.out), b["zl"].ptr, ptr(self.wav), pp("out.0.weight"), B * T, c0, b[f"d{n - 1}.dz"].ptr,
             gp(st.out_goff), gp(st.out_goff + c0 + 1), ptr(self.out_scratch), stream())
        for i in range(n - 1, -1, -1):
            k = f"d{i}"
            _, _, co = cfg.dec_channels(i)
            self._norm_bwd(k, k + ".dz", None, k + ".dy")
            self.wgrad(k + ".fwd")
            self.gemm(k + ".dg")
            call("sehip_wun_up2_bwd", b[k + ".dup"].ptr, B, self.lens[n - i], cfg.dec_channels(i)[0],
                 b[f"d{i - 1}.dz" if i > 0 else "m.dz"].ptr, stream())
        self._norm_bwd("m", "m.dz", None, "m.dy")
        self.wgrad("m.fwd")
        self.gemm("m.dg")
        for l in range(n - 1, -1, -1):
            k = f"e{l}"
            self._norm_bwd(k, k + ".dskip", k + ".dzeven", k + ".dy")
            if l > 0:
                self.wgrad(k + ".fwd")
                self.gemm(k + ".dg")
        call("sehip_wun_enc0_wgrad", b["e0.dy"].ptr, ptr(self.wav), B, T, c0, gp(st.enc0_goff), gp(st.enc0_goff + ENC_TAPS * c0),
             ptr(self.enc0_scratch), stream())
        return self._unpack(grads, tail)
