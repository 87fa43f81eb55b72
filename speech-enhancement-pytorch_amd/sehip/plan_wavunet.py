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
"""
import os

import numpy as np
import torch

from . import _lib
from ._lib import call, ptr, stream, SehipError
from .plan import Arena, CGemmDesc, ParamLayout, bind_chunk_table, dense_ntab, npad_of, pad_ktab, BF16
from .workspace import Buf, GemmWorkspace

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


class Prod:
    """One product of the engine (batch- and length-independent part).  srcs: [(buffer, pair view?)]; dsts: [(buffer, columns)];
    rows: [(source, frame offset, channel offset)] one per 8-channel chunk of K; level: the row space is T_level frames per item."""

    def __init__(self, name, rows, widx, srcs, dsts, level, bias=None, kind="fwd", dout=None):
        self.name, self.srcs, self.dsts, self.level, self.kind, self.dout = name, srcs, dsts, level, kind, dout
        self.ktab, self.K = pad_ktab([(s, fo, 0, co) for s, fo, co in rows])
        n, k0 = widx.shape
        self.N, self.Npad = n, npad_of(n)
        w = np.full((self.Npad, self.K), -1, dtype=np.int32)
        w[:n, :k0] = (widx.astype(np.int64) << 1).astype(np.int32)
        self.wtab = w.reshape(-1)
        self.bias = None
        if bias is not None:
            b = np.full((self.Npad, 2), -1, dtype=np.int32)
            b[:n, 0] = (np.asarray(bias, dtype=np.int64) << 1).astype(np.int32)
            self.bias = b
        assert sum(c for _, c in dsts) == n
        nt = np.concatenate([dense_ntab(c, c, q, 0) for q, (_, c) in enumerate(dsts)])
        self.ntab = np.concatenate([nt, np.zeros((self.Npad // 4 - nt.shape[0], 4), dtype=np.int32)])
        self.w_off = self.b_off = self.dw_off = self.db_off = self.kt_off = self.nt_off = None


def _chunks(src, frame_off, cn):
    assert cn % 8 == 0
    return [(src, frame_off, 8 * q) for q in range(cn // 8)]


class WavUnetStatic:
    """Products, packed-weight layout and gradient un-packing table (independent of batch and clip length)."""

    def __init__(self, cfg: WavUnetConfig):
        self.cfg = cfg
        self.layout = L = ParamLayout(cfg)
        # SEHIP_WUN_KEEP_GRADS=1 (tests): every layer keeps its own gradient buffers so that every kernel can be checked op-locally after
        # one step.  The plan gives every layer its own buffers anyway (nothing is shared yet): the switch is recorded and changes nothing, one plan serves both.
        self.keep_grads = bool(os.environ.get("SEHIP_WUN_KEEP_GRADS"))
        ia = L.index_array
        n, ci = cfg.n, cfg.ci
        self.prods = {}
        self.buffers = {}       # name -> (level, channels)
        self.norms = {}         # layer key -> dict(pre=parameter prefix, C, level, y, goff)
        ga = Arena(16)

        def buf(name, level, c):
            self.buffers[name] = (level, c)

        def prod(*a, **k):
            p = Prod(*a, **k)
            assert p.name not in self.prods
            self.prods[p.name] = p

        def norm(key, pre, c, level, y):
            self.norms[key] = dict(pre=pre, C=c, level=level, y=y, goff=ga.reserve(2 * c))

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
            norm(k, f"encoder.{l}.main.", cout, l, k + ".y")
        cm = n * ci
        buf("m.y", n, cm); buf("m.dy", n, cm); buf("m.dz", n, cm)
        conv15("m", "middle.", f"e{n - 1}.z", cm, cm, n, "m.y", "m.dy", f"e{n - 1}.dzeven")
        norm("m", "middle.", cm, n, "m.y")
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
            norm(k, pre, co, lv, k + ".y")
        buf("zl", 0, ci)                                               # the last decoder layer's activated output: the head reads it
        self.out_goff = ga.reserve(ci + 2)                              # dW [C0 + 1] | db

        wa, ba, kta, nta = Arena(64), Arena(4), Arena(1), Arena(1)
        for p in self.prods.values():
            p.kt_off = kta.add(p.ktab)
            p.nt_off = nta.add(p.ntab)
            p.w_off = wa.add(p.wtab)
            if p.bias is not None:
                p.b_off = ba.add(p.bias)
            if p.kind == "fwd":
                p.dw_off = ga.reserve(p.Npad * p.K)
                p.db_off = ga.reserve(p.Npad)
        self.n_wpack, self.n_bpack, self.n_gpack = wa.size, max(ba.size, 4), ga.size
        if max(self.n_wpack, self.n_gpack, L.n_params) >= 2 ** 30:
            raise SehipError("sehip WavUnet: the 32-bit packing tables hold fewer than 2^30 entries")
        self.wtab = wa.build(np.int32)
        self.btab = ba.build(np.int32, 2) if ba.size else np.full((4, 2), -1, dtype=np.int32)
        self.ktab = kta.build(np.int32, 4)
        self.ntab = nta.build(np.int32, 4, fill=0)
        for p in self.prods.values():
            p.wtab = None            # the arena's table holds the only copy from here on
        wa.pieces = []
        self.utab1 = self._build_unpack_table()

    def _build_unpack_table(self):
        """int32 [n_params]: (index in the packed-gradient buffer) << 1 of every parameter element, -1 for the layout's padding."""
        L, cfg = self.layout, self.cfg
        ia = L.index_array
        tab = np.full(L.n_params, -1, dtype=np.int32)
        total = [0]

        def put(pidx, gidx):
            pidx = np.asarray(pidx, dtype=np.int64).reshape(-1)
            gidx = np.asarray(gidx, dtype=np.int64).reshape(-1)
            tab[pidx] = (gidx << 1).astype(np.int32)
            total[0] += pidx.size

        for p in self.prods.values():
            if p.dw_off is None:
                continue
            w = self.wtab[p.w_off:p.w_off + p.Npad * p.K]
            m = np.flatnonzero(w >= 0)
            put(w[m] >> 1, p.dw_off + m)
            b = p.bias[:, 0]
            m = np.flatnonzero(b >= 0)
            put(b[m] >> 1, p.db_off + m)
        c0 = cfg.ci
        put(ia("encoder.0.main.0.weight"), self.enc0_goff + np.arange(ENC_TAPS * c0))
        put(ia("encoder.0.main.0.bias"), self.enc0_goff + ENC_TAPS * c0 + np.arange(c0))
        for nm in self.norms.values():
            put(ia(nm["pre"] + "1.weight"), nm["goff"] + np.arange(nm["C"]))
            put(ia(nm["pre"] + "1.bias"), nm["goff"] + nm["C"] + np.arange(nm["C"]))
        put(ia("out.0.weight"), self.out_goff + np.arange(c0 + 1))
        put(ia("out.0.bias"), self.out_goff + c0 + 1)
        used = np.zeros(L.n_params, dtype=bool)
        for name in L.param_names:
            off, shape = L.param_off[name]
            used[off:off + (int(np.prod(shape)) if len(shape) else 1)] = True
        # as many entries as parameter elements, every element has one, none outside: exactly one each
        assert total[0] == int(used.sum()) and (tab[used] >= 0).all() and (tab[~used] < 0).all(), \
            "every WavUnet parameter has exactly one packed-gradient entry"
        self.unpack_entries = (tab >= 0).astype(np.int8)
        return tab


class WavUnetDeviceTables:
    def __init__(self, st: WavUnetStatic, device):
        f = lambda a: torch.from_numpy(a).to(device)
        self.wtab, self.btab, self.ntab, self.utab1 = f(st.wtab), f(st.btab), f(st.ntab), f(st.utab1)
        self.tensor_offsets = f(st.layout.tensor_offsets)
        self.wpack = torch.zeros(st.n_wpack, dtype=BF16, device=device)
        self.bpack = torch.zeros(st.n_bpack, dtype=torch.float32, device=device)


def valid_lengths(T, n):
    """the nearest clip lengths below and above T that the n-layer network takes: multiples of 2^n with at least two middle frames"""
    m = 2 ** n
    lo = max(2 * m, T // m * m)
    hi = max(2 * m, -(-T // m) * m)
    return lo, hi


class WavUnetWorkspace(GemmWorkspace):
    def __init__(self, st: WavUnetStatic, tables: WavUnetDeviceTables, B, T, device):
        super().__init__()
        cfg = st.cfg
        n = cfg.n
        if T % 2 ** n or T // 2 ** n < 2:
            lo, hi = valid_lengths(T, n)
            raise SehipError(f"WavUnet: a clip of T={T} samples does not fit {n} layers: T must be a multiple of 2^{n} = {2 ** n} with at least "
                             f"two frames in the middle block (the reference fails in torch.cat otherwise); nearest valid lengths: {lo}"
                             + (f" and {hi}" if hi != lo else ""))
        if B < 1 or B > 65535:
            raise SehipError(f"WavUnet: batch size B={B} must be in 1 .. 65535")
        self.st, self.tb, self.B, self.T, self.device = st, tables, B, T, device
        self.lens = [T >> l for l in range(n + 1)]
        lib = _lib.lib()
        self.bufs = {}
        for name, (level, c) in st.buffers.items():
            self.bufs[name] = Buf(torch.zeros(B, self.lens[level], 1, c, dtype=BF16, device=device), self.lens[level], 1, c)
        self.out = torch.zeros(B, 1, T, dtype=torch.float32, device=device)
        self.coef = {k: torch.zeros(nm["C"], 4, dtype=torch.float32, device=device) for k, nm in st.norms.items()}
        self.bcoef = {k: torch.zeros(nm["C"], 4, dtype=torch.float32, device=device) for k, nm in st.norms.items()}
        # one row of partial sums per workgroup; every layer its own (the op-local tests read them back)
        self.part = {k: torch.zeros(int(lib.sehip_wun_bn_scratch_floats(B * self.lens[nm["level"]], nm["C"])), dtype=torch.float32, device=device)
                     for k, nm in st.norms.items()}
        self.bpart = {k: torch.zeros_like(v) for k, v in self.part.items()}
        self.enc0_scratch = torch.zeros(int(lib.sehip_wun_enc0_wgrad_scratch_floats(B, T, cfg.ci)), dtype=torch.float32, device=device)
        self.out_scratch = torch.zeros(int(lib.sehip_wun_out_bwd_scratch_floats(B * T, cfg.ci)), dtype=torch.float32, device=device)
        self.gpack = torch.zeros(st.n_gpack, dtype=torch.float32, device=device)
        self.wav = None
        self.training = True
        self._bwd_clean = False
        self.side = self._side_stream = self._new_side_stream(device)
        self._bind()

    def _view(self, name, pair):
        b = self.bufs[name]
        if not pair:
            return b.Tst, b.C
        assert b.Tst % 2 == 0
        return b.Tst // 2, 2 * b.C

    def _bind(self):
        st, tb, B = self.st, self.tb, self.B
        self.desc = {}
        kt = st.ktab.copy()
        for p in st.prods.values():
            bind_chunk_table(st.ktab, kt, p.kt_off, p.K // 8, [(1, self._view(*s)[1]) for s in p.srcs])
        self.ktab_dev = torch.from_numpy(kt).to(self.device)
        for name, p in st.prods.items():
            d = CGemmDesc()
            tt = self.lens[p.level]
            for q, s in enumerate(p.srcs):
                sT, sC = self._view(*s)
                assert sT == tt, (name, s, sT, tt)
                d.src[q].ptr, d.src[q].T, d.src[q].F, d.src[q].C, d.src[q].tlo, d.src[q].thi = self.bufs[s[0]].ptr, sT, 1, sC, 0, sT
            for q, (bname, cols) in enumerate(p.dsts):
                ob = self.bufs[bname]
                assert ob.Tst == tt and ob.C == cols, (name, bname)
                d.dst[q].ptr, d.dst[q].T, d.dst[q].F, d.dst[q].C = ob.ptr, tt, 1, ob.C
                d.dst[q].toff, d.dst[q].fmul, d.dst[q].fadd, d.dst[q].tmul, d.dst[q].is_f32 = 0, 1, 0, 1, 0
            d.ktab = self.ktab_dev.data_ptr() + 16 * p.kt_off
            d.ntab = tb.ntab.data_ptr() + 16 * p.nt_off
            d.W = tb.wpack.data_ptr() + 2 * p.w_off
            if p.b_off is not None:
                d.bias = tb.bpack.data_ptr() + 4 * p.b_off
            d.M, d.N, d.Npad, d.K = B * tt, p.N, p.Npad, p.K
            d.TT, d.J, d.fmul, d.tmul = tt, 1, 1, 1
            self.desc[name] = d
            if p.dw_off is not None:
                w = CGemmDesc.from_buffer_copy(d)
                w.dW = self.gpack.data_ptr() + 4 * p.dw_off
                w.dbias = self.gpack.data_ptr() + 4 * p.db_off
                gb = self.bufs[p.dout]
                assert gb.Tst == tt and gb.C == p.N, (name, p.dout)
                w.dst[0].ptr = gb.ptr
                self.desc[name + ".wg"] = w

    # ---- launches (gemm, wgrad: GemmWorkspace) ------------------------------------------------------------------------
    def _norm_coef(self, key, params, buffers, nbt, training):
        """batch (training) or running (eval) statistics of layer `key` -> its coefficient records"""
        nm, L = self.st.norms[key], self.st.layout
        y, pre = self.bufs[nm["y"]], nm["pre"]
        rows = self.B * y.Tst
        if training:
            call("sehip_wun_bn_stats", y.ptr, rows, nm["C"], ptr(self.part[key]), stream())
        call("sehip_wun_bn_finalize", ptr(self.part[key]), y.ptr, self._pp(params, pre + "1.weight"), self._pp(params, pre + "1.bias"),
             buffers.data_ptr() + 4 * L.buffer_off[pre + "1.running_mean"][0], buffers.data_ptr() + 4 * L.buffer_off[pre + "1.running_var"][0],
             nbt.data_ptr() + 8 * L.nbt_idx[pre + "1.num_batches_tracked"], rows, nm["C"], BN_EPS, BN_MOMENTUM, 1 if training else 0,
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
        st, cfg, b, tb = self.st, self.st.cfg, self.bufs, self.tb
        B, T, n, c0 = self.B, self.T, cfg.n, cfg.ci
        pp = lambda nme: self._pp(params, nme)
        self.wav, self.training = wav, bool(training)
        call("sehip_zero_regions", ptr(self.gpack), self.gpack.numel() * 4, None, 0, None, 0, None, 0, stream())
        self._bwd_clean = True
        call("sehip_pack_bf16", ptr(params), ptr(tb.wtab), st.n_wpack, ptr(tb.wpack), stream())
        call("sehip_pack_f32", ptr(params), ptr(tb.btab), st.n_bpack, ptr(tb.bpack), stream())
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
        st, cfg, b, tb = self.st, self.st.cfg, self.bufs, self.tb
        B, T, n, c0 = self.B, self.T, cfg.n, cfg.ci
        pp = lambda nme: self._pp(params, nme)
        gp = lambda off: self.gpack.data_ptr() + 4 * off
        if not self._bwd_clean:            # a second backward pass over the same forward
            self.gpack.zero_()
        self._bwd_clean = False
        self._chain_dirty = True
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
        self.join_side()
        np_ = st.layout.n_params
        if tail is not None:      # FlatOptimizer's accumulators: the un-pack also takes the clipping norm / metric sums
            call("sehip_unpack_grad1_sums", ptr(self.gpack), ptr(tb.utab1), np_, ptr(grads), tail[2], tail[3], tail[0], tail[1], tail[4],
                 None, stream())
        else:
            call("sehip_unpack_grad1", ptr(self.gpack), ptr(tb.utab1), np_, ptr(grads), stream())
        return grads
