"""Host-side plan of the U-Net train step on libsehip (reference: src/model/unet.py:9-146; `unet` of the registry).

Activations are channels-last bf16 ``[R][T_l][F_l][C]`` with frames = T, rows per frame = F and T_l = T >> l, F_l = F >> l (the floor of
MaxPool2d(2)); level L = unet_layer holds the middle block.  ``amp`` and every unet_channels-wide tensor of the head are stored Cp =
unet_channels rounded up to 8 channels wide, the padding channels exact zeros.  The spectrum, the output and the incoming gradient stay
fp32 ``[R][uc][F][T][2]``.

Every convolution is a product of the implicit-GEMM engine (csrc/gemm.hip, generic kernels):
  * Conv3x3 (pad 1, no bias): nine taps through the chunk table, the engine's zero fill outside [0, T) x [0, F) as the padding; K = 9 C
    padded to a multiple of 64 with empty chunks.  A concatenation is two sources; the input gradient of a decoder's first convolution
    has two destinations (d up | d skip);
  * the gradient that reaches a pooled tensor is the next block's input gradient plus the skip half of a concat gradient: the
    descriptor's `res` field adds the second to the first in the product that writes it;
  * ConvTranspose2d(2, 2): four parity-class 1x1 products scattered with dst.tmul = 2 / fmul = 2 / toff / fadd; its input gradient is
    ONE product that gathers the four parities (descriptor tmul = fmul = 2, K = 4 C_out); the weight gradients come from the forward
    descriptors (dOut = the scattered destination).  The far-end pad frame / row of an `up` buffer is zero from allocation and never
    written; its bias goes through the descriptor, the four classes' bias sums land in one region;
  * weight gradients: the same descriptors with dOut as the second operand, on the side stream.
Everything else is csrc/unet.hip (+ sehip_wun_bn_stats / sehip_wun_bn_bwd_finalize of csrc/wavunet.hip; the sums of both files are
csrc/clbn.h).  The full-resolution output
of an encoder block has one reader, MaxPool2d(2): sehip_unet_bn_act_pool applies BatchNorm, LeakyReLU, dropout and the pool in one pass
and never stores it.

The product graph itself (Prod, the arenas, the un-pack table, the bound descriptors with their canary bands, prologue and un-pack) is
sehip/prodgraph.py, shared with plan_wavunet.py; this module holds the network's own products, its shape refusals and its launch sequence.
"""
import numpy as np
import torch

from ._lib import call, ptr, stream, SehipError
from .plan_rnnmask import drop_threshold
from .prodgraph import ProdDeviceTables, ProdStatic, ProdWorkspace

BN_EPS, BN_MOMENTUM, WIDTH0 = 1e-5, 0.1, 16
MAX_LAYERS = 4
DROP_ENCODER, DROP_MIDDLE = 0, 1          # the `layer` word of the two dropout sites' keys


def pad8(n):
    return (n + 7) // 8 * 8


class UNetConfig:
    """Constructor arguments of the reference model (src/model/unet.py:10) and what of them is built."""

    def __init__(self, unet_channels=None, unet_layer=4, bilinear=False, unet_dropout=0.5, **_ignored):
        def bad(arg, val, why):
            raise SehipError(f"sehip UNet: {arg}={val!r} {why}")
        if unet_channels is None:
            bad("unet_channels", None, "has no HIP path yet: the reference's constructor has no default for it (UNet() is a TypeError "
                "there); give an integer in 1 .. 15")
        if isinstance(unet_channels, bool) or not isinstance(unet_channels, int) or not 1 <= unet_channels <= 15:
            bad("unet_channels", unet_channels, "must be an integer in 1 .. 15 (the reference asserts unet_channels < 16)")
        if isinstance(unet_layer, bool) or not isinstance(unet_layer, int) or not 1 <= unet_layer <= MAX_LAYERS:
            bad("unet_layer", unet_layer, f"must be an integer in 1 .. {MAX_LAYERS}")
        if bilinear:
            bad("bilinear", bilinear, "has no HIP path yet: the transposed-convolution decoder (bilinear: False, the shipped setting) is built")
        if isinstance(unet_dropout, bool) or not isinstance(unet_dropout, (int, float)) or not 0.0 <= float(unet_dropout) <= 1.0:
            bad("unet_dropout", unet_dropout, "must be a probability in [0, 1] (the p of the two dropout sites, 0.5 in the reference)")
        self.uc, self.L, self.p = unet_channels, unet_layer, float(unet_dropout)
        self.Cp = pad8(unet_channels)
        self.width = [WIDTH0 << l for l in range(unet_layer + 1)]          # encoder block l -> width[l]; the middle -> width[L]

    def key(self):
        return (self.uc, self.L, self.p)

    def param_specs(self):
        """[(name, shape, kind)] in the reference's state_dict() order (named_parameters() is the same without the buffers)."""
        out = []

        def bn(pre, c):
            out.append((pre + "weight", (c,), "param")); out.append((pre + "bias", (c,), "param"))
            out.append((pre + "running_mean", (c,), "buffer")); out.append((pre + "running_var", (c,), "buffer"))
            out.append((pre + "num_batches_tracked", (), "nbt"))

        def double_conv(pre, cin, cmid, cout):
            out.append((pre + "0.weight", (cmid, cin, 3, 3), "param")); bn(pre + "1.", cmid)
            out.append((pre + "3.weight", (cout, cmid, 3, 3), "param")); bn(pre + "4.", cout)

        def up(pre, cin):
            out.append((pre + "weight", (cin, cin // 2, 2, 2), "param")); out.append((pre + "bias", (cin // 2,), "param"))

        L, w, uc = self.L, self.width, self.uc
        for l in range(L):
            double_conv(f"encoder.{l}.maxpool_conv.0.double_conv.", uc if l == 0 else w[l - 1], w[l], w[l])
        double_conv("middle.double_conv.", w[L - 1], w[L], w[L])
        for n in range(L):
            cin = w[L - n]
            if n > 0:
                up(f"decoder.{n}.up.", cin)
            double_conv(f"decoder.{n}.conv.double_conv.", cin + w[L - 1] if n == 0 else cin, w[L - 1 - n], w[L - 1 - n])
        up("outconv.up.", w[0])
        double_conv("outconv.conv.double_conv.", w[0] // 2 + uc, uc, uc)
        return out


def conv3_tables(w, srcs, co_s):
    """forward product of a 3x3 convolution, weight index array w [co][sum of real source channels][kF][kT]; srcs [(real, stored
    channels)] in concatenation order -> (chunk rows, widx [co_s][9 sum stored])"""
    co_r = w.shape[0]
    rows, cols = [], []
    for a in range(3):              # frame (T) tap = kT
        for b in range(3):          # row (F) tap = kF
            c0 = 0
            for s, (cr, cs) in enumerate(srcs):
                blk = np.full((co_s, cs), -1, dtype=np.int64)
                blk[:co_r, :cr] = w[:, c0:c0 + cr, b, a]
                cols.append(blk)
                rows += [(s, a - 1, b - 1, 8 * q) for q in range(cs // 8)]
                c0 += cr
    assert c0 == w.shape[1]
    return rows, np.concatenate(cols, 1)


def conv3_dgrad_tables(w, srcs, ndst, co_s):
    """input gradient towards the first ndst sources: rows over dy [co_s], widx [sum stored of those sources][9 co_s]"""
    co_r = w.shape[0]
    rows, cols = [], []
    ntot = sum(cs for _, cs in srcs[:ndst])
    for a in range(3):
        for b in range(3):
            blk = np.full((ntot, co_s), -1, dtype=np.int64)
            c0 = r0 = 0
            for cr, cs in srcs[:ndst]:
                blk[r0:r0 + cr, :co_r] = w[:, c0:c0 + cr, b, a].T
                c0 += cr; r0 += cs
            cols.append(blk)
            rows += [(0, 1 - a, 1 - b, 8 * q) for q in range(co_s // 8)]
    return rows, np.concatenate(cols, 1)


class UNetStatic(ProdStatic):
    """Products, packed-weight layout and gradient un-packing table (independent of R, T, F).  A product's sources are buffer names."""
    plan_name = "UNet"

    def __init__(self, cfg: UNetConfig):
        super().__init__(cfg)
        ia = self.layout.index_array
        L, w, uc, Cp = cfg.L, cfg.width, cfg.uc, cfg.Cp
        buf, prod, norm = self.buf, self.prod, self.norm

        def double_conv(key, pre, srcs, mid, out, level, dg=None, res=None):
            """srcs [(buffer, real, stored)]; mid / out (real, stored); dg: [buffer names] the first convolution's input gradient goes
            to (one per leading source), res: added to the first"""
            (mr, ms), (orl, os_) = mid, out
            for nm, c in (("y1", ms), ("z1", ms), ("dy1", ms), ("dz1", ms), ("y2", os_), ("dy2", os_)):
                buf(f"{key}.{nm}", level, c)
            geo = [(cr, cs) for _, cr, cs in srcs]
            w1, w2 = ia(pre + "0.weight"), ia(pre + "3.weight")
            rows, widx = conv3_tables(w1, geo, ms)
            prod(key + ".c1", rows, widx, [b for b, _, _ in srcs], [(key + ".y1", ms)], level, dout=key + ".dy1")
            if dg:
                rows, widx = conv3_dgrad_tables(w1, geo, len(dg), ms)
                prod(key + ".c1.dg", rows, widx, [key + ".dy1"], [(b, cs) for b, (_, cs) in zip(dg, geo)], level, kind="dgrad", res=res)
            rows, widx = conv3_tables(w2, [(mr, ms)], os_)
            prod(key + ".c2", rows, widx, [key + ".z1"], [(key + ".y2", os_)], level, dout=key + ".dy2")
            rows, widx = conv3_dgrad_tables(w2, [(mr, ms)], 1, os_)
            prod(key + ".c2.dg", rows, widx, [key + ".dy2"], [(key + ".dz1", ms)], level, kind="dgrad")
            norm(key + ".n1", pre + "1.", ms, level, key + ".y1", cr=mr)
            norm(key + ".n2", pre + "4.", os_, level, key + ".y2", cr=orl)

        def up(key, pre, src, dsrc, cin, level):
            """ConvTranspose2d(cin -> cin / 2, k = 2, s = 2) from `src` (level + 1) into key.up (level); d key.up -> dsrc"""
            co = cin // 2
            buf(key + ".up", level, co); buf(key + ".dup", level, co)
            wt = ia(pre + "weight")                                          # [cin][co][kF][kT]
            chunks = [(0, 0, 0, 8 * q) for q in range(cin // 8)]
            for a in range(2):          # frame parity = kT
                for b in range(2):      # row parity = kF
                    prod(f"{key}.up{a}{b}", chunks, wt[:, :, b, a].T, [src], [(key + ".up", co)], level + 1, bias=ia(pre + "bias"),
                         dout=key + ".dup", scatter=(a, b), bias_key=key + ".up")
            rows = [(0, a, b, 8 * q) for a in range(2) for b in range(2) for q in range(co // 8)]
            widx = np.concatenate([wt[:, :, b, a] for a in range(2) for b in range(2)], 1)      # [cin][(a, b, co)]
            prod(key + ".up.dg", rows, widx, [key + ".dup"], [(dsrc, cin)], level + 1, kind="dgrad", stride=(2, 2))

        buf("amp", 0, Cp)
        x, xr, xs = "amp", uc, Cp
        for l in range(L):
            k = f"e{l}"
            buf(f"p{l}", l + 1, w[l]); buf(f"dp{l}", l + 1, w[l]); buf(f"ds{l}", l + 1, w[l])
            double_conv(k, f"encoder.{l}.maxpool_conv.0.double_conv.", [(x, xr, xs)], (w[l], w[l]), (w[l], w[l]), l,
                        dg=[f"dp{l - 1}"] if l > 0 else None, res=f"ds{l - 1}" if l > 0 else None)
            x, xr, xs = f"p{l}", w[l], w[l]
        buf("m.z2", L, w[L]); buf("m.dz2", L, w[L])
        double_conv("m", "middle.double_conv.", [(x, xr, xs)], (w[L], w[L]), (w[L], w[L]), L, dg=[f"dp{L - 1}"], res=f"ds{L - 1}")
        prev, dprev = "m.z2", "m.dz2"
        for n in range(L):
            k, lv, cin, co = f"d{n}", L - n, w[L - n], w[L - 1 - n]
            skip = f"p{L - 1 - n}"
            buf(k + ".z2", lv, co); buf(k + ".dz2", lv, co)
            if n == 0:
                first, dfirst, cf = prev, dprev, cin
            else:
                up(k, f"decoder.{n}.up.", prev, dprev, cin, lv)
                first, dfirst, cf = k + ".up", k + ".dup", cin // 2
            double_conv(k, f"decoder.{n}.conv.double_conv.", [(first, cf, cf), (skip, co, co)], (co, co), (co, co), lv,
                        dg=[dfirst, f"ds{L - 1 - n}"])
            prev, dprev = k + ".z2", k + ".dz2"
        up("o", "outconv.up.", prev, dprev, w[0], 0)
        buf("o.dz2", 0, Cp)
        # (amp takes no gradient: the mixture is data)
        double_conv("o", "outconv.conv.double_conv.", [("o.up", w[0] // 2, w[0] // 2), ("amp", uc, Cp)], (uc, Cp), (uc, Cp), 0, dg=["o.dup"])

        self._assemble()


UNetDeviceTables = ProdDeviceTables


class UNetWorkspace(ProdWorkspace):
    """Buffers and bound descriptors for inputs [R, uc, F, T, 2].  `guard` > 0 (tests): every activation buffer sits between two bands
    of that many canary elements inside its allocation."""

    def __init__(self, st: UNetStatic, tables: UNetDeviceTables, R, F, T, device, guard=0):
        cfg = st.cfg
        L = cfg.L
        if F < 2 ** L or T < 2 ** L:
            raise SehipError(f"UNet: an input of F={F} bins x T={T} frames does not fit unet_layer={L}: F and T must be at least 2^{L} = "
                             f"{2 ** L} (the reference fails inside max_pool2d below that)")
        if R < 1 or R * (cfg.Cp // 8) > 65535:
            raise SehipError(f"UNet: R={R} items (batch x audio channels) must be in 1 .. {65535 // (cfg.Cp // 8)}")
        if R * T * F * max(cfg.width[0], cfg.Cp) > 2 ** 32:
            raise SehipError(f"UNet: an activation of R={R} x T={T} x F={F} x {max(cfg.width[0], cfg.Cp)} channels has more than 2^32 elements (the "
                             "dropout index and the row counters are 32 bits wide)")
        if T >= 2 ** 15 or F >= 2 ** 15:
            raise SehipError(f"UNet: F={F}, T={T} must be below 32768 (16-bit offsets of the engine's chunk table)")
        self.R, self.F, self.T = R, F, T
        super().__init__(st, tables, R, [T >> l for l in range(L + 1)], [F >> l for l in range(L + 1)], device, guard=guard)
        self.code = {l: self._make(f"code{l}", (R, self.Tl[l + 1], self.Fl[l + 1], cfg.width[l] // 8), torch.int16) for l in range(L)}
        self.out = torch.zeros(R, cfg.uc, F, T, 2, dtype=torch.float32, device=device)
        self.ctr_used = torch.zeros(2, dtype=torch.int32, device=device)
        self.spec = None
        self.training, self.dropping, self.seed = True, False, 0

    # ---- launches (gemm, wgrad: GemmWorkspace) ------------------------------------------------------------------------
    def _drop(self, site):
        """the dropout arguments of a site (None: no dropout there)"""
        if site is None or not self.dropping:
            return (0, 0, None, 0, 0, 1.0)
        thresh, scale = drop_threshold(self.st.cfg.p)
        return (self.seed & 0xFFFFFFFF, (self.seed >> 32) & 0xFFFFFFFF, ptr(self.ctr_used), site, thresh, scale)

    def _norm_coef(self, key, params, buffers, nbt):
        """batch (training) or running (eval) statistics of a layer -> its coefficient records"""
        nm, Lay = self.st.norms[key], self.st.layout
        y, pre, rows = self.bufs[nm["y"]], nm["pre"], self._norm_rows(key)
        if self.training:
            call("sehip_wun_bn_stats", y.ptr, rows, nm["C"], ptr(self.part[key]), stream())
        call("sehip_unet_bn_finalize", ptr(self.part[key]), y.ptr, self._pp(params, pre + "weight"), self._pp(params, pre + "bias"),
             buffers.data_ptr() + 4 * Lay.buffer_off[pre + "running_mean"][0], buffers.data_ptr() + 4 * Lay.buffer_off[pre + "running_var"][0],
             nbt.data_ptr() + 8 * Lay.nbt_idx[pre + "num_batches_tracked"], rows, nm["C"], nm["Cr"], BN_EPS, BN_MOMENTUM,
             1 if self.training else 0, ptr(self.coef[key]), stream())

    def _act(self, key, z, site=None):
        nm = self.st.norms[key]
        call("sehip_unet_bn_act", self.bufs[nm["y"]].ptr, ptr(self.coef[key]), self._norm_rows(key), nm["C"], *self._drop(site), self.bufs[z].ptr,
             stream())

    def _double_conv(self, key, params, buffers, nbt):
        """first convolution, BatchNorm + LeakyReLU, second convolution, its BatchNorm records (the caller applies them)"""
        self.gemm(key + ".c1")
        self._norm_coef(key + ".n1", params, buffers, nbt)
        self._act(key + ".n1", key + ".z1")
        self.gemm(key + ".c2")
        self._norm_coef(key + ".n2", params, buffers, nbt)

    def _up(self, key):
        for a in range(2):
            for b in range(2):
                self.gemm(f"{key}.up{a}{b}")

    def forward(self, spec, params, buffers, nbt, seed=0, counter=None, training=True):
        """spec [R, uc, F, T, 2] fp32 on the device -> self.out, same shape."""
        cfg, b = self.st.cfg, self.bufs
        R, F, T, L = self.R, self.F, self.T, cfg.L
        s = stream()
        self.spec, self.training, self.seed = spec, bool(training), int(seed)
        self.dropping = self.training and cfg.p > 0.0
        self._prologue(params)
        if self.dropping:
            if counter is None:
                raise SehipError("UNet.forward: dropout needs the model's step counter")
            call("sehip_rsm_counter_next", ptr(counter), ptr(self.ctr_used), s)
        call("sehip_unet_features", ptr(spec), R, cfg.uc, F, T, cfg.Cp, b["amp"].ptr, s)
        for l in range(L):
            k = f"e{l}"
            self._double_conv(k, params, buffers, nbt)
            call("sehip_unet_bn_act_pool", b[k + ".y2"].ptr, ptr(self.coef[k + ".n2"]), R, self.Tl[l], self.Fl[l], cfg.width[l],
                 *self._drop(DROP_ENCODER if l == L - 1 else None), b[f"p{l}"].ptr, ptr(self.code[l]), s)
        self._double_conv("m", params, buffers, nbt)
        self._act("m.n2", "m.z2", DROP_MIDDLE)
        for n in range(L):
            k = f"d{n}"
            if n > 0:
                self._up(k)
            self._double_conv(k, params, buffers, nbt)
            self._act(k + ".n2", k + ".z2")
        self._up("o")
        self._double_conv("o", params, buffers, nbt)
        call("sehip_unet_mask_fwd", b["o.y2"].ptr, ptr(self.coef["o.n2"]), ptr(spec), R, cfg.uc, F, T, cfg.Cp, ptr(self.out), s)
        return self.out

    def _norm_bwd(self, key, dz, dy, code=None, site=None):
        nm = self.st.norms[key]
        lv = nm["level"]
        y = self.bufs[nm["y"]]
        g = self.gpack.data_ptr() + 4 * nm["goff"]
        geo = (self.R, self.Tl[lv], self.Fl[lv], nm["C"])
        cp = ptr(code) if code is not None else None
        drop = self._drop(site)
        call("sehip_unet_bn_bwd_reduce", self.bufs[dz].ptr, cp, y.ptr, ptr(self.coef[key]), *geo, *drop, ptr(self.bpart[key]), stream())
        call("sehip_wun_bn_bwd_finalize", ptr(self.bpart[key]), ptr(self.coef[key]), self._norm_rows(key), nm["C"], g, g + 4 * nm["C"],
             ptr(self.bcoef[key]), stream())
        call("sehip_unet_bn_bwd_apply", self.bufs[dz].ptr, cp, y.ptr, ptr(self.coef[key]), ptr(self.bcoef[key]), *geo, *drop, self.bufs[dy].ptr,
             stream())
        self._chain_dirty = True

    def _double_conv_bwd(self, key, dz2, code=None, site=None):
        """from the gradient at the block's output (dz2: full resolution, or pooled with `code`) to the first convolution's input gradient"""
        self._norm_bwd(key + ".n2", dz2, key + ".dy2", code, site)
        self.wgrad(key + ".c2")
        self.gemm(key + ".c2.dg")
        self._norm_bwd(key + ".n1", key + ".dz1", key + ".dy1")
        self.wgrad(key + ".c1")
        if key + ".c1.dg" in self.desc:
            self.gemm(key + ".c1.dg")

    def _up_bwd(self, key):
        for a in range(2):
            for b in range(2):
                self.wgrad(f"{key}.up{a}{b}")
        self.gemm(key + ".up.dg")

    def backward(self, dout, params, grads, tail=None):
        """dout [R, uc, F, T, 2] fp32 -> flat parameter gradients (overwritten)."""
        if not self.training:
            raise SehipError("UNet.backward in eval mode: the backward pass is built for batch statistics only (call model.train())")
        cfg, b = self.st.cfg, self.bufs
        R, F, T, L = self.R, self.F, self.T, cfg.L
        self._begin_backward()
        call("sehip_unet_mask_bwd", ptr(dout), ptr(self.spec), R, cfg.uc, F, T, cfg.Cp, b["o.dz2"].ptr, stream())
        self._double_conv_bwd("o", "o.dz2")
        self._up_bwd("o")
        for n in range(L - 1, -1, -1):
            k = f"d{n}"
            self._double_conv_bwd(k, k + ".dz2")
            if n > 0:
                self._up_bwd(k)
        self._double_conv_bwd("m", "m.dz2", site=DROP_MIDDLE)
        for l in range(L - 1, -1, -1):
            self._double_conv_bwd(f"e{l}", f"dp{l}", code=self.code[l], site=DROP_ENCODER if l == L - 1 else None)
        return self._unpack(grads, tail)
