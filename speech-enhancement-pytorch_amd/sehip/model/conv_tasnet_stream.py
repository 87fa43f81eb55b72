"""Chunked streaming inference of the low-latency Conv-TasNet (``ConvTasNet(causal=True, norm_type='cLN')``) on libsehip.

The network looks at no future frame: the encoder reads frames of L samples with hop h = L/2, every cLN is per frame, the depthwise
convolutions look back (P - 1) 2^x frames, the mask is per frame and the decoder overlap-adds a frame with one neighbour.  A
``ConvTasNetStreamer`` runs it chunk by chunk for S concurrent streams with a fixed delay of h samples::

    st = ConvTasNetStreamer(model, streams=S, chunk_frames=Kc, graph=False)
    y = st.feed(x)            # x [S, ac, Kc * h] fp32 on the device -> y [S, C, ac, Kc * h]
    tail = st.flush()         # [S, C, ac, h]: the last h samples; then every stream is reset
    st.reset(which=None)      # all streams, or an index list / bool mask: one call ends, another starts

The concatenated outputs are the offline ``model(x)`` delayed by h samples (the first h samples are zeros).  Forward only.  The streamer
reads the model's flat parameters and the forward product specs of its plan (plan_tasnet.TasNetStatic: bott.fwd, b{i}.in.fwd,
b{i}.pw.fwd, mask.fwd) but owns every buffer, descriptor and packed weight it uses: the model's own workspaces are untouched.

State per stream (csrc/tasnet_stream.hip says why each piece exists twice, [2][...], with one device word `phase` naming the current
half: no launch overwrites what it reads, and a chunk has the same launch arguments every time, so it can be captured):
h carried input samples per audio channel (fp32), the last (P - 1) 2^x rows of h1 of every block (bf16, H wide), the second half of the
last decoded frame [C][ac][h] (fp32), and the frame counter pos (int32, -1 on a fresh stream: the first call's first frame is a
phantom built from the zero carry that contributes nothing).

A chunk is ONE chain of 4 R X + 5 launches (+ 1 with the softmax mask) on the current stream: encoder, bottleneck product, per block
{product, depthwise step, cLN, product with the residual}, mask product, decoder, counter.  No side stream, no allocation, no
readback.  Construction, feed(), the capture of that chain under graph=True and reset() are streamer.ChunkStreamer's.
"""
import ctypes as C

import torch

from .._lib import SehipError, call, ptr, stream
from ..gemmdesc import BF16, fill_desc, row_ptr, upload_chunk_table
from . import streamer
from .conv_tasnet import ConvTasNet


def state_bytes_of(cfg, streams):
    """Bytes of carried state of `streams` streams (host arithmetic): both halves of carry, history and tail, pos, and the phase word."""
    h = cfg.L // 2
    hist_rows = sum((cfg.P - 1) * 2 ** x for _, x in cfg.blocks())
    per_stream = 2 * (cfg.audio_channels * h * 4 + hist_rows * cfg.H * 2 + cfg.C * cfg.audio_channels * h * 4) + 4
    return streams * per_stream + 4


def check_feed_input(x, streams, audio_channels, samples, device):
    """feed()'s argument check (before any launch): x [streams, audio_channels, samples] fp32 on `device`."""
    streamer.check_feed_input("ConvTasNetStreamer", x, (streams, audio_channels, samples), ConvTasNetStreamer.SHAPE_WORDS, device)


class ConvTasNetStreamer(streamer.ChunkStreamer):
    MODEL = ConvTasNet
    SHAPE_WORDS = "[streams, audio_channels, chunk_frames * L/2]"

    @staticmethod
    def _check_cfg(cfg):
        if not cfg.causal:
            raise SehipError("ConvTasNetStreamer: model was built with causal=False: its depthwise convolutions read future frames, "
                             "only causal=True, norm_type='cLN' can run chunk by chunk")
        if cfg.norm_type != "cLN":
            raise SehipError(f"ConvTasNetStreamer: model was built with norm_type={cfg.norm_type!r}: gLN's statistics span the whole clip, "
                             "so no frame is final before the clip ends; only causal=True, norm_type='cLN' can run chunk by chunk")

    def _sizes(self):
        h = self.cfg.L // 2
        return h, self.chunk_frames * h, state_bytes_of(self.cfg, self.streams)

    # ---- buffers and descriptors ---------------------------------------------------------------------
    def _alloc(self):
        cfg, S, Kc, dev, h = self.cfg, self.streams, self.chunk_frames, self.device, self.delay
        ac, N, B, H, Cs = cfg.audio_channels, cfg.N, cfg.B, cfg.H, cfg.C
        z = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device=dev)
        # state
        self.pos = torch.full((S,), -1, dtype=torch.int32, device=dev)
        self.phase = z(1, dtype=torch.int32)
        self.carry = z(2, S, ac, h)
        self.hist = [z(2, S, (cfg.P - 1) * 2 ** x, H, dtype=BF16) for _, x in self.st.blocks]
        self.tail = z(2, S, Cs, ac, h)
        # work buffers of one chunk: the residual stream alternates between two buffers, h1 / h2 / u are shared by all blocks
        self.xin = z(S, ac, Kc * h)
        self.w = z(S, Kc, N)
        row = lambda c: z(S, Kc, c, dtype=BF16)
        self.act = dict(cln=row(N), xa=row(B), xb=row(B), h1=row(H), h2=row(H), u=row(H), mlin=row(Cs * N))
        if cfg.mask_nonlinear == "softmax":
            self.act["msoft"] = row(Cs * N)
        self.out = z(S, Cs, ac, Kc * h)
        # own copies of the plan's device tables and packed weights
        f = lambda a: torch.from_numpy(a).to(dev)
        self.wtab, self.ntab = f(self.st.wtab), f(self.st.ntab)
        self.wpack = z(self.st.n_wpack, dtype=BF16)

    def _state_tensors(self):
        return [self.pos, self.phase, self.carry, self.tail] + self.hist

    def _buf(self, name):
        """activation buffer behind a buffer name of the plan's forward specs"""
        if name[0] == "x" and name[1:].isdigit():
            return self.act["xa" if int(name[1:]) % 2 == 0 else "xb"]
        for k in ("h1", "h2", "u"):
            if name.startswith(k):
                return self.act[k]
        return self.act[name]

    def _names(self):
        nb = len(self.st.blocks)
        return ["bott.fwd"] + [f"b{i}.{k}.fwd" for i in range(nb) for k in ("in", "pw")] + ["mask.fwd"]

    def _bind(self):
        st, S, Kc = self.st, self.streams, self.chunk_frames
        self.ktab = upload_chunk_table(st.ktab, [st.specs[name] for name in self._names()],
                                       lambda s: [(1, self._buf(b).shape[-1]) for b, _ in s.srcs], self.device)
        self.desc = {}
        for name in self._names():
            s = st.specs[name]
            b, o = self._buf(s.srcs[0][0]), self._buf(s.dsts[0][0])
            bc, oc = b.shape[-1], o.shape[-1]
            d = fill_desc([(b.data_ptr(), Kc, 1, bc, 0, Kc)], [(o.data_ptr(), Kc, 1, oc, 0, 1, 0, 1, 0)], row_ptr(self.ktab, s.kt_off),
                          row_ptr(self.ntab, s.nt_off), row_ptr(self.wpack, s.w_off), None, S * Kc, s.N, s.Npad, s.K, Kc, 1, 1, 1,
                          self._buf(s.res).data_ptr() if s.res is not None else None)
            d.dense_rows = 1 if (bc == s.K and oc == s.Npad == s.N) else 0      # (as plan_tasnet.TasNetWorkspace._bind)
            self.desc[name] = d

    # ---- weights -------------------------------------------------------------------------------------
    def refresh_weights(self):
        """Packs the model's current parameters into the streamer's bf16 product weights (done at construction and when the model's
        storage moves; call it after changing the parameters in place)."""
        self.model._require_gpu()
        call("sehip_pack_bf16", ptr(self.model.flat_params), ptr(self.wtab), self.st.n_wpack, ptr(self.wpack), stream())

    # ---- one chunk -----------------------------------------------------------------------------------
    def _chunk(self):
        """xin -> out, state advanced: the chain of launches on the current stream"""
        st, cfg, a, call = self.st, self.cfg, self.act, self._call
        S, Kc, N, H = self.streams, self.chunk_frames, cfg.N, cfg.H
        params, off = self.model.flat_params, self.st.layout.param_off
        pp = lambda n: params.data_ptr() + 4 * off[n][0]
        gemm = lambda n: call("sehip_gemm", C.byref(self.desc[n]), stream())
        net = "separator.network."
        ph, pos = ptr(self.phase), ptr(self.pos)
        call("sehip_ctns_encoder", ptr(self.xin), ptr(self.carry), ph, pp("encoder.conv1d_U.weight"), pp(net + "0.gamma"), pp(net + "0.beta"),
             S, cfg.audio_channels, Kc, N, cfg.L, ptr(self.w), ptr(a["cln"]), stream())
        gemm("bott.fwd")
        for i, (r, x) in enumerate(st.blocks):
            q = f"{net}2.{r}.{x}.net."
            a2, g2, b2 = st.inner[i]
            gemm(f"b{i}.in.fwd")
            call("sehip_ctns_dwconv", ptr(a["h1"]), ptr(self.hist[i]), ph, pos, pp(q + "1.weight"), pp(q + "2.gamma"), pp(q + "2.beta"),
                 pp(q + "3.net.0.weight"), cfg.P, 2 ** x, S, Kc, H, ptr(a["h2"]), stream())
            call("sehip_ctn_cln_apply", ptr(a["h2"]), pp(a2), pp(g2), pp(b2), S, Kc, H, ptr(a["u"]), stream())
            gemm(f"b{i}.pw.fwd")
        gemm("mask.fwd")
        mk = a["mlin"]
        if cfg.mask_nonlinear == "softmax":
            call("sehip_ctn_mask_softmax_fwd", ptr(a["mlin"]), S * Kc, cfg.C, N, ptr(a["msoft"]), stream())
            mk = a["msoft"]
        call("sehip_ctns_decoder", ptr(self.w), ptr(mk), pp("decoder.basis_signals.weight"), ptr(self.tail), ph, pos, S, Kc, N, cfg.L,
             cfg.audio_channels, cfg.C, ptr(self.out), stream())
        call("sehip_ctns_advance", pos, ph, S, Kc, stream())

    def flush(self):
        """The last L/2 samples of every stream [S, C, ac, L/2] (the carried tail: no compute); then all streams are reset."""
        with torch.no_grad():
            t = self.tail[self.chunks & 1].clone()
            self.reset()
            return t

    def _clear(self, idx):
        """A new call on the streams idx: pos = -1, both carries zero.  (The depthwise history needs no clearing: all of its rows have
        negative frame indices then.)"""
        self.pos[idx] = -1
        self.carry[:, idx] = 0
        self.tail[:, idx] = 0
