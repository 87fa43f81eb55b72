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
readback.  graph=True captures that chain once (torch.cuda.graph) and feed() copies into a static input and replays.
"""
import ctypes as C

import torch

from .._lib import SehipError, call, ptr, stream, stream_scope
from ..gemmdesc import BF16, fill_desc, row_ptr, upload_chunk_table
from .conv_tasnet import ConvTasNet


def state_bytes_of(cfg, streams):
    """Bytes of carried state of `streams` streams (host arithmetic): both halves of carry, history and tail, pos, and the phase word."""
    h = cfg.L // 2
    hist_rows = sum((cfg.P - 1) * 2 ** x for _, x in cfg.blocks())
    per_stream = 2 * (cfg.audio_channels * h * 4 + hist_rows * cfg.H * 2 + cfg.C * cfg.audio_channels * h * 4) + 4
    return streams * per_stream + 4


def check_feed_input(x, streams, audio_channels, samples, device):
    """feed()'s argument check (before any launch): x [streams, audio_channels, samples] fp32 on `device`."""
    if not isinstance(x, torch.Tensor):
        raise SehipError(f"ConvTasNetStreamer.feed: x must be a tensor, got {type(x).__name__}")
    want = (streams, audio_channels, samples)
    if tuple(x.shape) != want:
        raise SehipError(f"ConvTasNetStreamer.feed: x must have shape [streams, audio_channels, chunk_frames * L/2] = {list(want)}, "
                         f"got {list(x.shape)}")
    if x.dtype != torch.float32:
        raise SehipError(f"ConvTasNetStreamer.feed: x must have dtype torch.float32, got {x.dtype}")
    if x.device != device:
        raise SehipError(f"ConvTasNetStreamer.feed: x must be on device {device} (the model's), got {x.device}")


class ConvTasNetStreamer:
    def __init__(self, model, streams=1, chunk_frames=1, graph=False):
        if not isinstance(model, ConvTasNet):
            raise SehipError(f"ConvTasNetStreamer: model must be a sehip.model.ConvTasNet, got {type(model).__name__}")
        cfg = model.cfg
        if not cfg.causal:
            raise SehipError("ConvTasNetStreamer: model was built with causal=False: its depthwise convolutions read future frames, "
                             "only causal=True, norm_type='cLN' can run chunk by chunk")
        if cfg.norm_type != "cLN":
            raise SehipError(f"ConvTasNetStreamer: model was built with norm_type={cfg.norm_type!r}: gLN's statistics span the whole clip, "
                             "so no frame is final before the clip ends; only causal=True, norm_type='cLN' can run chunk by chunk")
        if not isinstance(streams, int) or streams < 1:
            raise SehipError(f"ConvTasNetStreamer: streams={streams!r} must be an integer >= 1")
        if not isinstance(chunk_frames, int) or chunk_frames < 1:
            raise SehipError(f"ConvTasNetStreamer: chunk_frames={chunk_frames!r} must be an integer >= 1")
        dev = model.flat_params.device
        if dev.type != "cuda":
            raise SehipError(f"ConvTasNetStreamer: model is on {dev}: the HIP path needs a gfx950 GPU (no CPU fallback); "
                             "call model.to('cuda') first")
        self.model, self.cfg, self.st, self.device = model, cfg, model.static, dev
        self.streams, self.chunk_frames, self.graph = streams, chunk_frames, bool(graph)
        self.delay = cfg.L // 2
        self.chunk_samples = chunk_frames * self.delay
        self.state_bytes = state_bytes_of(cfg, streams)
        self._alloc()
        self._bind()
        self._graph = None
        self._epoch = None
        self._sync_model()

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
        self._calls = 0          # host mirror of `phase`: flush() reads the current half of the tail
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

    def _sync_model(self):
        if self._epoch != self.model.storage_epoch:
            if self.model.flat_params.device != self.device:
                raise SehipError(f"ConvTasNetStreamer: model moved from {self.device} to {self.model.flat_params.device}; build a new streamer")
            self.refresh_weights()
            self._graph = None          # (captured launches hold pointers into the old flat parameters)
            self._epoch = self.model.storage_epoch

    # ---- one chunk -----------------------------------------------------------------------------------
    def _chunk(self):
        """xin -> out, state advanced: the chain of launches on the current stream"""
        st, cfg, a = self.st, self.cfg, self.act
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

    def _capture(self):
        call("sehip_init")
        torch.cuda.synchronize(self.device)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g), stream_scope():          # (records, runs nothing: the state does not move; the scope: the capturing stream)
            self._chunk()
        return g

    def feed(self, x):
        """x [S, ac, Kc * L/2] fp32 on the model's device -> [S, C, ac, Kc * L/2]: the offline output of the samples fed so far, delayed
        by L/2 samples."""
        check_feed_input(x, self.streams, self.cfg.audio_channels, self.chunk_samples, self.device)
        with torch.no_grad(), stream_scope():
            self._sync_model()
            self.xin.copy_(x)
            if self.graph:
                if self._graph is None:
                    self._graph = self._capture()
                self._graph.replay()
            else:
                self._chunk()
            self._calls += 1
            return self.out.clone()

    def flush(self):
        """The last L/2 samples of every stream [S, C, ac, L/2] (the carried tail: no compute); then all streams are reset."""
        with torch.no_grad():
            t = self.tail[self._calls & 1].clone()
            self.reset()
            return t

    def reset(self, which=None):
        """Starts a new call on all streams (which=None) or on those of an index list / bool mask [S]: pos = -1, both carries zero.  The
        other streams are untouched.  (The depthwise history needs no clearing: all of its rows have negative frame indices then.)"""
        with torch.no_grad():
            if which is None:
                idx = slice(None)
            else:
                idx = torch.as_tensor(which, device=self.device)
                if idx.dtype == torch.bool:
                    if tuple(idx.shape) != (self.streams,):
                        raise SehipError(f"ConvTasNetStreamer.reset: which as a bool mask must have shape [{self.streams}], got {list(idx.shape)}")
                else:
                    idx = idx.reshape(-1).long()
                    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= self.streams):
                        raise SehipError(f"ConvTasNetStreamer.reset: which holds a stream index outside [0, {self.streams})")
            self.pos[idx] = -1
            self.carry[:, idx] = 0
            self.tail[:, idx] = 0
