"""Chunked streaming inference of DCCRN on libsehip, with a fixed look-ahead delay.

DCCRN is not strictly causal: each of its six decoder layers is a transposed convolution with two time taps followed by `out[..., 1:]`
(src/model/dccrn.py:193-196), so output frame t of a decoder layer reads input frames t and t + 1 -- the network looks LA = 6 frames
ahead -- and a sample is final once the R = win_len / win_inc frames that overlap it are.  A ``DCCRNStreamer`` runs the network chunk
by chunk for S concurrent streams with the delay D = (LA + R - 1) * win_inc samples (900 at 400 / 100)::

    st = DCCRNStreamer(model, streams=S, chunk_frames=Kc, graph=False)
    y = st.feed(x)            # x [S, 1, Kc * win_inc] fp32 on the model's device -> y [S, 1, Kc * win_inc]
    tail = st.flush()         # [S, 1, D]: the rest of the clip with the exact end-of-clip behaviour; then every stream is reset
    st.reset(which=None)      # all streams, or an index list / bool mask
    st.delay, st.chunk_samples, st.state_bytes, st.refresh_weights()

After N samples (a multiple of Kc * win_inc), cat(feeds)[..., D:] followed by flush() is the offline model.eval()(x) of a model built
with length = N, the final clamp included; the first D samples a stream emits are exact zeros.  Forward only.  BatchNorm always uses the
running statistics (whatever model.training says) and never moves them.  The streamer reads the model's flat parameters / running
statistics and the forward product specs of its plan (plan.DCCRNStatic: enc{i}.fwd, ih{l}_{r,i}, proj_{r,i}, dec{j}.fwd{0,1}) but owns
every buffer, descriptor, device table and packed weight it uses (weights in [Npad][K] order: the products run on the engine's generic
gather kernels, whose choice does not depend on the plan's tile layouts): the model's own workspaces are untouched.

Frames.  A chunk fed at frame position pos produces encoder / LSTM frames pos .. pos + Kc - 1, decoder-j frames lagging by j + 1, mask
frames lagging by LA and output hop blocks lagging by LA + R - 1.  Every product reads [history | chunk] buffers (csrc/dccrn_stream.hip):
one history row per encoder-layer input and decoder main input, j + 1 rows of skip 5 - j for decoder j (encoder output i keeps
max(1, 6 - i) rows), LA rows of the fp32 spectrum.  End of clip: flush() sets the device word end[s] = pos[s] + R - 1 and feeds
LA + R - 1 hops of zeros -- the first R - 1 are the reference's right pad; a frame >= end is ABSENT (a zero row for every decoder
product, nothing in the overlap-add), which feeding zeros alone does not reproduce.

A chunk is ONE chain of launches on the current stream (analysis; per encoder layer product + normalise; per LSTM layer two input
products + the recurrence + its state carry; two projections + history; per decoder layer two products (+ normalise); synthesis (two
launches); advance) with the same arguments every time.  Construction, feed(), the capture under graph=True and reset() are ChunkStreamer's.
"""
import ctypes as C

import numpy as np
import torch

from .. import ops
from .._lib import SehipError, call, ptr, stream, stream_scope
from ..gemmdesc import BF16, Arena, enc_entry, fill_desc, row_ptr, upload_chunk_table
from . import streamer
from .dccrn import DCCRN

LA = 6                       # frames of look-ahead: one per decoder layer
NO_END = 2 ** 31 - 1


def delay_of(win_len, win_inc):
    """The streamer's delay in samples: (LA + win_len / win_inc - 1) * win_inc."""
    return (LA + win_len // win_inc - 1) * win_inc


def skip_rows(i):
    """history rows of encoder output i: one for encoder layer i + 1 (the LSTM for i = 5), 6 - i for decoder 5 - i"""
    return max(1, 6 - i)


def state_bytes_of(cfg, streams):
    """Bytes of carried state of `streams` streams (host arithmetic): both halves of every renewed piece, the (h, c) of every recurrence,
    pos and end, and the phase word."""
    kn, pad = cfg.kernel_num, cfg.win_len - cfg.win_inc
    per = 2 * pad * 4 + 2 * pad * 4 + 2 * LA * 257 * 8 + 2 * 256 * 2 * 2
    per += sum(2 * skip_rows(i) * (256 >> (i + 1)) * kn[i + 1] * 2 for i in range(6))
    per += 2 * 4 * kn[6] * 2
    per += sum(2 * (256 >> (5 - j)) * kn[5 - j] * 2 for j in range(5))
    per += cfg.rnn_layers * 4 * cfg.hid * (2 + 4)
    per += 8
    return streams * per + 4


def check_feed_input(x, streams, samples, device):
    """feed()'s argument check (before any launch): x [streams, 1, samples] fp32 on `device`."""
    streamer.check_feed_input("DCCRNStreamer", x, (streams, 1, samples), DCCRNStreamer.SHAPE_WORDS, device)


class DCCRNStreamer(streamer.ChunkStreamer):
    MODEL = DCCRN
    SHAPE_WORDS = "[streams, 1, chunk_frames * win_inc]"
    UNCOUNTED_LAUNCHES = 1           # (the synthesis is two launches)

    @staticmethod
    def _check_cfg(cfg):
        if not cfg.use_clstm:
            raise SehipError("DCCRNStreamer: model was built with use_clstm=False: the carried-state recurrence is built for the complex "
                             "LSTM only")
        if cfg.win_len % cfg.win_inc != 0:
            raise SehipError(f"DCCRNStreamer: win_len={cfg.win_len} is not a multiple of win_inc={cfg.win_inc}: the delay "
                             "(6 + win_len / win_inc - 1) * win_inc needs an integer number of hops per window")

    def _sizes(self):
        cfg = self.cfg
        return delay_of(cfg.win_len, cfg.win_inc), self.chunk_frames * cfg.win_inc, state_bytes_of(cfg, self.streams)

    # ---- product names -------------------------------------------------------------------------------
    def _names(self):
        L = self.cfg.rnn_layers
        return ([f"enc{i}.fwd" for i in range(6)] + [f"ih{l}_{t}" for l in range(1, L + 1) for t in "ri"] + ["proj_r", "proj_i"]
                + [f"dec{j}.fwd{p}" for j in range(6) for p in (0, 1)])

    # ---- own packing tables: every product's weights in [Npad][K] order, biases, recurrent weights -----
    def _tables(self):
        st, cfg, dev = self.st, self.cfg, self.device
        wa, ba = Arena(64), Arena(16)
        self.w_off, self.b_off, self.whh_off = {}, {}, {}
        for name in self._names():
            s = st.specs[name]
            self.w_off[name] = wa.add(enc_entry(s.widx, s.wneg).reshape(-1))
            if s.bias_pairs is not None:
                self.b_off[name] = ba.add(s.bias_pairs)
        ia = st.layout.index_array
        for layer in range(1, cfg.rnn_layers + 1):
            hh = np.stack([ia(f"enhance.{layer - 1}.{part}.weight_hh_l0") for part in ("real_lstm", "imag_lstm")])
            self.whh_off[layer] = wa.add(enc_entry(hh, 0).reshape(-1))
        self.n_wpack, self.n_bpack = wa.size, ba.size
        f = lambda a: torch.from_numpy(a).to(dev)
        self.wtab, self.btab, self.ntab = f(wa.build(np.int32)), f(ba.build(np.int32, 2)), f(st.ntab)
        self.wpack = torch.zeros(self.n_wpack, dtype=BF16, device=dev)
        self.bpack = torch.zeros(self.n_bpack, dtype=torch.float32, device=dev)
        self.window = f(ops.window_of(cfg.win_type, cfg.win_len).astype(np.float32))
        R = cfg.win_len // cfg.win_inc
        # 1 / (window energy + 1e-8) of a fully covered hop: every emitted sample is covered by R frames, so it is periodic in the hop
        self.inv_coff = f(ops.inv_window_energy(cfg.win_len, cfg.win_inc, 2 * R, cfg.win_inc, cfg.win_type))

    # ---- buffers -------------------------------------------------------------------------------------
    def _alloc(self):
        cfg, S, Kc, dev = self.cfg, self.streams, self.chunk_frames, self.device
        kn, hid, L = cfg.kernel_num, cfg.hid, cfg.rnn_layers
        pad = cfg.win_len - cfg.win_inc
        z = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device=dev)
        bz = lambda *shape: z(*shape, dtype=BF16)
        # state
        self.pos = z(S, dtype=torch.int32)
        self.end = torch.full((S,), NO_END, dtype=torch.int32, device=dev)
        self.phase = z(1, dtype=torch.int32)
        self.carry, self.tail = z(2, S, pad), z(2, S, pad)
        self.ring = z(2, S, LA, 257, 2)
        self.enc_hist = bz(2, S, 256, 2)
        self.geo = {}                # layer buffer name -> (history rows H, rows per frame F, channels C)
        for i in range(6):
            self.geo[f"z{i}"] = (skip_rows(i), 256 >> (i + 1), kn[i + 1])
        self.geo["P"] = (1, 4, kn[6])
        for j in range(5):
            self.geo[f"zd{j}"] = (1, 256 >> (5 - j), kn[5 - j])
        self.hist = {n: bz(2, S, H, F, Cc) for n, (H, F, Cc) in self.geo.items()}
        Sp = (S + 3) // 4 * 4
        self.h = {l: bz(4, S, Kc + 1, hid) for l in range(1, L + 1)}
        self.c = {l: z(4, Sp, Kc + 1, hid) for l in range(1, L + 1)}
        # work buffers of one chunk
        self.xin = z(S, 1, Kc * cfg.win_inc)
        self.spec = z(S, Kc, 257, 2)
        self.enc_in = bz(S, 1 + Kc, 256, 2)
        self.y = {n: bz(S, Kc, F, Cc) for n, (H, F, Cc) in self.geo.items()}              # a product's chunk rows
        self.z = {n: bz(S, H + Kc, F, Cc) for n, (H, F, Cc) in self.geo.items()}          # history | chunk
        self.pre = {(l, t): z(S, Kc + 1, 8 * hid) for l in range(1, L + 1) for t in "ri"}
        self.gates = bz(4, Sp, Kc + 1, 4 * hid)       # (records of sehip_lstm_fwd_chunk that nobody reads here: shared by the layers)
        self.mask = z(S, Kc, 256, 2)
        self.frames = z(S, Kc, cfg.win_len)
        self.out = z(S, 1, Kc * cfg.win_inc)
        # eval-mode BatchNorm records (sehip_cbn_finalize, training = 0), one per layer with a BatchNorm
        self.bn_coef = {pre: z(cr, 16) for pre, cr in self.st.bn}
        maxcr = max(cr for _, cr in self.st.bn)
        self.bn_zero, self.bn_dummy, self.bn_part = z(maxcr), z(maxcr), z(64)
        self.mode = {"E": 0, "C": 1, "R": 2}[cfg.masking_mode]

    def _state_tensors(self):
        return ([self.pos, self.end, self.phase, self.carry, self.tail, self.ring, self.enc_hist] + list(self.hist.values())
                + list(self.h.values()) + list(self.c.values()))

    # ---- descriptors ---------------------------------------------------------------------------------
    def _src(self, name, first_row, tlo, thi):
        """source tuple of fill_desc for the history | chunk buffer `name` ("enc_in", a z name, or ("h", layer, combo)): the pointer is
        moved to row first_row, [tlo, thi) are the rows a product may read, counted from there"""
        if isinstance(name, tuple):
            t = self.h[name[1]][name[2]]
            T, F, Cc = self.chunk_frames + 1, 1, self.cfg.hid
        elif name == "enc_in":
            t, T, F, Cc = self.enc_in, self.chunk_frames + 1, 256, 2
        else:
            H, F, Cc = self.geo[name]
            t, T = self.z[name], H + self.chunk_frames
        return (t.data_ptr() + first_row * F * Cc * 2, T, F, Cc, tlo, thi)

    def _bind(self):
        st, cfg, S, Kc = self.st, self.cfg, self.streams, self.chunk_frames
        L, hid = cfg.rnn_layers, cfg.hid
        srcs, dsts = {}, {}
        # encoder layer i reads frames t - 1 and t of its input (chunk-table frame offsets -1, 0): row 0 is the chunk's first frame
        for i in range(6):
            name = "enc_in" if i == 0 else f"z{i - 1}"
            H = 1 if i == 0 else self.geo[name][0]
            srcs[f"enc{i}.fwd"] = [self._src(name, H, -1, Kc)]
            _, F, Cc = self.geo[f"z{i}"]
            dsts[f"enc{i}.fwd"] = [(self.y[f"z{i}"].data_ptr(), Kc, F, Cc, 0, 1, 0, 0, 0)]
        combos = {"r": (0, 3), "i": (2, 1)}
        for tag in "ri":
            srcs[f"ih1_{tag}"] = [self._src("z5", self.geo["z5"][0], 0, Kc)]
            for l in range(2, L + 1):
                srcs[f"ih{l}_{tag}"] = [self._src(("h", l - 1, q), 1, 0, Kc) for q in combos[tag]]
            srcs[f"proj_{tag}"] = [self._src(("h", L, q), 1, 0, Kc) for q in combos[tag]]
            for l in range(1, L + 1):      # the pre-gates of step k + 1 (step 0 of the recurrence's buffers is the carried state)
                p = self.pre[(l, tag)]
                dsts[f"ih{l}_{tag}"] = [(p.data_ptr() + 8 * hid * 4, Kc + 1, 1, 8 * hid, 0, 1, 0, 0, 1)]
            _, F, Cc = self.geo["P"]
            dsts[f"proj_{tag}"] = [(self.y["P"].data_ptr(), Kc, 1, F * Cc, 0, 1, 0, 0, 0)]
        # decoder j, output row k = frame f = pos - (j + 1) + k = in[f + 1] w[kt = 0] + in[f] w[kt = 1]; frame f is row k of both its main
        # input and (behind j + 1 history rows) its skip.  The plan's chunk tables address frame t' - kt of the skip and frame
        # t' - kt (+ 1: stored behind a dropped frame) of the main input, t' = f + 1 (+ 1 more in the last layer, which produces t' - 1)
        for j in range(6):
            main, skip = ("P" if j == 0 else f"zd{j - 1}"), f"z{5 - j}"
            assert self.geo[skip][0] == j + 1 and self.geo[main][0] == 1
            if j == 5:
                sm, ss = self._src(main, -1, 1, Kc + 2), self._src(skip, 0, 0, Kc + 1)
            elif j == 0:
                sm, ss = self._src(main, 1, -1, Kc), self._src(skip, 1, -1, Kc)
            else:
                sm, ss = self._src(main, 0, 0, Kc + 1), self._src(skip, 1, -1, Kc)
            for p in (0, 1):
                srcs[f"dec{j}.fwd{p}"] = [sm, ss]
                if j == 5:
                    dsts[f"dec{j}.fwd{p}"] = [(self.mask.data_ptr(), Kc, 256, 2, 0, 2, p, 0, 1)]
                else:
                    _, F, Cc = self.geo[f"zd{j}"]
                    dsts[f"dec{j}.fwd{p}"] = [(self.y[f"zd{j}"].data_ptr(), Kc, F, Cc, 0, 2, p, 0, 0)]
        specs = [st.specs[n] for n in self._names()]
        self.ktab = upload_chunk_table(st.ktab, specs, lambda s: [(v[2], v[3]) for v in srcs[s.name]], self.device)
        self.desc = {}
        for s in specs:
            for (bname, toff, fmul, fadd), d in zip(s.dsts, dsts[s.name]):
                assert (toff, fmul, fadd) == (d[4], d[5], d[6]), (s.name, bname)
            self.desc[s.name] = fill_desc(srcs[s.name], dsts[s.name], row_ptr(self.ktab, s.kt_off), row_ptr(self.ntab, s.nt_off),
                                          row_ptr(self.wpack, self.w_off[s.name]),
                                          row_ptr(self.bpack, self.b_off[s.name]) if s.name in self.b_off else None,
                                          S * Kc * s.J, s.N, s.Npad, s.K, Kc, s.J, s.fmul, 0)
            # (cv_nf stays 0: the products are not described as regular convolutions, so the engine takes its gather kernels, which
            #  honour T / tlo / thi of a history | chunk source for every row count)

    # ---- weights -------------------------------------------------------------------------------------
    def _bn_args(self, pre, cr):
        lay, m = self.st.layout, self.model
        params, buffers = m.flat_params, m._bflat

        def pp(k):
            f = lay.bn_field(pre, k, cr)
            return ptr(self.bn_zero) if f is None else params.data_ptr() + 4 * (lay.param_off[f[0]][0] + f[1])

        def bp(k):
            f = lay.bn_field(pre, k, cr)
            return ptr(self.bn_dummy) if f is None else buffers.data_ptr() + 4 * (lay.buffer_off[f[0]][0] + f[1])
        return pp, bp

    def refresh_weights(self):
        """Packs the model's current parameters into the streamer's bf16 product weights and fp32 biases and derives the eval-mode
        BatchNorm records from its running statistics (done at construction and when the model's storage moves; call it after
        changing parameters or running statistics in place: only the PReLU slopes are read where they are).  Nothing of the model is
        written."""
        self.model._require_gpu()
        params = self.model.flat_params
        call("sehip_pack_bf16", ptr(params), ptr(self.wtab), self.n_wpack, ptr(self.wpack), stream())
        call("sehip_pack_f32", ptr(params), ptr(self.btab), self.n_bpack, ptr(self.bpack), stream())
        eps = 1e-5 if self.cfg.use_cbn else -1e-5
        for pre, cr in self.st.bn:
            pp, bp = self._bn_args(pre, cr)
            call("sehip_cbn_finalize", ptr(self.bn_part), pp("1.Wrr"), pp("1.Wri"), pp("1.Wii"), pp("1.Br"), pp("1.Bi"), bp("1.RMr"),
                 bp("1.RMi"), bp("1.RVrr"), bp("1.RVri"), bp("1.RVii"), None, 1, cr, eps, 0.1, 0, ptr(self.bn_coef[pre]), stream())

    # ---- one chunk -----------------------------------------------------------------------------------
    def _chunk(self):
        """xin -> out, state advanced: the chain of launches on the current stream"""
        cfg, S, Kc, call = self.cfg, self.streams, self.chunk_frames, self._call
        L, hid = cfg.rnn_layers, cfg.hid
        params, off = self.model.flat_params, self.st.layout.param_off
        ph, pos, end = ptr(self.phase), ptr(self.pos), ptr(self.end)

        def run(name, *args):
            call(name, *args, stream())

        def gemm(name):
            run("sehip_gemm", C.byref(self.desc[name]))

        def norm(buf, pre, lag):
            H, F, Cc = self.geo[buf]
            coef = ptr(self.bn_coef[pre]) if pre else None
            slope = params.data_ptr() + 4 * off[pre + "2.weight"][0] if pre else None
            run("sehip_dcs_norm_hist", ptr(self.y[buf]), coef, slope, ptr(self.hist[buf]), ph, pos, end, lag, S, Kc, H, F, Cc // 2,
                ptr(self.z[buf]))

        run("sehip_dcs_analysis", ptr(self.xin), ptr(self.carry), ph, ptr(self.window), S, Kc, cfg.win_len, cfg.win_inc, ptr(self.spec),
            ptr(self.ring), ptr(self.enc_in), ptr(self.enc_hist))
        for i in range(6):
            gemm(f"enc{i}.fwd")
            norm(f"z{i}", f"encoder.{i}.", 0)
        for l in range(1, L + 1):
            gemm(f"ih{l}_r")
            gemm(f"ih{l}_i")
            run("sehip_lstm_fwd_chunk", ptr(self.pre[(l, "r")]), ptr(self.pre[(l, "i")]), self.wpack.data_ptr() + 2 * self.whh_off[l], S,
                Kc + 1, hid, 1, Kc + 1, ptr(self.h[l]), ptr(self.gates), ptr(self.c[l]))
        gemm("proj_r")
        gemm("proj_i")
        for l in range(1, L + 1):       # (behind the last reader of step Kc of this chunk and of step 0: nothing later reads either)
            run("sehip_dcs_lstm_carry", ptr(self.h[l]), ptr(self.c[l]), S, Kc, hid)
        norm("P", None, 0)
        for j in range(6):
            gemm(f"dec{j}.fwd0")
            gemm(f"dec{j}.fwd1")
            if j < 5:
                norm(f"zd{j}", f"decoder.{j}.", j + 1)
        run("sehip_dcs_synthesis", ptr(self.spec), ptr(self.ring), ptr(self.mask), ptr(self.window), ptr(self.inv_coff), ptr(self.tail), ph,
            pos, end, S, Kc, cfg.win_len, cfg.win_inc, self.mode, ptr(self.frames), ptr(self.out))
        run("sehip_dcs_advance", pos, ph, S, Kc)

    def flush(self):
        """The last `delay` samples of every stream [S, 1, D]: end[s] = pos[s] + R - 1 is marked, then LA + R - 1 hops of zeros are fed
        (whole chunks; the first R - 1 hops are the reference's right pad, frames >= end are absent).  Then all streams are reset."""
        cfg = self.cfg
        R = cfg.win_len // cfg.win_inc
        with torch.no_grad(), stream_scope():
            self._sync_model()
            call("sehip_dcs_mark_end", ptr(self.pos), ptr(self.end), self.streams, R - 1, stream())
            zeros = torch.zeros(self.streams, 1, self.chunk_samples, device=self.device)
            outs = [self._run(zeros) for _ in range(-(-(LA + R - 1) // self.chunk_frames))]
            t = torch.cat(outs, dim=-1)[..., :self.delay].contiguous()
            self.reset()
            return t

    def _clear(self, idx):
        """A new clip on the streams idx: pos = 0, end open, every carried piece zero (both halves)."""
        self.pos[idx] = 0
        self.end[idx] = NO_END
        for t in [self.carry, self.tail, self.ring, self.enc_hist] + list(self.hist.values()):
            t[:, idx] = 0
        hid = self.cfg.hid
        for l in self.h:
            self.h[l][:, idx, 0] = 0
            # the cell-state record of a step is [batch tile][thread]; thread = 64 w + 16 ug + 4 rs + (stream mod 4) (csrc/lstm.hip)
            cv = self.c[l].view(4, -1, self.chunk_frames + 1, hid // 16, 4, 4, 4)
            cv[:, idx // 4, 0, :, :, :, idx % 4] = 0


check_model = DCCRNStreamer.check_args          # the constructor's refusals (before any launch)
