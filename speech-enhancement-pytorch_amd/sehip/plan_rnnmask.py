"""Host-side plan of the rnn-stft-mask train step on libsehip (reference: src/model/stft_rnn.py:5-119; `rnn-stft-mask` of the registry).

Two things the reference does are not what the names suggest, and both are reproduced:
  * the features are ``|re^2 - im^2|`` (Amplitude, :112-119), not a magnitude; Phase is never called;
  * nn.LSTM / nn.GRU run with batch_first=False on ``[B C][T][F]``: the recurrence walks the L = B C axis and the T frames are its
    independent rows.  The output therefore depends on how a batch is composed.
So every activation here is ``[T][L][channels]`` (row r = t L + l: a frame's L steps are contiguous rows, as the step kernels and the
shifted W_hh weight-gradient product want), bf16 with the channel axes F and S F padded to a multiple of 8 by zeros.

Launch list of one layer: the input projection of all steps and both directions (sehip_rsm_gemm_nt), then L step launches
(sehip_rsm_rnn_fwd).  Backward: L step launches, per direction the two weight-gradient products (sehip_rsm_gemm_tn, the recurrent one
with a row shift of -+1), and the input gradient of both directions in one product.  Weight gradients land in the flat gradient
buffer in the parameters' own layout: there is no packed-gradient buffer and no un-packing table for this model.

That per-layer loop, its weight copies and its buffers are the recurrent stack (stack_arena / stack_pack_launches / stack_buffer_shapes,
RnnStackWorkspace.stack_forward / stack_backward), parametrised by the cell and shared with mel-rnn (sehip/plan_melrnn.py), which adds the
Elman cell (sehip_rsm_elman_fwd / _bwd).
"""
import numpy as np
import torch

from . import _lib
from ._lib import call, ptr, stream, SehipError
from .gemmdesc import ParamLayout, BF16
from .workspace import Workspace

BN_EPS, BN_MOMENTUM = 1e-5, 0.1
GOLDEN = 0x9E3779B9


def pad8(n):
    return (n + 7) // 8 * 8


# ---- the dropout generator's Python twin (csrc/rnnmask.hip: rsm_mix / rsm_key / rsm_keep) -----------------------------------------------
def _mix(x):
    x = np.asarray(x, dtype=np.uint64) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & 0xFFFFFFFF
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def drop_threshold(p):
    """(threshold on the top 24 bits, scale): an element is kept when its bits are >= the threshold"""
    return int(round(float(p) * (1 << 24))), (0.0 if p >= 1.0 else 1.0 / (1.0 - float(p)))


def drop_keep_mask(seed, counter, layer, n, p):
    """bool [n]: what the device keeps of elements 0 .. n-1 of layer `layer`'s output at step counter `counter` (64-bit seed)"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    lo, hi = seed & 0xFFFFFFFF, seed >> 32
    key = _mix(lo ^ int(_mix(hi ^ int(_mix(((int(counter) & 0xFFFFFFFF) * GOLDEN + int(layer)) & 0xFFFFFFFF)))))
    idx = np.arange(n, dtype=np.uint64)
    bits = _mix((_mix(idx ^ key) + GOLDEN) & 0xFFFFFFFF)
    return (bits >> 8) >= drop_threshold(p)[0]


class RnnMaskConfig:
    """Constructor arguments of the reference model (src/model/stft_rnn.py:6-19) and what of them is built."""

    def __init__(self, num_spk=2, audio_channels=2, n_fft=512, hop_length=256, sample_rate=16000, rnn_hidden=256, rnn_layer=2, rnn_type="rnn",
                 drop_out=0.5, activation="relu", bidirectional=False, **_ignored):
        def bad(arg, val, why):
            raise SehipError(f"sehip RNNBaseSTFTMask: {arg}={val!r} {why}")
        if rnn_type == "rnn":
            bad("rnn_type", rnn_type, "(the Elman cell, the constructor's default) has no HIP path yet: 'lstm' and 'gru' are built")
        if rnn_type not in ("lstm", "gru"):
            bad("rnn_type", rnn_type, "must be 'lstm' or 'gru'")
        if not isinstance(rnn_layer, int) or not 1 <= rnn_layer <= 8:
            bad("rnn_layer", rnn_layer, "must be an integer in 1 .. 8")
        if not isinstance(rnn_hidden, int) or rnn_hidden < 32 or rnn_hidden > 1024 or rnn_hidden % 32:
            bad("rnn_hidden", rnn_hidden, "must be a multiple of 32 in 32 .. 1024 (one MFMA covers 32 hidden units of K)")
        if not isinstance(bidirectional, bool):
            bad("bidirectional", bidirectional, "must be True or False")
        if not isinstance(num_spk, int) or not 1 <= num_spk <= 6:
            bad("num_spk", num_spk, "must be an integer in 1 .. 6")
        if not isinstance(audio_channels, int) or audio_channels < 1:
            bad("audio_channels", audio_channels, "must be a positive integer")
        if not isinstance(n_fft, int) or n_fft < 2 or n_fft > 4096 or n_fft % 2:
            bad("n_fft", n_fft, "must be an even integer in 2 .. 4096")
        if not isinstance(drop_out, (int, float)) or isinstance(drop_out, bool) or not 0.0 <= drop_out <= 1.0:
            bad("drop_out", drop_out, "must be a number in [0, 1]")
        if activation != "relu":
            bad("activation", activation, "must be 'relu' (all the reference maps to a module)")
        self.num_spk, self.audio_channels, self.n_fft, self.hop_length, self.sample_rate = num_spk, audio_channels, n_fft, hop_length, sample_rate
        self.rnn_hidden, self.rnn_layer, self.rnn_type, self.drop_out, self.bidirectional = rnn_hidden, rnn_layer, rnn_type, float(drop_out), bidirectional
        self.gru = rnn_type == "gru"
        self.G = 3 if self.gru else 4
        self.GB = 4                                  # blocks of H per direction in dG and the transposed W_ih (the GRU's fourth: r d pre_n)
        self.has_dropout = True                      # a dropped-out copy hd{k} of every layer's output but the last
        self.D = 2 if bidirectional else 1
        self.H = rnn_hidden
        self.Hout = self.D * self.H
        self.F = n_fft // 2 + 1
        self.Fp = pad8(self.F)
        self.SF = num_spk * self.F
        self.SFp = pad8(self.SF)

    def key(self):
        return (self.rnn_type, self.rnn_layer, self.H, self.D, self.num_spk, self.n_fft, self.audio_channels, self.drop_out)

    def layer_in(self, k):
        """(input width, its padded width) of RNN layer k"""
        return (self.F, self.Fp) if k == 0 else (self.Hout, self.Hout)

    def param_specs(self):
        """[(name, shape, kind)] in the reference's state_dict() order"""
        out = []
        for k in range(self.rnn_layer):
            for sfx in ("", "_reverse")[:self.D]:
                out.append((f"rnn.weight_ih_l{k}{sfx}", (self.G * self.H, self.layer_in(k)[0]), "param"))
                out.append((f"rnn.weight_hh_l{k}{sfx}", (self.G * self.H, self.H), "param"))
        c = self.Hout
        out += [("batchnorm.weight", (c,), "param"), ("batchnorm.bias", (c,), "param"), ("batchnorm.running_mean", (c,), "buffer"),
                ("batchnorm.running_var", (c,), "buffer"), ("batchnorm.num_batches_tracked", (), "nbt"),
                ("fc_layers.0.weight", (self.SF, c), "param"), ("fc_layers.0.bias", (self.SF,), "param")]
        return out


# ---- the recurrent stack: the part rnn-stft-mask and mel-rnn share.  A configuration names its cell through G (gates of H in the
# pre-activations: 4 lstm, 3 gru, 1 Elman), GB (blocks of H per direction in dG: 4, 4, 1), gru and, for the Elman cell, elman ----------------
def stack_arena(cfg, w, off):
    """adds the stack's bf16 weight copies to the arena map w ((layer, what) -> element offset) from offset `off`; returns the next offset"""
    G, GB, H, D = cfg.G, cfg.GB, cfg.H, cfg.D
    for k in range(cfg.rnn_layer):
        kin, kp = cfg.layer_in(k)
        for what, n in (("ih", D * G * H * kp),          # [D G H][kp]      operand of the input projection
                        ("ihT", kp * D * GB * H),        # [kp][D][GB][H]   operand of the input gradient (GRU: block 3 stays zero)
                        ("hh", D * G * H * H),           # [D][G H][H]      forward steps
                        ("hhT", D * H * G * H)):         # [D][H][G H]      backward steps
            w[(k, what)] = off
            off += n
    return off


def stack_pack_launches(cfg, w):
    """[(parameter name, row offset in it, N, K, transpose, ld, arena offset)]: the stack's sehip_rsm_pack_w calls of one step"""
    G, GB, H, D = cfg.G, cfg.GB, cfg.H, cfg.D
    out = []
    for k in range(cfg.rnn_layer):
        kin, kp = cfg.layer_in(k)
        for d, sfx in enumerate(("", "_reverse")[:D]):
            ih, hh = f"rnn.weight_ih_l{k}{sfx}", f"rnn.weight_hh_l{k}{sfx}"
            out.append((ih, 0, G * H, kin, 0, kp, w[(k, "ih")] + d * G * H * kp))
            out.append((hh, 0, G * H, H, 0, H, w[(k, "hh")] + d * G * H * H))
            out.append((hh, 0, G * H, H, 1, G * H, w[(k, "hhT")] + d * H * G * H))
            if k > 0:
                out.append((ih, 0, G * H, kin, 1, D * GB * H, w[(k, "ihT")] + d * GB * H))
    return out


def stack_buffer_shapes(cfg, R, T, s):
    """adds the stack's per-batch buffers (R = T L rows) to the map s: name -> (shape, dtype name)"""
    G, GB, H, D, Ho = cfg.G, cfg.GB, cfg.H, cfg.D, cfg.Hout
    elman = getattr(cfg, "elman", False)
    if not elman:
        s["carry"] = ((D, T, H), "f32")
    for k in range(cfg.rnn_layer):
        s[f"pre{k}"] = ((R, D, G, H), "f32")
        if not elman:
            s[f"gates{k}"] = ((R, D, 4, H), "f32")
        s[f"hs{k}"] = ((R, Ho), "bf16")
        s[f"state{k}"] = ((R, Ho), "f32")
        s[f"dG{k}"] = ((R, D, GB, H), "bf16")
        if k < cfg.rnn_layer - 1:
            if cfg.has_dropout:
                s[f"hd{k}"] = ((R, Ho), "bf16")
            s[f"dx{k + 1}"] = ((R, Ho), "bf16")
    return s


class RnnMaskStatic:
    """Parameter layout and the bf16 weight arena (independent of the batch)."""

    def __init__(self, cfg: RnnMaskConfig):
        self.cfg = cfg
        self.layout = ParamLayout(cfg)
        self.w = {}                # (layer, what) -> element offset in the bf16 arena
        off = stack_arena(cfg, self.w, 0)
        self.w["fc"] = off;  off += cfg.SF * cfg.Hout        # [S F][Hout]
        self.w["fcT"] = off; off += cfg.Hout * cfg.SFp       # [Hout][SFp]
        self.n_wpack = off

    def pack_launches(self):
        """[(parameter name, row offset in it, N, K, transpose, ld, arena offset)]: the sehip_rsm_pack_w calls of one step"""
        cfg = self.cfg
        out = stack_pack_launches(cfg, self.w)
        out.append(("fc_layers.0.weight", 0, cfg.SF, cfg.Hout, 0, cfg.Hout, self.w["fc"]))
        out.append(("fc_layers.0.weight", 0, cfg.SF, cfg.Hout, 1, cfg.SFp, self.w["fcT"]))
        return out

    def step_launches(self, L):
        """kernel launches of one training step's recurrence: (forward, backward) step launches over all layers"""
        return self.cfg.rnn_layer * L, self.cfg.rnn_layer * L

    def buffer_shapes(self, B, T):
        """name -> (shape, dtype name) of every per-batch buffer of a workspace for inputs [B, C, F, T, 2]"""
        cfg = self.cfg
        L = B * cfg.audio_channels
        R = T * L
        Ho = cfg.Hout
        s = {"feat": ((R, cfg.Fp), "bf16"), "z": ((R, Ho), "bf16"), "dz": ((R, Ho), "bf16"), "dy": ((R, Ho), "bf16"),
             "mask": ((R, cfg.SFp), "bf16"), "dpre": ((R, cfg.SFp), "bf16"),
             "out": ((B, cfg.num_spk, cfg.audio_channels, cfg.F, T, 2), "f32")}
        return stack_buffer_shapes(cfg, R, T, s)


class RnnStackWorkspace(Workspace):
    """What the workspaces of rnn-stft-mask and mel-rnn share: guarded allocation and the per-layer loop of the recurrent stack
    (projection, steps; steps, weight gradients, input gradient), parametrised by the cell.  A subclass sets st, cfg, T, L, R, device,
    guard, _alloc, bufs, wpack and dropping."""

    def _make(self, name, shape, dtype):
        n = int(np.prod(shape))
        g = self.guard
        if not g:
            return torch.zeros(shape, dtype=dtype, device=self.device)
        g = (g + 7) // 8 * 8                      # the payload keeps its 16-byte alignment
        raw = torch.zeros(n + 2 * g, dtype=dtype, device=self.device)
        raw[:g] = 7.0
        raw[g + n:] = 7.0
        self._alloc[name] = (raw, g, n)
        return raw[g:g + n].view(shape)

    def guards_intact(self):
        """names of the buffers whose canary bands were written"""
        return [k for k, (raw, g, n) in self._alloc.items() if not (bool((raw[:g] == 7.0).all()) and bool((raw[g + n:] == 7.0).all()))]

    def _wp(self, off):
        return self.wpack.data_ptr() + 2 * off

    def _drop_args(self, model_seed, k, active):
        thresh, scale = drop_threshold(self.cfg.drop_out) if active else (0, 1.0)
        return (model_seed & 0xFFFFFFFF, (model_seed >> 32) & 0xFFFFFFFF, ptr(self.ctr_used), k, thresh, scale)

    def stack_forward(self, xin, seed, s):
        """the layers over xin bf16 [R][Fp]; returns the last layer's output hs bf16 [R][Hout]"""
        st, cfg, b = self.st, self.cfg, self.bufs
        R, L, T, H, D, G = self.R, self.L, self.T, cfg.H, cfg.D, cfg.G
        elman = getattr(cfg, "elman", False)
        for k in range(cfg.rnn_layer):
            kin, kp = cfg.layer_in(k)
            call("sehip_rsm_gemm_nt", ptr(xin), kp, self._wp(st.w[(k, "ih")]), kp, R, D * G * H, kp, 0, None, ptr(b[f"pre{k}"]), D * G * H, s)
            if elman:
                call("sehip_rsm_elman_fwd", ptr(b[f"pre{k}"]), self._wp(st.w[(k, "hh")]), ptr(b[f"hs{k}"]), ptr(b[f"state{k}"]), T, L, H, D, s)
                xin = b[f"hs{k}"]
                continue
            drop = self.dropping and k < cfg.rnn_layer - 1
            hd = b[f"hd{k}"] if drop else None
            call("sehip_rsm_rnn_fwd", int(cfg.gru), ptr(b[f"pre{k}"]), self._wp(st.w[(k, "hh")]), ptr(b[f"gates{k}"]), ptr(b[f"hs{k}"]),
                 ptr(b[f"state{k}"]), ptr(hd), T, L, H, D, *self._drop_args(seed, k, drop), s)
            xin = hd if drop else b[f"hs{k}"]
        return b[f"hs{cfg.rnn_layer - 1}"]

    def stack_backward(self, dh, gp, seed, s):
        """dh bf16 [R][Hout]: the gradient of the last layer's output; gp(name): address of a parameter's gradient in the flat buffer"""
        st, cfg, b = self.st, self.cfg, self.bufs
        R, L, T, H, D, G, GB, Ho = self.R, self.L, self.T, cfg.H, cfg.D, cfg.G, cfg.GB, cfg.Hout
        elman = getattr(cfg, "elman", False)
        for k in range(cfg.rnn_layer - 1, -1, -1):
            kin, kp = cfg.layer_in(k)
            drop = self.dropping and k < cfg.rnn_layer - 1
            if elman:
                call("sehip_rsm_elman_bwd", self._wp(st.w[(k, "hhT")]), ptr(b[f"state{k}"]), ptr(dh), ptr(b[f"dG{k}"]), T, L, H, D, s)
            else:
                call("sehip_rsm_rnn_bwd", int(cfg.gru), ptr(b[f"gates{k}"]), self._wp(st.w[(k, "hhT")]), ptr(b[f"state{k}"]), ptr(dh), ptr(b[f"dG{k}"]),
                     ptr(b["carry"]), T, L, H, D, *self._drop_args(seed, k, drop), s)
            xin = b["feat"] if k == 0 else (b[f"hd{k - 1}"] if self.dropping else b[f"hs{k - 1}"])
            dG, hs = b[f"dG{k}"], b[f"hs{k}"]
            for d, sfx in enumerate(("", "_reverse")[:D]):
                a0 = dG.data_ptr() + 2 * d * GB * H
                call("sehip_rsm_gemm_tn", a0, D * GB * H, ptr(xin), kp, R, G * H, kin, 1, 0, gp(f"rnn.weight_ih_l{k}{sfx}"), kin, s)
                x0 = hs.data_ptr() + 2 * d * H
                ghh = gp(f"rnn.weight_hh_l{k}{sfx}")
                shift = 1 if d else -1
                if cfg.gru:       # r and z: blocks 0, 1; n: block 3 (the gradient of W_hn h carries the factor r)
                    call("sehip_rsm_gemm_tn", a0, D * 4 * H, x0, Ho, R, 2 * H, H, L, shift, ghh, H, s)
                    call("sehip_rsm_gemm_tn", a0 + 2 * 3 * H, D * 4 * H, x0, Ho, R, H, H, L, shift, ghh + 4 * 2 * H * H, H, s)
                else:
                    call("sehip_rsm_gemm_tn", a0, D * GB * H, x0, Ho, R, G * H, H, L, shift, ghh, H, s)
            if k > 0:
                call("sehip_rsm_gemm_nt", ptr(dG), D * GB * H, self._wp(st.w[(k, "ihT")]), D * GB * H, R, kin, D * GB * H, 1, None, ptr(b[f"dx{k}"]), kin, s)
                dh = b[f"dx{k}"]


class RnnMaskWorkspace(RnnStackWorkspace):
    """Buffers and launches for inputs [B, C, F, T, 2].  `guard` > 0 (tests): every buffer sits between two bands of that many
    canary elements inside its allocation."""

    def __init__(self, st: RnnMaskStatic, B, T, device, guard=0):
        super().__init__()
        cfg = st.cfg
        if B < 1 or T < 1:
            raise SehipError(f"RNNBaseSTFTMask: B={B}, T={T} must be positive")
        L = B * cfg.audio_channels
        if L * cfg.num_spk > 65535 or T * L >= 2 ** 31 // (4 * cfg.Hout) or (T * L + 255) // 256 > 65535:
            raise SehipError(f"RNNBaseSTFTMask: B C = {L} steps of T = {T} rows are more than the kernels' index ranges take")
        self.st, self.cfg, self.B, self.T, self.L, self.R, self.device = st, cfg, B, T, L, T * L, device
        self.guard, self._alloc = int(guard), {}
        self.bufs = {}
        for name, (shape, dt) in st.buffer_shapes(B, T).items():
            self.bufs[name] = self._make(name, shape, BF16 if dt == "bf16" else torch.float32)
        self.out = self.bufs["out"]
        self.wpack = self._make("wpack", (st.n_wpack,), BF16)
        C = cfg.Hout
        lib = _lib.lib()
        self.coef = self._make("coef", (C, 4), torch.float32)
        self.bcoef = self._make("bcoef", (C, 4), torch.float32)
        self.part = self._make("part", (int(lib.sehip_wun_bn_scratch_floats(self.R, C)),), torch.float32)
        self.bpart = self._make("bpart", (int(lib.sehip_rsm_sum_scratch_floats(self.R, max(C, cfg.SF))),), torch.float32)
        self.ctr_used = torch.zeros(2, dtype=torch.int32, device=device)
        self.x = None
        self.training, self.dropping = True, False

    def forward(self, x, params, buffers, nbt, seed, counter, training=True):
        """x [B, C, F, T, 2] fp32 on the device -> self.out [B, S, C, F, T, 2]"""
        st, cfg, b = self.st, self.cfg, self.bufs
        Lay = st.layout
        R, L, T, Ho = self.R, self.L, self.T, cfg.Hout
        s = stream()
        self.x, self.training = x, bool(training)
        self.dropping = self.training and cfg.drop_out > 0.0 and cfg.rnn_layer > 1
        for name, r0, n, k_, tr, ld, off in st.pack_launches():
            call("sehip_rsm_pack_w", self._pp(params, name) + 4 * r0, n, k_, tr, ld, self._wp(off), s)
        if self.dropping:
            call("sehip_rsm_counter_next", ptr(counter), ptr(self.ctr_used), s)
        call("sehip_rsm_features", ptr(x), L, cfg.F, T, cfg.Fp, ptr(b["feat"]), s)
        y = self.stack_forward(b["feat"], seed, s)
        pre = "batchnorm."
        if training:
            call("sehip_wun_bn_stats", ptr(y), R, Ho, ptr(self.part), s)
        call("sehip_wun_bn_finalize", ptr(self.part), ptr(y), self._pp(params, pre + "weight"), self._pp(params, pre + "bias"),
             buffers.data_ptr() + 4 * Lay.buffer_off[pre + "running_mean"][0], buffers.data_ptr() + 4 * Lay.buffer_off[pre + "running_var"][0],
             nbt.data_ptr() + 8 * Lay.nbt_idx[pre + "num_batches_tracked"], R, Ho, BN_EPS, BN_MOMENTUM, 1 if training else 0, ptr(self.coef), s)
        call("sehip_rsm_bn_apply", ptr(y), ptr(self.coef), R, Ho, ptr(b["z"]), s)
        call("sehip_rsm_gemm_nt", ptr(b["z"]), Ho, self._wp(st.w["fc"]), Ho, R, cfg.SF, Ho, 2, self._pp(params, "fc_layers.0.bias"),
             ptr(b["mask"]), cfg.SFp, s)
        call("sehip_rsm_mask_fwd", ptr(b["mask"]), ptr(x), self.B, cfg.audio_channels, cfg.num_spk, cfg.F, T, cfg.SFp, ptr(self.out), s)
        return self.out

    def backward(self, dout, params, grads, seed):
        """dout [B, S, C, F, T, 2] fp32 -> flat parameter gradients (overwritten)"""
        if not self.training:
            raise SehipError("RNNBaseSTFTMask.backward in eval mode: the backward pass is built for batch statistics only (call model.train())")
        st, cfg, b = self.st, self.cfg, self.bufs
        R, T, Ho = self.R, self.T, cfg.Hout
        s = stream()
        gp = lambda name: grads.data_ptr() + 4 * st.layout.param_off[name][0]
        call("sehip_zero_regions", ptr(grads), grads.numel() * 4, None, 0, None, 0, None, 0, s)
        call("sehip_rsm_mask_bwd", ptr(dout), ptr(self.x), ptr(b["mask"]), self.B, cfg.audio_channels, cfg.num_spk, cfg.F, T, cfg.SFp,
             ptr(b["dpre"]), s)
        call("sehip_rsm_gemm_tn", ptr(b["dpre"]), cfg.SFp, ptr(b["z"]), Ho, R, cfg.SF, Ho, 1, 0, gp("fc_layers.0.weight"), Ho, s)
        call("sehip_rsm_colsum", ptr(b["dpre"]), cfg.SFp, None, None, R, cfg.SF, ptr(self.bpart), s)
        call("sehip_rsm_colsum_finalize", ptr(self.bpart), R, cfg.SF, None, None, gp("fc_layers.0.bias"), None, None, s)
        call("sehip_rsm_gemm_nt", ptr(b["dpre"]), cfg.SFp, self._wp(st.w["fcT"]), cfg.SFp, R, Ho, cfg.SFp, 1, None, ptr(b["dz"]), Ho, s)
        y = b[f"hs{cfg.rnn_layer - 1}"]
        call("sehip_rsm_colsum", ptr(b["dz"]), Ho, ptr(y), ptr(self.coef), R, Ho, ptr(self.bpart), s)
        call("sehip_rsm_colsum_finalize", ptr(self.bpart), R, Ho, self._pp(params, "batchnorm.weight"), ptr(self.coef), gp("batchnorm.bias"),
             gp("batchnorm.weight"), ptr(self.bcoef), s)
        call("sehip_rsm_bn_bwd_apply", ptr(b["dz"]), ptr(y), ptr(self.coef), ptr(self.bcoef), R, Ho, ptr(b["dy"]), s)
        self.stack_backward(b["dy"], gp, seed, s)
        return grads
