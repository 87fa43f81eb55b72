"""Host-side plan of the mel-rnn train step on libsehip (reference: src/model/mel_rnn.py:8-123; `mel-rnn` of the registry), at n_mels = 0.

At n_mels = 0 the model is rnn-stft-mask's sibling (sehip/plan_rnnmask.py) with one channel, one speaker, no dropout, one direction and
another head:
  * the features are ``|re^2 - im^2|`` (Amplitude, :116-123), not a magnitude;
  * nn.RNN / nn.LSTM / nn.GRU run with batch_first=False on ``[B][T][F]``: the recurrence walks the L = B axis, the T frames are its
    independent rows, and an utterance's output depends on its batch;
  * BatchNorm1d over all T L positions, then Linear + ReLU + Linear + Sigmoid, the mask times the complex input.
n_mels > 0 (the constructor's default 128) is refused: it goes through torchaudio's MelScale / InverseMelScale(max_iter=0), and the
inverse at zero iterations is its random starting point (later releases do not take the argument): there is nothing to pin a kernel to.

Layouts as in the sibling: bf16 ``[T][L][channels]`` (row r = t L + l), F padded to Fp = pad8(F) by zeros.  The recurrent stack is the
sibling's own loop (RnnStackWorkspace); the Elman cell ('rnn', tanh, no bias) runs on sehip_rsm_elman_fwd / _bwd: one block of H per
direction in the pre-activations and in dG, no gates buffer, no carried scratch.

Launch list of the head.  Forward: fc_layers.0 with bias + ReLU (sehip_rsm_gemm_nt, epilogue 2) -> a1 [R][Fp]; fc_layers.2 with bias +
sigmoid (sehip_rsm_gemm_nt_head, epilogue 3) -> mask [R][Fp]; sehip_rsm_mask_fwd with S = 1, Cn = 1.  Backward: sehip_rsm_mask_bwd_sigmoid
-> dpre2; weight and bias gradient of fc_layers.2 (sehip_rsm_gemm_tn, sehip_rsm_colsum); the input gradient through the ReLU
(sehip_rsm_gemm_nt_head, epilogue 4, gated by a1) -> dpre1; weight and bias gradient of fc_layers.0; the plain input gradient -> dz.
Weight gradients land in the flat gradient buffer in the parameters' own layout.
"""
import torch

from . import _lib
from ._lib import call, ptr, stream, SehipError
from .gemmdesc import ParamLayout, BF16
from .plan_rnnmask import (BN_EPS, BN_MOMENTUM, RnnStackWorkspace, pad8, stack_arena, stack_buffer_shapes, stack_pack_launches)


class MelRnnConfig:
    """Constructor arguments of the reference model (src/model/mel_rnn.py:9-20) and what of them is built."""

    def __init__(self, n_fft=512, hop_length=256, n_mels=128, f_min=100, f_max=8000, sample_rate=16000, rnn_hidden=256, rnn_layer=2,
                 rnn_type="rnn", **_ignored):
        def bad(arg, val, why):
            raise SehipError(f"sehip MelRNN: {arg}={val!r} {why}")
        if n_mels:
            bad("n_mels", n_mels, "(a mel front end; 128 is the constructor's default) has no HIP path yet: it runs through torchaudio's MelScale and "
                "InverseMelScale(max_iter=0), whose inverse at zero iterations is its random starting point, so there is nothing to check a "
                "kernel against; n_mels=0 (the shipped configuration) is built")
        if rnn_type not in ("rnn", "lstm", "gru"):
            bad("rnn_type", rnn_type, "must be 'rnn', 'lstm' or 'gru'")
        if not isinstance(rnn_layer, int) or isinstance(rnn_layer, bool) or not 1 <= rnn_layer <= 8:
            bad("rnn_layer", rnn_layer, "must be an integer in 1 .. 8")
        if not isinstance(rnn_hidden, int) or isinstance(rnn_hidden, bool) or rnn_hidden < 32 or rnn_hidden > 1024 or rnn_hidden % 32:
            bad("rnn_hidden", rnn_hidden, "must be a multiple of 32 in 32 .. 1024 (one MFMA covers 32 hidden units of K)")
        if not isinstance(n_fft, int) or isinstance(n_fft, bool) or n_fft < 2 or n_fft > 4096 or n_fft % 2:
            bad("n_fft", n_fft, "must be an even integer in 2 .. 4096")
        self.n_fft, self.hop_length, self.n_mels, self.f_min, self.f_max, self.sample_rate = n_fft, hop_length, 0, f_min, f_max, sample_rate
        self.rnn_hidden, self.rnn_layer, self.rnn_type = rnn_hidden, rnn_layer, rnn_type
        self.elman, self.gru = rnn_type == "rnn", rnn_type == "gru"
        self.G = {"rnn": 1, "lstm": 4, "gru": 3}[rnn_type]
        self.GB = 1 if self.elman else 4
        self.D, self.H, self.Hout = 1, rnn_hidden, rnn_hidden
        self.has_dropout, self.drop_out = False, 0.0
        self.num_spk = self.audio_channels = 1
        self.F = n_fft // 2 + 1
        self.Fp = pad8(self.F)
        self.SF, self.SFp = self.F, self.Fp

    def key(self):
        return (self.rnn_type, self.rnn_layer, self.H, self.n_fft)

    def layer_in(self, k):
        """(input width, its padded width) of RNN layer k"""
        return (self.F, self.Fp) if k == 0 else (self.H, self.H)

    def param_specs(self):
        """[(name, shape, kind)] in the reference's state_dict() order"""
        out = []
        for k in range(self.rnn_layer):
            out.append((f"rnn.weight_ih_l{k}", (self.G * self.H, self.layer_in(k)[0]), "param"))
            out.append((f"rnn.weight_hh_l{k}", (self.G * self.H, self.H), "param"))
        c, f = self.H, self.F
        out += [("batchnorm.weight", (c,), "param"), ("batchnorm.bias", (c,), "param"), ("batchnorm.running_mean", (c,), "buffer"),
                ("batchnorm.running_var", (c,), "buffer"), ("batchnorm.num_batches_tracked", (), "nbt"),
                ("fc_layers.0.weight", (f, c), "param"), ("fc_layers.0.bias", (f,), "param"),
                ("fc_layers.2.weight", (f, f), "param"), ("fc_layers.2.bias", (f,), "param")]
        return out


class MelRnnStatic:
    """Parameter layout and the bf16 weight arena (independent of the batch)."""

    def __init__(self, cfg: MelRnnConfig):
        self.cfg = cfg
        self.layout = ParamLayout(cfg)
        self.w = {}                # (layer, what) -> element offset in the bf16 arena
        off = stack_arena(cfg, self.w, 0)
        for what, n in (("fc0", cfg.F * cfg.H),              # [F][H]     fc_layers.0
                        ("fc0T", cfg.H * cfg.Fp),            # [H][Fp]    its input gradient
                        ("fc2", cfg.F * cfg.Fp),             # [F][Fp]    fc_layers.2
                        ("fc2T", cfg.F * cfg.Fp)):           # [F][Fp]    transposed: its input gradient
            self.w[what] = off
            off += n
        self.n_wpack = off

    def pack_launches(self):
        """[(parameter name, row offset in it, N, K, transpose, ld, arena offset)]: the sehip_rsm_pack_w calls of one step"""
        cfg = self.cfg
        out = stack_pack_launches(cfg, self.w)
        out.append(("fc_layers.0.weight", 0, cfg.F, cfg.H, 0, cfg.H, self.w["fc0"]))
        out.append(("fc_layers.0.weight", 0, cfg.F, cfg.H, 1, cfg.Fp, self.w["fc0T"]))
        out.append(("fc_layers.2.weight", 0, cfg.F, cfg.F, 0, cfg.Fp, self.w["fc2"]))
        out.append(("fc_layers.2.weight", 0, cfg.F, cfg.F, 1, cfg.Fp, self.w["fc2T"]))
        return out

    def step_launches(self, L):
        """kernel launches of one training step's recurrence: (forward, backward) step launches over all layers"""
        return self.cfg.rnn_layer * L, self.cfg.rnn_layer * L

    def buffer_shapes(self, B, T):
        """name -> (shape, dtype name) of every per-batch buffer of a workspace for inputs [B, 1, F, T, 2]"""
        cfg = self.cfg
        R, H, Fp = T * B, cfg.H, cfg.Fp
        s = {"feat": ((R, Fp), "bf16"), "z": ((R, H), "bf16"), "dz": ((R, H), "bf16"), "dy": ((R, H), "bf16"), "a1": ((R, Fp), "bf16"),
             "mask": ((R, Fp), "bf16"), "dpre2": ((R, Fp), "bf16"), "dpre1": ((R, Fp), "bf16"), "out": ((B, 1, 1, cfg.F, T, 2), "f32")}
        return stack_buffer_shapes(cfg, R, T, s)


class MelRnnWorkspace(RnnStackWorkspace):
    """Buffers and launches for inputs [B, 1, F, T, 2].  `guard` > 0 (tests): every buffer sits between two bands of that many canary
    elements inside its allocation."""

    def __init__(self, st: MelRnnStatic, B, T, device, guard=0):
        super().__init__()
        cfg = st.cfg
        if B < 1 or T < 1:
            raise SehipError(f"MelRNN: B={B}, T={T} must be positive")
        if B > 65535 or T * B >= 2 ** 31 // (4 * cfg.H) or (T * B + 255) // 256 > 65535:
            raise SehipError(f"MelRNN: B = {B} steps of T = {T} rows are more than the kernels' index ranges take")
        self.st, self.cfg, self.B, self.T, self.L, self.R, self.device = st, cfg, B, T, B, T * B, device
        self.guard, self._alloc = int(guard), {}
        self.bufs = {}
        for name, (shape, dt) in st.buffer_shapes(B, T).items():
            self.bufs[name] = self._make(name, shape, BF16 if dt == "bf16" else torch.float32)
        self.out6 = self.bufs["out"]
        self.out = self.out6.view(B, 1, cfg.F, T, 2)
        self.wpack = self._make("wpack", (st.n_wpack,), BF16)
        lib = _lib.lib()
        self.coef = self._make("coef", (cfg.H, 4), torch.float32)
        self.bcoef = self._make("bcoef", (cfg.H, 4), torch.float32)
        self.part = self._make("part", (int(lib.sehip_wun_bn_scratch_floats(self.R, cfg.H)),), torch.float32)
        self.bpart = self._make("bpart", (int(lib.sehip_rsm_sum_scratch_floats(self.R, max(cfg.H, cfg.F))),), torch.float32)
        self.ctr_used = None         # no dropout in this model: the step kernels take a null counter
        self.x = None
        self.training, self.dropping = True, False

    def forward(self, x, params, buffers, nbt, training=True):
        """x [B, 1, F, T, 2] fp32 on the device -> self.out [B, 1, F, T, 2]"""
        st, cfg, b = self.st, self.cfg, self.bufs
        Lay = st.layout
        R, L, T, H, F, Fp = self.R, self.L, self.T, cfg.H, cfg.F, cfg.Fp
        s = stream()
        self.x, self.training = x, bool(training)
        for name, r0, n, k_, tr, ld, off in st.pack_launches():
            call("sehip_rsm_pack_w", self._pp(params, name) + 4 * r0, n, k_, tr, ld, self._wp(off), s)
        call("sehip_rsm_features", ptr(x), L, F, T, Fp, ptr(b["feat"]), s)
        y = self.stack_forward(b["feat"], 0, s)
        pre = "batchnorm."
        if training:
            call("sehip_wun_bn_stats", ptr(y), R, H, ptr(self.part), s)
        call("sehip_wun_bn_finalize", ptr(self.part), ptr(y), self._pp(params, pre + "weight"), self._pp(params, pre + "bias"),
             buffers.data_ptr() + 4 * Lay.buffer_off[pre + "running_mean"][0], buffers.data_ptr() + 4 * Lay.buffer_off[pre + "running_var"][0],
             nbt.data_ptr() + 8 * Lay.nbt_idx[pre + "num_batches_tracked"], R, H, BN_EPS, BN_MOMENTUM, 1 if training else 0, ptr(self.coef), s)
        call("sehip_rsm_bn_apply", ptr(y), ptr(self.coef), R, H, ptr(b["z"]), s)
        call("sehip_rsm_gemm_nt", ptr(b["z"]), H, self._wp(st.w["fc0"]), H, R, F, H, 2, self._pp(params, "fc_layers.0.bias"), ptr(b["a1"]), Fp, s)
        call("sehip_rsm_gemm_nt_head", ptr(b["a1"]), Fp, self._wp(st.w["fc2"]), Fp, R, F, Fp, 3, self._pp(params, "fc_layers.2.bias"), None, 0,
             ptr(b["mask"]), Fp, s)
        call("sehip_rsm_mask_fwd", ptr(b["mask"]), ptr(x), self.B, 1, 1, F, T, Fp, ptr(self.out6), s)
        return self.out

    def backward(self, dout, params, grads):
        """dout [B, 1, F, T, 2] fp32 -> flat parameter gradients (overwritten)"""
        if not self.training:
            raise SehipError("MelRNN.backward in eval mode: the backward pass is built for batch statistics only (call model.train())")
        st, cfg, b = self.st, self.cfg, self.bufs
        R, T, H, F, Fp = self.R, self.T, cfg.H, cfg.F, cfg.Fp
        s = stream()
        gp = lambda name: grads.data_ptr() + 4 * st.layout.param_off[name][0]
        call("sehip_zero_regions", ptr(grads), grads.numel() * 4, None, 0, None, 0, None, 0, s)
        call("sehip_rsm_mask_bwd_sigmoid", ptr(dout), ptr(self.x), ptr(b["mask"]), self.B, 1, 1, F, T, Fp, ptr(b["dpre2"]), s)
        call("sehip_rsm_gemm_tn", ptr(b["dpre2"]), Fp, ptr(b["a1"]), Fp, R, F, F, 1, 0, gp("fc_layers.2.weight"), F, s)
        call("sehip_rsm_colsum", ptr(b["dpre2"]), Fp, None, None, R, F, ptr(self.bpart), s)
        call("sehip_rsm_colsum_finalize", ptr(self.bpart), R, F, None, None, gp("fc_layers.2.bias"), None, None, s)
        call("sehip_rsm_gemm_nt_head", ptr(b["dpre2"]), Fp, self._wp(st.w["fc2T"]), Fp, R, F, Fp, 4, None, ptr(b["a1"]), Fp, ptr(b["dpre1"]), Fp, s)
        call("sehip_rsm_gemm_tn", ptr(b["dpre1"]), Fp, ptr(b["z"]), H, R, F, H, 1, 0, gp("fc_layers.0.weight"), H, s)
        call("sehip_rsm_colsum", ptr(b["dpre1"]), Fp, None, None, R, F, ptr(self.bpart), s)
        call("sehip_rsm_colsum_finalize", ptr(self.bpart), R, F, None, None, gp("fc_layers.0.bias"), None, None, s)
        call("sehip_rsm_gemm_nt", ptr(b["dpre1"]), Fp, self._wp(st.w["fc0T"]), Fp, R, H, Fp, 1, None, ptr(b["dz"]), H, s)
        y = b[f"hs{cfg.rnn_layer - 1}"]
        call("sehip_rsm_colsum", ptr(b["dz"]), H, ptr(y), ptr(self.coef), R, H, ptr(self.bpart), s)
        call("sehip_rsm_colsum_finalize", ptr(self.bpart), R, H, self._pp(params, "batchnorm.weight"), ptr(self.coef), gp("batchnorm.bias"),
             gp("batchnorm.weight"), ptr(self.bcoef), s)
        call("sehip_rsm_bn_bwd_apply", ptr(b["dz"]), ptr(y), ptr(self.coef), ptr(self.bcoef), R, H, ptr(b["dy"]), s)
        self.stack_backward(b["dy"], gp, 0, s)
        return grads
