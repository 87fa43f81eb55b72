"""CPU restatement of chunked DCCRN inference (sehip.model.DCCRNStreamer, csrc/dccrn_stream.hip) on the functions of
oracle/dccrn_oracle.py -- TEST INFRASTRUCTURE ONLY.

The network looks LA = 6 frames ahead (each of the six transposed convolutions reads frames t and t + 1) and the overlap-add needs
R - 1 more frames (R = win_len / win_inc), so a chunk of Kc hops fed at frame position `pos` yields

    analysis, encoder, LSTM    frames pos .. pos + Kc - 1                      (lag 0)
    decoder j                  frames pos - (j + 1) .. pos + Kc - 1 - (j + 1)   (lag j + 1; its mask, j = 5, lags LA = 6)
    output                     hop blocks pos - (LA + R - 1) ..                 (block q is the sum of frames q .. q + R - 1)

History rows in front of a chunk: one per encoder-layer input and decoder main input, j + 1 of skip 5 - j for decoder j (so skip i keeps
6 - i rows, the innermost one), LA spectrum rows.  A frame with index >= `end` is ABSENT: it enters every decoder product as a zero row
(main input and skip) and adds nothing to the overlap-add; frames and output blocks with a negative index contribute nothing either.
`sim` as in the oracle (NoSim / Bf16Sim: bf16 storage of activations and product weights)."""
import torch
import torch.nn.functional as F

from oracle import dccrn_oracle as O

LA = 6                      # frames of look-ahead: one per decoder layer
NO_END = 2 ** 31 - 1


def delay_of(win_len, win_inc):
    return (LA + win_len // win_inc - 1) * win_inc


def state_bytes_of(kernel_num, rnn_layers, rnn_units, win_len, win_inc, streams):
    """Closed form of DCCRNStreamer.state_bytes (kernel_num: the six widths)."""
    kn = [2] + list(kernel_num)
    pad, hid = win_len - win_inc, rnn_units // 2
    per = 2 * pad * 4                                        # input carry, both halves
    per += 2 * pad * 4                                       # overlap-add tail
    per += 2 * LA * 257 * 8                                  # spectrum ring
    per += 2 * 1 * 256 * 2 * 2                               # encoder input: one row
    for i in range(6):
        per += 2 * (1 if i == 5 else 6 - i) * (256 >> (i + 1)) * kn[i + 1] * 2      # encoder output i: max(1, 6 - i) rows
    per += 2 * 1 * 4 * kn[6] * 2                             # LSTM projection: one row
    for j in range(5):
        per += 2 * 1 * (256 >> (5 - j)) * kn[5 - j] * 2      # decoder output j: one row
    per += rnn_layers * 4 * hid * (2 + 4)                    # h (bf16) and c (fp32) of the four recurrences of a layer
    per += 8                                                 # pos, end
    return streams * per + 4                                 # + the phase word


def _lstm_steps(x, w_ih, w_hh, b_ih, b_hh, h, c, sim):
    """O.lstm_single from a carried state: x [K,S,I] -> ([K,S,H], h, c)"""
    w_ih, w_hh = sim.weight(w_ih), sim.weight(w_hh)
    pre = x @ w_ih.t() + (b_ih + b_hh)
    outs = []
    for t in range(x.shape[0]):
        gates = pre[t] + h @ w_hh.t()
        i, f, g, o = gates.chunk(4, 1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = sim.act(torch.sigmoid(o) * torch.tanh(c))
        outs.append(h)
    return torch.stack(outs, 0), h, c


class StreamRef:
    def __init__(self, p, cfg, streams, chunk_frames, sim=O.NoSim):
        assert cfg.win_len % cfg.win_inc == 0 and cfg.use_clstm
        self.p, self.cfg, self.S, self.Kc, self.sim = p, cfg, streams, chunk_frames, sim
        self.dt = p["encoder.0.0.real_conv.weight"].dtype
        self.hop, self.win, self.R = cfg.win_inc, cfg.win_len, cfg.win_len // cfg.win_inc
        self.pad = self.win - self.hop
        self.delay = delay_of(self.win, self.hop)
        an, sy, w = O.stft_bases(cfg.win_len, cfg.fft_len, getattr(cfg, "win_type", "hann"))
        if self.dt == torch.float64:          # (the bases at full precision: the offline oracle is given the same ones)
            an, sy, w = bases64(cfg)
        self.analysis, self.synthesis, self.window = an, sy, w
        w2 = self.window.to(self.dt) ** 2
        self.coff = sum(w2[r * self.hop:(r + 1) * self.hop] for r in range(self.R - 1, -1, -1)) + 1e-8     # periodic in the hop
        kn = cfg.kernel_num
        self.hid = cfg.rnn_units // 2
        self.skip_rows = [1 if i == 5 else 6 - i for i in range(6)]
        self.state_bytes = state_bytes_of(kn[1:], cfg.rnn_layers, cfg.rnn_units, self.win, self.hop, streams)
        self.reset()

    def bases(self):
        return self.analysis, self.synthesis, self.window

    def reset(self, which=None):
        S, kn, z = self.S, self.cfg.kernel_num, lambda *s: torch.zeros(*s, dtype=self.dt)
        if which is None:
            self.pos = [0] * S
            self.end = [NO_END] * S
            self.carry, self.tail = z(S, self.pad), z(S, self.pad)
            self.ring = z(S, 2, 257, LA)
            self.h_in = z(S, 2, 256, 1)
            self.h_z = [z(S, kn[i + 1], 256 >> (i + 1), self.skip_rows[i]) for i in range(6)]
            self.h_p = z(S, kn[6], 4, 1)
            self.h_zd = [z(S, kn[5 - j], 256 >> (5 - j), 1) for j in range(5)]
            self.lstm = [[(z(S, self.hid), z(S, self.hid)) for _ in range(4)] for _ in range(self.cfg.rnn_layers)]
            return
        idx = torch.as_tensor(which)
        idx = idx.nonzero().reshape(-1).tolist() if idx.dtype == torch.bool else idx.reshape(-1).tolist()
        for s in idx:
            self.pos[s], self.end[s] = 0, NO_END
            for t in [self.carry, self.tail, self.ring, self.h_in, self.h_p] + self.h_z + self.h_zd:
                t[s] = 0
            for layer in self.lstm:
                for h, c in layer:
                    h[s] = 0
                    c[s] = 0

    def _absent(self, x, lag):
        """zero the frames (last axis, the chunk's Kc) whose index pos + k - lag is >= end"""
        x = x.clone()
        for s in range(self.S):
            for k in range(self.Kc):
                if self.pos[s] + k - lag >= self.end[s]:
                    x[s, ..., k] = 0
        return x

    def _bn(self, x, pre):
        bn = O.complex_batchnorm if self.cfg.use_cbn else O.real_batchnorm
        return self.sim.act(F.prelu(bn(x, self.p, pre + "1.", False), self.p[pre + "2.weight"]))

    def feed(self, x):
        """x [S,1,Kc*hop] -> [S,1,Kc*hop]"""
        p, cfg, sim, S, Kc, hop, win = self.p, self.cfg, self.sim, self.S, self.Kc, self.hop, self.win
        assert tuple(x.shape) == (S, 1, Kc * hop)
        sig = torch.cat([self.carry, x[:, 0].to(self.dt)], 1)
        self.carry = sig[:, -self.pad:].clone() if self.pad else self.carry
        spec = F.conv1d(sig[:, None], self.analysis.to(self.dt)[:, None, :], stride=hop)           # [S, 514, Kc]
        spec = torch.stack([spec[:, :257], spec[:, 257:]], 1)                                        # [S, 2, 257, Kc]
        specs = torch.cat([self.ring, spec], -1)                                                     # frames pos - 6 ..
        self.ring = specs[..., -LA:].clone()
        cur = torch.cat([self.h_in, sim.act(spec[:, :, 1:])], -1)
        self.h_in = cur[..., -1:].clone()
        skips = []
        for i in range(6):
            pre = f"encoder.{i}."
            y = O.complex_conv2d(cur[..., -(Kc + 1):], sim.weight(p[pre + "0.real_conv.weight"]), p[pre + "0.real_conv.bias"],
                                 sim.weight(p[pre + "0.imag_conv.weight"]), p[pre + "0.imag_conv.bias"], time_pad=0)
            zc = self._absent(self._bn(sim.act(y), pre), 0)
            cur = torch.cat([self.h_z[i], zc], -1)
            self.h_z[i] = cur[..., -self.skip_rows[i]:].clone()
            skips.append(cur)
        zc = cur[..., -Kc:]
        ch, d = zc.shape[1], zc.shape[2]
        seq = zc.permute(3, 0, 1, 2)
        r_in, i_in = seq[:, :, :ch // 2].reshape(Kc, S, -1), seq[:, :, ch // 2:].reshape(Kc, S, -1)
        for layer in range(cfg.rnn_layers):
            q = f"enhance.{layer}."
            st, outs = self.lstm[layer], []
            for combo, (xin, which) in enumerate(((r_in, "real_lstm"), (r_in, "imag_lstm"), (i_in, "real_lstm"), (i_in, "imag_lstm"))):
                w = q + which + "."
                o, h, c = _lstm_steps(xin, p[w + "weight_ih_l0"], p[w + "weight_hh_l0"], p[w + "bias_ih_l0"], p[w + "bias_hh_l0"],
                                      st[combo][0], st[combo][1], sim)
                st[combo] = (h, c)
                outs.append(o)
            r_in, i_in = outs[0] - outs[3], outs[2] + outs[1]
            if layer == cfg.rnn_layers - 1:
                r_in = sim.act(F.linear(r_in, sim.weight(p[q + "r_trans.weight"]), p[q + "r_trans.bias"]))
                i_in = sim.act(F.linear(i_in, sim.weight(p[q + "i_trans.weight"]), p[q + "i_trans.bias"]))
        pc = torch.cat([r_in.reshape(Kc, S, ch // 2, d), i_in.reshape(Kc, S, ch // 2, d)], 2).permute(1, 2, 3, 0)
        main = torch.cat([self.h_p, self._absent(pc, 0)], -1)                 # frames pos - 1 .. pos + Kc - 1
        self.h_p = main[..., -1:].clone()
        for j in range(6):
            pre = f"decoder.{j}."
            sk = skips[5 - j][..., -(Kc + j + 1):][..., :Kc + 1]              # frames pos - (j + 1) .. pos + Kc - (j + 1)
            y = O.complex_deconv2d(O.complex_cat(main, sk), sim.weight(p[pre + "0.real_conv.weight"]), p[pre + "0.real_conv.bias"],
                                   sim.weight(p[pre + "0.imag_conv.weight"]), p[pre + "0.imag_conv.bias"])[..., 1:Kc + 1]
            if j == 5:
                mask = y                                                       # frames pos - 6 .. pos + Kc - 7
                break
            zc = self._absent(self._bn(sim.act(y), pre), j + 1)
            main = torch.cat([self.h_zd[j], zc], -1)
            self.h_zd[j] = main[..., -1:].clone()
        m_r, m_i = F.pad(mask[:, 0], [0, 0, 1, 0]), F.pad(mask[:, 1], [0, 0, 1, 0])
        real, imag = specs[:, 0, :, :Kc], specs[:, 1, :, :Kc]
        if cfg.masking_mode == "E":
            mags, phase = torch.sqrt(real ** 2 + imag ** 2 + 1e-8), torch.atan2(imag, real)
            m_mag = (m_r ** 2 + m_i ** 2) ** 0.5
            m_phase = torch.atan2(m_i / (m_mag + 1e-8), m_r / (m_mag + 1e-8))
            est_mag, est_phase = torch.tanh(m_mag) * mags, phase + m_phase
            real, imag = est_mag * torch.cos(est_phase), est_mag * torch.sin(est_phase)
        elif cfg.masking_mode == "C":
            real, imag = real * m_r - imag * m_i, real * m_i + imag * m_r
        else:
            real, imag = real * m_r, imag * m_i
        frames = torch.einsum("sck,cn->skn", torch.cat([real, imag], 1), self.synthesis.to(self.dt))     # [S, Kc, win]
        # overlap-add: position j counts from the first sample of hop block q0 = pos - LA - (R - 1); every sample is the carried tail plus
        # the chunk's frames in ascending order
        acc = torch.cat([self.tail, torch.zeros(S, Kc * hop, dtype=self.dt)], 1)
        for s in range(S):
            for k in range(Kc):
                f = self.pos[s] - LA + k
                if 0 <= f < self.end[s]:
                    acc[s, k * hop:k * hop + win] += frames[s, k]
        out = acc[:, :Kc * hop] / self.coff.repeat(Kc)
        for s in range(S):
            for k in range(Kc):
                if self.pos[s] - LA - (self.R - 1) + k < 0:
                    out[s, k * hop:(k + 1) * hop] = 0
        self.tail = acc[:, Kc * hop:].clone()
        self.pos = [q + Kc for q in self.pos]
        return torch.clamp(out, -1, 1)[:, None]

    def flush(self):
        """[S,1,D]: R - 1 hops of zeros are the reference's right pad, then LA hops with every frame >= end absent; resets."""
        self.end = [q + self.R - 1 for q in self.pos]
        hops, outs = LA + self.R - 1, []
        for _ in range(-(-hops // self.Kc)):
            outs.append(self.feed(torch.zeros(self.S, 1, self.Kc * self.hop, dtype=self.dt)))
        self.reset()
        return torch.cat(outs, -1)[..., :self.delay]


def bases64(cfg):
    """stft_bases in float64 (the oracle's are rounded to fp32)"""
    import numpy as np
    n = np.arange(cfg.win_len, dtype=np.float64)[None, :]
    k = np.arange(cfg.fft_len // 2 + 1, dtype=np.float64)[:, None]
    ang = 2.0 * np.pi * k * n / cfg.fft_len
    basis = np.concatenate([np.cos(ang), -np.sin(ang)], axis=0)
    win = O.window_of(getattr(cfg, "win_type", "hann"), cfg.win_len)
    return torch.from_numpy(basis * win[None, :]), torch.from_numpy(np.linalg.pinv(basis).T * win[None, :]), torch.from_numpy(win)


def run_stream(ref, x, flush=True):
    """feeds x [S,1,N] chunk by chunk -> (cat of the outputs, flush tail or None)"""
    n = ref.Kc * ref.hop
    assert x.shape[-1] % n == 0
    outs = [ref.feed(x[..., j * n:(j + 1) * n]) for j in range(x.shape[-1] // n)]
    return torch.cat(outs, -1), (ref.flush() if flush else None)


def make_params(cfg, seed=3, dtype=torch.float32):
    """oracle parameters with non-trivial biases, affine terms and RUNNING STATISTICS (eval-mode BatchNorm is what streams)"""
    p = O.perturb_params(O.init_params(cfg, seed=seed), seed=seed + 1)
    g = torch.Generator().manual_seed(seed + 2)
    for k in list(p):
        if k.endswith((".RMr", ".RMi", ".running_mean")):
            p[k] = 0.1 * torch.randn(p[k].shape, generator=g)
        elif k.endswith((".RVrr", ".RVii", ".running_var")):
            p[k] = 0.5 + torch.rand(p[k].shape, generator=g)
        elif k.endswith(".RVri"):
            p[k] = 0.2 * (torch.rand(p[k].shape, generator=g) - 0.5)
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in p.items()}
