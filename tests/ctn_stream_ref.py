"""float64 / fp32 restatement of the CHUNKED ConvTasNet(causal=True, norm_type='cLN') -- TEST INFRASTRUCTURE ONLY: what
sehip.model.ConvTasNetStreamer computes, in plain torch in the dtype of the parameters it is given.

Per stream: h carried input samples per audio channel, per block the last (P - 1) 2^x frames of n1 = cLN(PReLU(h1)) (the HIP path
keeps h1 and recomputes; a frame's n1 depends on that frame alone), the second half of the last decoded frame, and pos, the global
index of the coming call's first frame (-1 on a fresh stream).  The first frame of a fresh stream is a phantom built from the zero
carry: it is computed like any other, but a depthwise tap with a negative global index is ABSENT (zero, not cLN(PReLU(0)) = beta) and
the decoder adds nothing for a frame with a negative index.  Pinned against ctn_variants_ref.variants_forward by
tests/test_ctn_stream_host.py."""
import torch
import torch.nn.functional as F

from oracle import convtasnet_oracle as CT
from ctn_variants_ref import inner_keys


class StreamRef:
    def __init__(self, p, streams, chunk_frames, C=2, N=128, L=40, B=128, H=256, P=3, X=7, R=2, audio_channels=1, mask_nonlinear="relu"):
        self.p, self.S, self.Kc = p, streams, chunk_frames
        self.C, self.N, self.L, self.H, self.P, self.X, self.R, self.ac = C, N, L, H, P, X, R, audio_channels
        self.mask_nonlinear = mask_nonlinear
        self.h = L // 2
        self.dtype = p["encoder.conv1d_U.weight"].dtype
        z = lambda *s: torch.zeros(*s, dtype=self.dtype)
        self.carry = z(streams, audio_channels, self.h)
        self.hist = {(r, x): z(streams, H, (P - 1) * 2 ** x) for r in range(R) for x in range(X)}
        self.tail = z(streams, C, audio_channels, self.h)
        self.pos = torch.full((streams,), -1, dtype=torch.int64)

    @property
    def state_bytes(self):
        """what the HIP streamer holds: both halves of carry (fp32), history (bf16 rows of h1) and tail (fp32), pos, the phase word"""
        rows = sum(v.shape[-1] for v in self.hist.values())
        return self.S * (2 * (self.ac * self.h * 4 + rows * self.H * 2 + self.C * self.ac * self.h * 4) + 4) + 4

    def reset(self, which=None):
        idx = slice(None) if which is None else torch.as_tensor(which)
        self.pos[idx] = -1
        self.carry[idx] = 0
        self.tail[idx] = 0
        for v in self.hist.values():      # (the HIP path leaves its rows: their indices are negative after the reset, so they are absent)
            v[idx] = 0

    def feed(self, x):
        p, S, Kc, h = self.p, self.S, self.Kc, self.h
        assert tuple(x.shape) == (S, self.ac, Kc * h)
        x = x.to(self.dtype)
        cat = torch.cat([self.carry, x], dim=-1)
        self.carry = x[..., -h:].clone()
        w = F.relu(F.conv1d(cat, p["encoder.conv1d_U.weight"], stride=h))                    # [S, N, Kc]
        assert w.shape[-1] == Kc
        valid = ((self.pos[:, None] + torch.arange(Kc)[None, :]) >= 0).to(self.dtype)       # [S, Kc]: frames with index >= 0
        net = "separator.network."
        y = F.conv1d(CT.cln(w, p[net + "0.gamma"], p[net + "0.beta"]), p[net + "1.weight"])
        for r in range(self.R):
            for i in range(self.X):
                q = f"{net}2.{r}.{i}.net."
                a2, g2, b2 = inner_keys(q, True)
                h1 = F.conv1d(y, p[q + "0.weight"])
                n1 = CT.cln(F.prelu(h1, p[q + "1.weight"]), p[q + "2.gamma"], p[q + "2.beta"]) * valid[:, None, :]
                full = torch.cat([self.hist[(r, i)], n1], dim=-1)                             # [S, H, (P - 1) d + Kc]
                self.hist[(r, i)] = full[..., Kc:].clone()
                h2 = F.conv1d(full, p[q + "3.net.0.weight"], dilation=2 ** i, groups=self.H)
                u = CT.cln(F.prelu(h2, p[a2]), p[g2], p[b2])
                y = F.conv1d(u, p[q + "3.pointwise_conv.weight"]) + y
        score = F.conv1d(y, p[net + "3.weight"]).view(S, self.C, self.N, Kc)
        mask = F.relu(score) if self.mask_nonlinear == "relu" else F.softmax(score, dim=1)
        fr = F.linear((w.unsqueeze(1) * mask).transpose(2, 3), p["decoder.basis_signals.weight"])      # [S, C, Kc, ac * L]
        fr = fr.view(S, self.C, Kc, self.ac, self.L) * valid[:, None, :, None, None]
        lower, upper = fr[..., :h], fr[..., h:]                                                        # [S, C, Kc, ac, h]
        prev = torch.cat([self.tail.unsqueeze(2), upper[:, :, :-1]], dim=2)
        out = (prev + lower).permute(0, 1, 3, 2, 4).reshape(S, self.C, self.ac, Kc * h)
        self.tail = upper[:, :, -1].clone()
        self.pos += Kc
        return out

    def flush(self):
        t = self.tail.clone()
        self.reset()
        return t


def run_stream(make, mix, Kc, h):
    """feeds mix [S, ac, T] (T a multiple of h) in chunks of Kc frames as far as whole chunks go -> (outputs concatenated, flush)"""
    st = make(Kc)
    n = mix.shape[-1] // (Kc * h)
    outs = [st.feed(mix[..., j * Kc * h:(j + 1) * Kc * h]) for j in range(n)]
    return torch.cat(outs, dim=-1), st.flush()
