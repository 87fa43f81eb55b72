"""Float64 numpy restatement of the chunked hearing-aid stage (csrc/ha_stream.hip, sehip.ha.AmplifyStreamer), written for this project.

It keeps what the device keeps and nothing else: per row a position, a ring of the last K - 1 input samples and a ring of the last
W - 1 filtered samples (each one chunk longer than its history, sample a at slot a mod length; the rings start as NaN: a sample before
position 0 must read as zero by its INDEX, not by what the ring holds) and the gain c.  The window sums are formed afresh in every chunk
from the stored samples, as sums of non-negative terms only -- per segment of len = min(seg, W, rest) samples a suffix sum of the
outgoing samples, one sum of the untouched middle and a prefix sum of the incoming ones; there is no running sum.

    AmplifyStreamRef(taps [R, K], cfg, chunk, soft_clip=True, seg=1024)      cfg: ha_ref.compressor_config(...), cfg["W"] the window
      .feed(x [R, n])     -> dict(fir, level, gain, gain32, prod, out), each [R, n] float64 (the keys of ha_ref.chain)
      .flush()            -> the same for the K - 1 samples after the last one; then every row is fresh
      .reset(rows=None)   -> rows start afresh (position 0, c = 1); the rings are NOT cleared
    comp_signal(W, n, fs)  the 4-row compressor input of tests/test_gpu_ha_stream.py's cases
"""
import numpy as np

import ha_ref as R

#              W    n_total  chunk       (tests/test_gpu_ha_stream.py: compressor against float64, fs 16 000, ha_ref.CHAIN's settings)
COMP_CASES = ((1, 700, 7), (2, 700, 1), (50, 3000, 49), (64, 3000, 64), (64, 3000, 257), (1500, 6000, 64), (1024, 300, 17))
LONG_CASE = (50, 6400, 16)                                        # 400 chunks
COMP_FS = 16000


def comp_signal(W, n, fs=COMP_FS):
    """4 rows of randn * 1.2 * (0.5 + 0.5 sin(2 pi (3 + r) t + r))^2 from torch.Generator().manual_seed(9000 + W + n), fp32"""
    import torch
    g = torch.Generator().manual_seed(9000 + W + n)
    t = torch.arange(n, dtype=torch.float64) / fs
    return torch.stack([(torch.randn(n, generator=g).double() * 1.2 * (0.5 + 0.5 * torch.sin(2 * np.pi * (3 + r) * t + r)) ** 2).float()
                        for r in range(4)])


def comp_cfg(W, fs=COMP_FS):
    cfg = R.compressor_config(fs, **R.CHAIN["compressor"])
    cfg["W"] = W
    return cfg


def input_checks(level, threshold):
    """(margin, crossings, share above) of a compressor input's float64 levels [R, n]"""
    above = level > threshold
    return R.margin(level, threshold), int((np.diff(above.astype(np.int8), axis=-1) != 0).sum()), float(above.mean())


class AmplifyStreamRef:
    def __init__(self, taps, cfg, chunk, soft_clip=True, seg=1024):
        self.taps = np.asarray(taps, np.float64)
        self.rows, self.K = self.taps.shape
        self.cfg, self.W, self.C, self.soft_clip, self.seg = cfg, int(cfg["W"]), int(chunk), soft_clip, seg
        self.xring = np.full((self.rows, self.K - 1 + self.C), np.nan)
        self.zring = np.full((self.rows, self.W - 1 + self.C), np.nan)
        self.pos = np.zeros(self.rows, np.int64)
        self.c = np.ones(self.rows)

    def reset(self, rows=None):
        rows = range(self.rows) if rows is None else rows
        for r in rows:
            self.pos[r], self.c[r] = 0, 1.0

    def _history(self, ring, r, depth):
        """samples pos - depth .. pos - 1 of row r (zero before position 0)"""
        a = self.pos[r] - depth + np.arange(depth)
        return np.where(a >= 0, ring[r, np.maximum(a, 0) % ring.shape[1]], 0.0)

    def _window_sums(self, V, n):
        """V = squares of [W - 1 filtered history | chunk of n]: for chunk sample j the sum of V[j .. j + W - 1]"""
        W, ss, j0 = self.W, np.empty(n), 0
        while j0 < n:
            ln = min(self.seg, W, n - j0)
            mid = V[j0 + ln:j0 + W].sum()
            suf = np.cumsum(V[j0:j0 + ln][::-1])[::-1]
            inc = np.concatenate(([0.0], np.cumsum(V[j0 + W:j0 + W + ln - 1])))
            ss[j0:j0 + ln] = (suf + mid) + inc
            j0 += ln
        return ss

    def feed(self, x):
        x = np.asarray(x, np.float64)
        n = x.shape[1]
        assert x.shape[0] == self.rows and 1 <= n <= self.C
        st = {k: np.empty((self.rows, n)) for k in ("fir", "level", "gain")}
        for r in range(self.rows):
            v = np.concatenate((self._history(self.xring, r, self.K - 1), x[r]))
            y = np.convolve(v, self.taps[r], mode="full")[self.K - 1:self.K - 1 + n]
            V = np.concatenate((self._history(self.zring, r, self.W - 1), y)) ** 2
            lv = np.sqrt(self._window_sums(V, n) / self.W + R.EPS)
            a, b = R.maps(lv, self.cfg)
            c = self.c[r]
            for i in range(n):
                c = c * a[i] + b[i]
                st["gain"][r, i] = c
            # the chunk's slots are written only now: they are not among the history's
            slots = self.pos[r] + np.arange(n)
            self.xring[r, slots % self.xring.shape[1]] = x[r]
            self.zring[r, slots % self.zring.shape[1]] = y
            self.c[r] = c
            self.pos[r] += n
            st["fir"][r], st["level"][r] = y, lv
        st["gain32"] = st["gain"].astype(np.float32).astype(np.float64)
        st["prod"] = st["fir"] * st["gain32"]
        st["out"] = np.tanh(st["prod"]) if self.soft_clip else st["prod"]
        return st

    def flush(self):
        parts = [self.feed(np.zeros((self.rows, self.C))) for _ in range(-(-(self.K - 1) // self.C))]
        self.reset()
        if not parts:
            return {k: np.zeros((self.rows, 0)) for k in ("fir", "level", "gain", "gain32", "prod", "out")}
        return {k: np.concatenate([p[k] for p in parts], -1)[:, :self.K - 1] for k in parts[0]}


def run(ref, x, pieces):
    """feeds x [R, n] in pieces of the given lengths (cycled), then flushes -> dict of [R, n + K - 1] stages"""
    parts, i, k = [], 0, 0
    while i < x.shape[1]:
        n = min(pieces[k % len(pieces)], x.shape[1] - i)
        parts.append(ref.feed(x[:, i:i + n]))
        i, k = i + n, k + 1
    parts.append(ref.flush())
    return {key: np.concatenate([p[key] for p in parts], -1) for key in parts[0]}
