"""float64 numpy restatement of the streaming resampler (csrc/resample_stream.hip, sehip.ResampleStreamer), shared by
tests/test_resample_stream_host.py and tests/test_gpu_resample_stream.py:

  offline()            the offline formula of include/sehip.h on whole rows, with the magnitude sum_k |h[p][k]| |x_k| of every output
                       (the bound (K + 2) * 2^-24 * that sum is the error of a K-term fp32 dot product in any summation order: each of
                       the K products and K - 1 additions -- or K fused steps -- rounds once, relative 2^-24 of a partial sum that is
                       at most the magnitude; tests/test_gpu_resample.py holds the offline kernels to the same bound)
  ResampleStreamRef    the streamer as a state machine working with exactly the state the device keeps: per row a frame position and a
                       ring of H + C * old samples; both clamps; flush() through end lengths; reset(which)
"""
import numpy as np

EPS32 = 2.0 ** -24


def tables(old_sr, new_sr):
    """(table float64 [new][K] holding the fp32 table's values, width, old, new)"""
    from sehip import ops
    table, width, old, new = ops.resample_kernels(old_sr, new_sr)
    return table.double().numpy(), width, old, new


def offline(x, table, old, new, width):
    """x [rows, n] -> (y [rows, floor(n * new / old)], mag of the same shape): y[q new + p] = sum_k h[p][k] x[clamp(q old + k - width)]"""
    x = np.asarray(x, dtype=np.float64)
    rows, n = x.shape
    K = table.shape[1]
    m = n * new // old
    if m == 0:
        return np.zeros((rows, 0)), np.zeros((rows, 0))
    frames = -(-m // new)
    idx = np.clip(np.arange((frames - 1) * old + K) - width, 0, n - 1)
    win = np.lib.stride_tricks.sliding_window_view(x[:, idx], K, axis=-1)[:, ::old]      # [rows, frames, K]
    y = win @ table.T
    mag = np.abs(win) @ np.abs(table).T
    return y.reshape(rows, -1)[:, :m], mag.reshape(rows, -1)[:, :m]


def bound(mag, K):
    return (K + 2) * EPS32 * mag


def delay_frames(old, width):
    return -(-width // old)


def flush_lengths(fed, r, old, new, dq):
    """(frames to run, leading samples to drop, samples to keep) of a flush after `fed` frames and r tail samples"""
    extra = r * new // old
    return dq + (1 if extra else 0), max(dq - fed, 0) * new, fed * new + extra - max(fed - dq, 0) * new


class ResampleStreamRef:
    def __init__(self, old_sr, new_sr, rows, chunk_frames):
        self.table, self.width, self.old, self.new = tables(old_sr, new_sr)
        self.K, self.rows, self.C = self.table.shape[1], rows, chunk_frames
        self.dq = delay_frames(self.old, self.width)
        self.H = self.dq * self.old + self.width
        self.L = self.H + chunk_frames * self.old
        self.pos = np.zeros(rows, dtype=np.int64)
        self.ring = np.full((rows, self.L), np.nan)               # (a slot that is read before it is written would show)
        self.fed = 0
        self.reads = []                                           # per call: lowest chunk index read, highest minus the chunk's length

    def _sample(self, r, x, i, end):
        """samples at chunk indices i (int array) of row r: chunk x [f * old], ring history, both clamps"""
        base = int(self.pos[r]) * self.old
        i = i.copy()
        if end >= 0:
            i = np.minimum(i, end - 1)
        i = np.where(base + i < 0, -base, i)
        assert i.min() >= -self.H and i.max() < len(x)
        slot = (base + i) % self.L
        hist = self.ring[r, np.where(i < 0, slot, 0)]
        return np.where(i >= 0, x[np.maximum(i, 0)], hist)

    def step(self, x, end=-1):
        """x [rows, f * old] (columns from `end` on are ignored when end >= 0) -> [rows, f * new]; state advanced by f frames"""
        old, new, K = self.old, self.new, self.K
        f = x.shape[1] // old
        assert x.shape == (self.rows, f * old) and 1 <= f <= self.C and end <= f * old
        out = np.zeros((self.rows, f * new))
        w = np.arange((f - 1) * old + K) - self.dq * old - self.width
        self.reads.append((int(w[0]), int(w[-1]) - f * old))
        store = np.arange(f * old)
        for r in range(self.rows):
            win = np.lib.stride_tricks.sliding_window_view(self._sample(r, x[r], w, end), K)[::old]
            y = (win @ self.table.T)
            y[np.arange(f) + self.pos[r] - self.dq < 0] = 0.0
            out[r] = y.reshape(-1)
            vals = self._sample(r, x[r], store, end)              # (read before the ring is written: no slot is both)
            read_slots = set(((int(self.pos[r]) * old + w[w < 0]) % self.L).tolist())
            write_slots = ((int(self.pos[r]) * old + store) % self.L)
            assert not read_slots & set(write_slots.tolist())
            self.ring[r, write_slots] = vals
        self.pos += f
        return out

    def feed(self, x):
        self.fed += x.shape[1] // self.old
        return self.step(np.asarray(x, dtype=np.float64))

    def flush(self, tail=None):
        r = 0 if tail is None else tail.shape[1]
        assert r < self.old
        run, drop, keep = flush_lengths(self.fed, r, self.old, self.new, self.dq)
        if self.fed * self.old + r == 0 or keep == 0:
            self.reset()
            return np.zeros((self.rows, 0))
        outs, end = [], r
        for f0 in range(0, run, self.C):
            f = min(self.C, run - f0)
            x = np.full((self.rows, f * self.old), np.nan)        # only the tail is real
            if f0 == 0 and r:
                x[:, :r] = tail
            outs.append(self.step(x, end))
            end = 0
        self.reset()
        return np.concatenate(outs, -1)[:, drop:drop + keep]

    def reset(self, rows=None):
        if rows is None:
            self.pos[:] = 0
            self.fed = 0
        else:
            self.pos[list(rows)] = 0


def pieces(total, sizes):
    """piece lengths (cycled through `sizes`) that add up to `total`"""
    out, k = [], 0
    while sum(out) < total:
        out.append(min(sizes[k % len(sizes)], total - sum(out)))
        k += 1
    return out


def signal(rows, n, seed):
    """different data in every row, with an offset so that the replicate padding matters"""
    rng = np.random.RandomState(seed)
    return (0.3 * rng.standard_normal((rows, n)) + 0.05 * (1 + np.arange(rows))[:, None]).astype(np.float32)
