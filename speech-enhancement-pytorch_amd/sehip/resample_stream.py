"""julius.resample_frac chunk by chunk: what ``sehip.ops.resample_frac`` computes on a whole utterance, as the link between the 16 kHz
streaming enhancers and 44.1 / 48 kHz audio (csrc/resample_stream.hip; formulas in include/sehip.h)::

    st = ResampleStreamer(old_sr, new_sr, streams=S, channels=1, chunk_frames=C, graph=False)
    y = st.feed(x)            # x [S, channels, f * old] fp32 on the device -> [S, channels, f * new]; 1 <= f <= C (f == C with graph=True)
    tail = st.flush(tail)     # tail [S, channels, r], 0 <= r < old (or None): the end of the clip; then every stream is fresh
    st.reset(which=None)      # all streams, an index list or a bool mask [S]

old / new is the reduced ratio; the `new` output samples that `old` input samples yield are a frame.  ``cat(feeds, -1)[..., delay:]``
followed by ``flush(tail)`` is ``ops.resample_frac(cat(inputs + [tail]), old_sr, new_sr)`` to the bit: the first ``delay`` =
``delay_frames * new`` output samples of a fresh stream are exact zeros (``delay_frames = ceil(width / old)``: an output frame looks
``width`` input samples ahead), indices before the start read the stream's sample 0 and, in ``flush``, indices past the end read its last
sample, as offline's replicate padding does.  Rows are stream * channels + channel: [S, 1, n] is what the enhancers' streamers take and
[S, 2, n] what ``AmplifyStreamer`` takes.  Inference only: no autograd graph is built.

State per row, on the device only, nothing is ever read back: a frame position and a ring of input samples one chunk longer than the
history ``delay_frames * old + width`` (so the slots a chunk writes are not the slots it reads, and nothing is copied).  A chunk is two
launches (frames + ring store, advance) with the same arguments every time; running, counting, capturing and resetting are
streamcore.StreamCore's, as for the other streamers."""
import numpy as np
import torch

from . import _lib, ops
from ._lib import SehipError, ptr, stream, stream_scope
from .streamcore import StreamCore, check_feed_input

TERM_MAX = 1024
CHUNK_MAX = 4096
ROWS_MAX = 65535
SHAPE_WORDS = "[streams, channels, f * old]"
WHO = "ResampleStreamer"


def _positive_int(name, v):
    if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or v < 1:
        raise SehipError(f"{WHO}: {name}={v!r} must be an integer >= 1")


def reduced_ratio(old_sr, new_sr):
    """(old, new) = old_sr / new_sr reduced; refuses what the kernels do not take (before any launch)"""
    _positive_int("old_sr", old_sr)
    _positive_int("new_sr", new_sr)
    g = int(np.gcd(int(old_sr), int(new_sr)))
    old, new = int(old_sr) // g, int(new_sr) // g
    if old == new:
        raise SehipError(f"{WHO}: {old_sr} -> {new_sr} is the ratio 1 -> 1: nothing to resample")
    if old > TERM_MAX or new > TERM_MAX:
        raise SehipError(f"{WHO}: {old_sr} -> {new_sr} reduces to {old} -> {new}: a term above {TERM_MAX}")
    return old, new


def check_sizes(streams, channels, chunk_frames):
    """The refusals of sizes outside what csrc/resample_stream.hip is built for (before any launch)."""
    _positive_int("streams", streams)
    _positive_int("channels", channels)
    _positive_int("chunk_frames", chunk_frames)
    if streams * channels > ROWS_MAX:
        raise SehipError(f"{WHO}: streams={streams} x channels={channels}: at most {ROWS_MAX} rows")
    if chunk_frames > CHUNK_MAX:
        raise SehipError(f"{WHO}: chunk_frames={chunk_frames} outside [1, {CHUNK_MAX}]")


def check_feed(x, streams, channels, old, chunk_frames, graph, device):
    """feed()'s argument check (before any launch): x [streams, channels, f * old] fp32 on `device`, f == chunk_frames with graph=True and
    1 <= f <= chunk_frames otherwise.  Returns f."""
    if not isinstance(x, torch.Tensor):
        raise SehipError(f"{WHO}.feed: x must be a tensor, got {type(x).__name__}")
    if x.dim() != 3 or x.shape[1] != channels:
        raise SehipError(f"{WHO}.feed: x must have shape {SHAPE_WORDS} = [{streams}, {channels}, f * {old}], got {list(x.shape)}")
    n = int(x.shape[2])
    if n % old:
        raise SehipError(f"{WHO}.feed: x must have shape {SHAPE_WORDS}: {n} samples are not whole frames of old = {old} "
                         f"(the last samples of a clip go to flush(tail))")
    f = n // old
    if graph and f != chunk_frames:
        raise SehipError(f"{WHO}.feed: graph=True replays one captured chunk: f must be chunk_frames = {chunk_frames}, got {f}")
    if not 1 <= f <= chunk_frames:
        raise SehipError(f"{WHO}.feed: f={f} frames outside [1, chunk_frames = {chunk_frames}]")
    check_feed_input(WHO, x, (streams, channels, n), SHAPE_WORDS, device)
    return f


def check_tail(tail, streams, channels, old, device):
    """flush()'s argument check (before any launch): None, or [streams, channels, r] fp32 on `device` with 0 <= r < old.  Returns r."""
    if tail is None:
        return 0
    if not isinstance(tail, torch.Tensor):
        raise SehipError(f"{WHO}.flush: tail must be a tensor or None, got {type(tail).__name__}")
    if tail.dim() != 3 or tuple(tail.shape[:2]) != (streams, channels):
        raise SehipError(f"{WHO}.flush: tail must have shape [streams, channels, r] = [{streams}, {channels}, r], got {list(tail.shape)}")
    r = int(tail.shape[2])
    if r >= old:
        raise SehipError(f"{WHO}.flush: r={r} tail samples: whole frames go to feed(), the tail has 0 <= r < old = {old}")
    if tail.dtype != torch.float32:
        raise SehipError(f"{WHO}.flush: tail must have dtype torch.float32, got {tail.dtype}")
    if tail.device != device:
        raise SehipError(f"{WHO}.flush: tail must be on device {device}, got {tail.device}")
    return r


def delay_frames_of(old, new, width):
    """Dq = ceil(width / old) (host arithmetic in the library)"""
    dq = int(_lib.lib().sehip_rss_delay_frames(old, new, width))
    if dq < 0:
        raise SehipError(f"{WHO}: no delay for the ratio {old} -> {new}, width={width}")
    return dq


def state_bytes_of(rows, old, new, width, chunk_frames):
    """bytes of carried state (host arithmetic in the library): the position and the ring of every row"""
    return int(_lib.lib().sehip_rss_state_bytes(rows, old, new, width, chunk_frames))


def flush_plan(fed, r, old, new, dq):
    """(frames to run, leading samples to drop, samples to keep) of a flush after `fed` whole frames and r tail samples:
    n_out = floor((fed * old + r) * new / old) samples in all, of which max(fed - dq, 0) * new came out of feed()."""
    extra = r * new // old
    run = dq + (1 if extra else 0)                 # the output frames fed - dq .. fed (the last one only if the tail yields a sample)
    drop = max(dq - fed, 0) * new                  # frames before the stream's first: the delay's zeros
    keep = fed * new + extra - max(fed - dq, 0) * new
    return run, drop, keep


class ResampleStreamer(StreamCore):
    SHAPE_WORDS = SHAPE_WORDS

    def __init__(self, old_sr, new_sr, streams=1, channels=1, chunk_frames=1, graph=False, device="cuda"):
        old, new = reduced_ratio(old_sr, new_sr)
        check_sizes(streams, channels, chunk_frames)
        dev = torch.device(device)
        if dev.type != "cuda":
            raise SehipError(f"{WHO}: device {dev}: the HIP path needs a gfx950 GPU (no CPU fallback)")
        if not torch.cuda.is_available():
            raise SehipError(f"{WHO}: no GPU is visible: the HIP path needs a gfx950 GPU (no CPU fallback)")
        dev = torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev
        self._init_core(streams, graph, dev)
        table, width, _, _ = ops.resample_kernels(old, new, dev)
        self.table_t = table.t().contiguous()        # [K][new]: the lanes of a frame read consecutive words
        self.old_sr, self.new_sr, self.channels, self.chunk_frames = int(old_sr), int(new_sr), channels, chunk_frames
        self.in_block, self.out_block, self.width = old, new, width
        self.delay_frames = delay_frames_of(old, new, width)
        self.delay = self.delay_frames * new
        self.history = self.delay_frames * old + width
        self.chunk_in, self.chunk_out = chunk_frames * old, chunk_frames * new
        R = streams * channels
        self.state_bytes = state_bytes_of(R, old, new, width, chunk_frames)
        if self.state_bytes <= 0:
            raise SehipError(f"{WHO}: no state for rows={R}, {old} -> {new}, width={width}, chunk_frames={chunk_frames}")
        z = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device=dev)
        # state (rows = stream * channels + channel)
        self.pos = z(R, dtype=torch.int64)
        self.ring = z(R, self.history + self.chunk_in)
        # work buffers of one chunk
        self.xin, self.out = z(streams, channels, self.chunk_in), z(streams, channels, self.chunk_out)
        self._f, self._end = chunk_frames, -1        # frames of the current chunk and its end length (the launches' arguments)
        self._fed = [0] * streams                    # whole frames fed per stream since its reset (host bookkeeping of flush's length)

    def _state_tensors(self):
        return [self.pos, self.ring]

    def _chunk(self):
        """xin[:, :, :f * old] -> out[:, :, :f * new], state advanced: the frames of [history | chunk] + the ring store, advance"""
        call, R = self._call, self.streams * self.channels
        call("sehip_rss_feed", ptr(self.xin), R, self._f, self.chunk_frames, ptr(self.table_t), self.in_block, self.out_block, self.width,
             ptr(self.pos), ptr(self.ring), self._end, ptr(self.out), stream())
        call("sehip_rss_advance", ptr(self.pos), R, self._f, stream())

    def feed(self, x):
        """x [S, channels, f * old] fp32 on the device -> [S, channels, f * new]: the next f frames of the offline output, `delay` samples
        late."""
        f = check_feed(x, self.streams, self.channels, self.in_block, self.chunk_frames, self.graph, self.device)
        with torch.no_grad(), stream_scope():
            self._f, self._end = f, -1
            self.xin[:, :, :f * self.in_block].copy_(x)
            self._launch()
            self._fed = [n + f for n in self._fed]
            return self.out[:, :, :f * self.out_block].clone()

    def flush(self, tail=None):
        """The rest of the clip, [S, channels, n_out - max(F - delay_frames, 0) * new] for F whole frames fed and a tail of r samples
        (n = F * old + r, n_out = floor(n * new / old)): the frames still owed, indices past the end reading sample n - 1 as offline does
        (several launches when they exceed chunk_frames; never a captured one).  Nothing fed and no tail: an empty tensor.  Afterwards
        every stream is fresh.  F is that of the stream fed longest; a stream reset since and fed fewer than delay_frames frames has
        fewer samples, which start its row, followed by zeros (lengths per stream are not supported)."""
        r = check_tail(tail, self.streams, self.channels, self.in_block, self.device)
        old, new, C = self.in_block, self.out_block, self.chunk_frames
        fed = max(self._fed)
        run, drop, keep = flush_plan(fed, r, old, new, self.delay_frames)
        with torch.no_grad(), stream_scope():
            if fed * old + r == 0 or keep == 0:
                self.reset()
                return torch.zeros(self.streams, self.channels, 0, device=self.device)
            outs, end = [], r
            if r:
                self.xin[:, :, :r].copy_(tail)
            for f0 in range(0, run, C):
                self._f, self._end = min(C, run - f0), end
                self._chunk()
                self.chunks += 1
                outs.append(self.out[:, :, :self._f * new].clone())
                end = 0                              # the ring now holds the replicate-padded stream
            y = torch.cat(outs, -1)
            rows = []
            for s in range(self.streams):            # (one slice for all streams unless one was reset less than delay_frames frames ago)
                _, d, k = flush_plan(self._fed[s], r, old, new, self.delay_frames)
                k = min(k, keep)
                row = y[s, :, d:d + k]
                rows.append(row if k == keep else torch.cat((row, row.new_zeros(self.channels, keep - k)), -1))
            self._f, self._end = C, -1
            self.reset()
            return torch.stack(rows).contiguous()

    def _clear(self, idx):
        """The streams idx start afresh: position 0.  The ring needs no clearing: indices before the start read the new sample 0."""
        ch = torch.arange(self.channels, device=self.device)
        self.pos[(idx[:, None] * self.channels + ch).reshape(-1)] = 0
        for s in idx.tolist():
            self._fed[s] = 0
