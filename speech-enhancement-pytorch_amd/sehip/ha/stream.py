"""The hearing-aid back end chunk by chunk: what ``sehip.audio.amplify_torch`` computes on a whole utterance (NAL-R FIR, compressor,
tanh), sample-synchronously behind a streaming enhancer (csrc/ha_stream.hip; formulas in include/sehip.h)::

    st = AmplifyStreamer(enhancer, compressor, audiograms, streams=S, chunk_samples=64, graph=False)
    y = st.feed(x)            # x [S, 2, n] fp32 on the device -> [S, 2, n]; 1 <= n <= chunk_samples (n == chunk_samples with graph=True)
    tail = st.flush()         # [S, 2, nfir]: zeros pushed through, the compressor running on; then every stream is fresh
    st.reset(which=None)      # all streams, an index list or a bool mask [S]: one listener leaves, another arrives

``cat(feeds, -1)`` followed by ``flush()`` is ``amplify_torch(x[:, None], ...)[:, 0]`` of the concatenated input, all n_total + nfir
samples of it; there is no delay beyond the filter's own (``delay == 0``; ``group_delay == nfir // 2`` is the linear-phase filter's and is
there offline as well).  The filtered signal has the bits of the offline FIR.  Inference only: no autograd graph is built.

State per row (row = stream x ear), on the device only, nothing is ever read back: a position, the last K - 1 input samples and the last
W - 1 filtered samples in rings one chunk longer than the history (so the slots a chunk writes are not the slots it reads, and nothing
is copied), and the gain c as a float64.  Nothing but c is accumulated across chunks: the window sums are float64 sums formed afresh in
every chunk from the stored samples.  A chunk is three launches (FIR, compressor, advance) with the same arguments every time; running,
counting, capturing and resetting are streamcore.StreamCore's, as for the enhancers' streamers."""
import numpy as np
import torch

from .. import _lib
from .._lib import SehipError, ptr, stream, stream_scope
from ..streamcore import StreamCore, check_feed_input
from .amplifier import K_MAX, NALRTorch, stored_to_filter_order
from .compressor import CompressorTorch

W_MAX = 1 << 20
CHUNK_MAX = 1 << 16
ROWS_MAX = 65535
SHAPE_WORDS = "[streams, 2 (ears), n]"


def _positive_int(name, v):
    if not isinstance(v, int) or isinstance(v, bool) or v < 1:
        raise SehipError(f"AmplifyStreamer: {name}={v!r} must be an integer >= 1")


def check_sizes(streams, chunk_samples, K, W):
    """The refusals of sizes outside what csrc/ha_stream.hip is built for (before any launch)."""
    _positive_int("streams", streams)
    _positive_int("chunk_samples", chunk_samples)
    if 2 * streams > ROWS_MAX:
        raise SehipError(f"AmplifyStreamer: streams={streams}: 2 rows per stream, at most {ROWS_MAX} rows")
    if chunk_samples > CHUNK_MAX:
        raise SehipError(f"AmplifyStreamer: chunk_samples={chunk_samples} outside [1, {CHUNK_MAX}]")
    if not isinstance(K, int) or not 1 <= K <= K_MAX:
        raise SehipError(f"AmplifyStreamer: K={K} taps outside [1, {K_MAX}]")
    if not isinstance(W, int) or not 1 <= W <= W_MAX:
        raise SehipError(f"AmplifyStreamer: window W={W} (rms_buffer_size * fs) outside [1, {W_MAX}]")


def check_feed(x, streams, chunk_samples, graph, device):
    """feed()'s argument check (before any launch): x [streams, 2, n] fp32 on `device`, n == chunk_samples with graph=True and
    1 <= n <= chunk_samples otherwise.  Returns n."""
    who = "AmplifyStreamer"
    if not isinstance(x, torch.Tensor):
        raise SehipError(f"{who}.feed: x must be a tensor, got {type(x).__name__}")
    if x.dim() != 3 or x.shape[1] != 2:
        raise SehipError(f"{who}.feed: x must have shape {SHAPE_WORDS} = [{streams}, 2, n], got {list(x.shape)}")
    n = x.shape[2]
    if graph and n != chunk_samples:
        raise SehipError(f"{who}.feed: graph=True replays one captured chunk: n must be chunk_samples = {chunk_samples}, got {n}")
    if not 1 <= n <= chunk_samples:
        raise SehipError(f"{who}.feed: n={n} samples outside [1, chunk_samples = {chunk_samples}]")
    check_feed_input(who, x, (streams, 2, n), SHAPE_WORDS, device)
    return n


def audiogram_list(audiograms, streams):
    """one dict for all streams, or a list of `streams` dicts -> a list of `streams` dicts"""
    if isinstance(audiograms, dict):
        return [audiograms] * streams
    if not isinstance(audiograms, (list, tuple)) or len(audiograms) != streams or not all(isinstance(a, dict) for a in audiograms):
        n = len(audiograms) if isinstance(audiograms, (list, tuple)) else type(audiograms).__name__
        raise SehipError(f"AmplifyStreamer: audiograms must be one dict or a list of streams = {streams} dicts, got {n}")
    return list(audiograms)


def state_bytes_of(streams, K, W, chunk_samples):
    """bytes of carried state (host arithmetic in the library): positions, both rings and c of 2 * streams rows"""
    return int(_lib.lib().sehip_has_state_bytes(2 * streams, K, W, chunk_samples))


class AmplifyStreamer(StreamCore):
    SHAPE_WORDS = SHAPE_WORDS

    def __init__(self, enhancer, compressor, audiograms, streams=1, chunk_samples=64, soft_clip=True, own_right_filter=False, graph=False,
                 device="cuda"):
        """enhancer: NALRTorch; compressor: CompressorTorch; audiograms: the dict amplify_torch takes ('audiogram_cfs',
        'audiogram_levels_l', 'audiogram_levels_r') for all streams, or a list of `streams` of them (one listener per stream).

        By default the right ear goes through the LEFT ear's taps, the reference's quirk that amplify_torch reproduces (src/audio.py:49);
        the right ear's filter is still designed, so that its ValueError surfaces.  own_right_filter=True gives each ear its own."""
        if not isinstance(enhancer, NALRTorch):
            raise SehipError(f"AmplifyStreamer: enhancer must be a sehip.ha.NALRTorch, got {type(enhancer).__name__}")
        self._check_compressor(compressor)
        check_sizes(streams, chunk_samples, enhancer.nfir + 1, compressor.win_len)
        grams = audiogram_list(audiograms, streams)
        if torch.device(device).type != "cuda":
            self._device(device)
        sets, row_set = [], []
        for a in grams:
            cfs = np.array(a["audiogram_cfs"])
            left = enhancer.build(np.array(a["audiogram_levels_l"]), cfs)
            right = enhancer.build(np.array(a["audiogram_levels_r"]), cfs)      # designed in any case, as in the reference
            row_set += [len(sets), len(sets) + 1 if own_right_filter else len(sets)]
            sets += [left, right]
        dev = self._device(device)
        taps = stored_to_filter_order(torch.cat(sets, 0).to(dev), "AmplifyStreamer")
        self._setup(taps, torch.tensor(row_set, dtype=torch.int32, device=dev), compressor, streams, chunk_samples, soft_clip, graph)

    @classmethod
    def from_taps(cls, taps, row_set, compressor, streams=1, chunk_samples=64, soft_clip=True, graph=False):
        """taps [F, K] fp32 on the device in filter order (what stored_to_filter_order returns); row_set int32 [streams * 2] on the
        device: the tap set of row stream * 2 + ear."""
        self = cls.__new__(cls)
        cls._check_compressor(compressor)
        if not torch.is_tensor(taps) or taps.dim() != 2 or taps.dtype != torch.float32:
            raise SehipError(f"AmplifyStreamer.from_taps: taps must be an fp32 tensor [F, K], got "
                             f"{list(taps.shape) if torch.is_tensor(taps) else type(taps).__name__}")
        check_sizes(streams, chunk_samples, int(taps.shape[1]), compressor.win_len)
        if not 1 <= taps.shape[0] <= 65535:
            raise SehipError(f"AmplifyStreamer.from_taps: F={taps.shape[0]} tap sets outside [1, 65535]")
        if not torch.is_tensor(row_set) or row_set.dtype != torch.int32 or tuple(row_set.shape) != (2 * streams,):
            raise SehipError(f"AmplifyStreamer.from_taps: row_set must be int32 [streams * 2] = [{2 * streams}], got "
                             f"{(row_set.dtype, list(row_set.shape)) if torch.is_tensor(row_set) else type(row_set).__name__}")
        _lib.require_gpu(taps, "AmplifyStreamer.from_taps (taps)")
        _lib.require_gpu(row_set, "AmplifyStreamer.from_taps (row_set)")
        if row_set.device != taps.device:
            raise SehipError(f"AmplifyStreamer.from_taps: taps on {taps.device}, row_set on {row_set.device}")
        self._setup(taps.contiguous(), row_set.contiguous(), compressor, streams, chunk_samples, soft_clip, graph)
        return self

    @staticmethod
    def _check_compressor(compressor):
        if not isinstance(compressor, CompressorTorch):
            raise SehipError(f"AmplifyStreamer: compressor must be a sehip.ha.CompressorTorch, got {type(compressor).__name__}")

    @staticmethod
    def _device(device):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise SehipError(f"AmplifyStreamer: device {dev}: the HIP path needs a gfx950 GPU (no CPU fallback)")
        if not torch.cuda.is_available():
            raise SehipError("AmplifyStreamer: no GPU is visible: the HIP path needs a gfx950 GPU (no CPU fallback)")
        return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev

    def _setup(self, taps, row_set, compressor, streams, chunk_samples, soft_clip, graph):
        self._init_core(streams, graph, taps.device)
        self.taps, self.row_set, self.compressor, self.soft_clip = taps, row_set, compressor, bool(soft_clip)
        self.K, self.W, self.chunk_samples = int(taps.shape[1]), int(compressor.win_len), chunk_samples
        self.nfir, self.delay, self.group_delay = self.K - 1, 0, (self.K - 1) // 2
        self.state_bytes = state_bytes_of(streams, self.K, self.W, chunk_samples)
        if self.state_bytes <= 0:
            raise SehipError(f"AmplifyStreamer: no state for streams={streams}, K={self.K}, W={self.W}, chunk_samples={chunk_samples}")
        # the settings as the launches take them, fixed here: a captured chunk holds them
        self._settings = (float(compressor.threshold), float(compressor.attack), float(compressor.release), float(compressor.attenuation))
        S, C, dev = streams, chunk_samples, self.device
        z = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device=dev)
        # state (rows = stream * 2 + ear)
        self.pos = z(2 * S, dtype=torch.int64)
        self.xring = z(2 * S, self.K - 1 + C)
        self.zring = z(2 * S, self.W - 1 + C)
        self.c = torch.ones(2 * S, dtype=torch.float64, device=dev)
        # work buffers of one chunk
        self.c_next = z(2 * S, dtype=torch.float64)
        self.xin, self._filt, self._gain, self.out = z(S, 2, C), z(S, 2, C), z(S, 2, C), z(S, 2, C)
        self._n = C                      # samples of the current chunk (the launches' argument; always C under graph=True)
        self._tail = None                # after flush(): the tail's (filtered, gain)

    def _state_tensors(self):
        return [self.pos, self.xring, self.zring, self.c]

    def _chunk(self):
        """xin[:, :, :n] -> out[:, :, :n], state advanced: FIR over [history | chunk], compressor from the carried c, advance"""
        call, R, n, C = self._call, 2 * self.streams, self._n, self.chunk_samples
        thr, att, rel, atten = self._settings
        call("sehip_has_fir", ptr(self.xin), R, n, C, ptr(self.taps), self.taps.shape[0], self.K, self.W, ptr(self.row_set), ptr(self.pos),
             ptr(self.xring), ptr(self.zring), ptr(self._filt), stream())
        call("sehip_has_compress", ptr(self.zring), R, n, C, self.W, ptr(self.pos), ptr(self.c), thr, att, rel, atten, int(self.soft_clip),
             ptr(self.c_next), ptr(self._gain), ptr(self.out), stream())
        call("sehip_has_advance", ptr(self.pos), ptr(self.c), ptr(self.c_next), R, n, stream())

    def _feed(self, x, n):
        self._n, self._tail = n, None
        self.xin[:, :, :n].copy_(x)
        self._launch()
        return self.out[:, :, :n].clone()

    def feed(self, x):
        """x [S, 2, n] fp32 on the device -> [S, 2, n]: the next n samples of the offline output."""
        n = check_feed(x, self.streams, self.chunk_samples, self.graph, self.device)
        with torch.no_grad(), stream_scope():
            return self._feed(x, n)

    @property
    def filtered(self):
        """[S, 2, n] copy of the last chunk's FIR output (after flush(): of the tail, [S, 2, nfir])"""
        return self._filt[:, :, :self._n].clone() if self._tail is None else self._tail[0].clone()

    @property
    def gain(self):
        """[S, 2, n] copy of the last chunk's compressor gain (after flush(): of the tail, [S, 2, nfir])"""
        return self._gain[:, :, :self._n].clone() if self._tail is None else self._tail[1].clone()

    def flush(self):
        """The nfir samples after the last one fed, [S, 2, nfir]: zeros pushed through the filter, the compressor running on (with
        nfir > chunk_samples several zero chunks, of which the first nfir samples are kept).  Afterwards every stream is fresh, and
        `filtered` / `gain` hold the tail's."""
        C = self.chunk_samples
        with torch.no_grad(), stream_scope():
            zeros = torch.zeros(self.streams, 2, C, device=self.device)
            outs, filt, gain = [], [], []
            for _ in range(-(-self.nfir // C)):
                outs.append(self._feed(zeros, C))
                filt.append(self.filtered)
                gain.append(self.gain)
            cut = lambda ts: (torch.cat(ts, -1)[:, :, :self.nfir].contiguous() if ts else
                              torch.zeros(self.streams, 2, 0, device=self.device))
            self.reset()
            self._tail = (cut(filt), cut(gain))
            return cut(outs)

    def _clear(self, idx):
        """A new listener on the streams idx: position 0 and c = 1.  The rings need no clearing: samples before position 0 read as zero."""
        rows = torch.stack((2 * idx, 2 * idx + 1), -1).reshape(-1)
        self.pos[rows] = 0
        self.c[rows] = 1.0
