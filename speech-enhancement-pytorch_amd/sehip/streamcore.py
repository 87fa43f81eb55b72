"""The model-free core of the chunked streamers (model/streamer.py adds the model; ha/stream.py has none): feed()'s and reset()'s
argument checks and ``StreamCore``, which runs one chunk as a chain of launches, counts them, captures the chain once under graph=True
(torch.cuda.graph, after one eager pass) and replays it on static buffers."""
import torch

from ._lib import SehipError, call, stream_scope


def check_feed_input(who, x, want, words, device):
    """feed()'s argument check (before any launch) of the streamer class `who`: x of shape `want`, which `words` describes, fp32 on
    `device`."""
    if not isinstance(x, torch.Tensor):
        raise SehipError(f"{who}.feed: x must be a tensor, got {type(x).__name__}")
    if x.shape != want:
        raise SehipError(f"{who}.feed: x must have shape {words} = {list(want)}, got {list(x.shape)}")
    if x.dtype != torch.float32:
        raise SehipError(f"{who}.feed: x must have dtype torch.float32, got {x.dtype}")
    if x.device != device:
        raise SehipError(f"{who}.feed: x must be on device {device} (the model's), got {x.device}")


def parse_which(who, which, streams, device):
    """reset()'s `which` -- None (all streams), an index list / tensor, or a bool mask [streams] -- as a long index tensor on `device`."""
    if which is None:
        return torch.arange(streams, device=device)
    idx = torch.as_tensor(which, device=device)
    if idx.dtype == torch.bool:
        if tuple(idx.shape) != (streams,):
            raise SehipError(f"{who}.reset: which as a bool mask must have shape [{streams}], got {list(idx.shape)}")
        return idx.nonzero().reshape(-1)
    idx = idx.reshape(-1).long()
    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= streams):
        raise SehipError(f"{who}.reset: which holds a stream index outside [0, {streams})")
    return idx


class StreamCore:
    """The part of a chunked streamer that knows no model: one chunk as a chain of launches (`_chunk`, every launch through
    `self._call`) that is run, counted, captured once and replayed, fed and reset.  A subclass sets `streams`, `graph`, `device` through
    _init_core() and provides the static buffers `xin` / `out`, SHAPE_WORDS, _state_tensors(), _chunk(), _clear(idx) and, where
    something must be checked before every chunk, _before_chunk().  (sehip.ha.AmplifyStreamer is one without a model.)"""
    UNCOUNTED_LAUNCHES = 0           # launches of a chunk beyond one per library call

    def _init_core(self, streams, graph, device):
        self.streams, self.graph, self.device = streams, bool(graph), device
        self.launches = 0            # launches of one chunk (counted when the chain first runs or is captured)
        self.chunks = 0              # chunks run: its low bit is the host's mirror of `phase`
        self._call, self._graph = call, None

    def _before_chunk(self):
        """what feed() does before the chunk runs (nothing by default)"""

    def _counted_chunk(self):
        """_chunk() with its launches counted into `launches`"""
        n = [0]

        def counting(name, *args):
            n[0] += 1
            call(name, *args)

        self._call = counting
        try:
            self._chunk()
        finally:
            self._call = call
        self.launches = n[0] + self.UNCOUNTED_LAUNCHES

    def _capture(self):
        """Captures one chunk.  The chain runs once eagerly first, on the capturing stream, with the state saved and put back: the engine
        sizes its per-stream scratch (split-K partial sums) on a product's first launch, which must not happen inside a capture."""
        call("sehip_init")
        torch.cuda.synchronize(self.device)
        side = torch.cuda.Stream(device=self.device)
        saved = [t.clone() for t in self._state_tensors()]
        with torch.cuda.stream(side), stream_scope():
            self._chunk()
        side.synchronize()
        for t, v in zip(self._state_tensors(), saved):
            t.copy_(v)
        torch.cuda.synchronize(self.device)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side), stream_scope():     # (records, runs nothing: the state does not move)
            self._counted_chunk()
        return g

    def _launch(self):
        """one chunk on the static buffers: replayed, run, or run and counted"""
        if self.graph:
            if self._graph is None:
                self._graph = self._capture()
            self._graph.replay()
        elif self.launches:
            self._chunk()
        else:
            self._counted_chunk()
        self.chunks += 1

    def _run(self, x):
        self.xin.copy_(x)
        self._launch()
        return self.out.clone()

    def feed(self, x):
        """x of the static input's shape (`xin`), fp32 on the model's device -> a copy of the static output (`out`): the offline output
        of the samples fed so far, delayed by `delay` samples."""
        check_feed_input(type(self).__name__, x, self.xin.shape, self.SHAPE_WORDS, self.device)
        with torch.no_grad(), stream_scope():
            self._before_chunk()
            return self._run(x)

    def reset(self, which=None):
        """Starts afresh all streams (which=None) or those of an index list / bool mask [S] (_clear says what that means); the other
        streams are untouched."""
        with torch.no_grad():
            self._clear(parse_which(type(self).__name__, which, self.streams, self.device))
