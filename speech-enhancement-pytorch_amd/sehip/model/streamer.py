"""The host side that the chunked streamers share (conv_tasnet_stream.ConvTasNetStreamer, dccrn_stream.DCCRNStreamer).

The contract of a ``ChunkStreamer``: S concurrent streams, Kc frames per chunk.  Every piece of state that a launch both reads and
renews is held twice and one device word `phase` names the current half, so no launch overwrites what it reads and a chunk is ONE chain
of launches on the current stream with the same arguments every time: graph=True captures it once (torch.cuda.graph, after one eager
pass) and feed() copies into a static input and replays.  reset(which) starts some streams afresh and leaves the others untouched.

A subclass names its model class (MODEL) and the words for feed()'s shape (SHAPE_WORDS) and provides _check_cfg(cfg), _sizes(),
_alloc(), _bind() (and _tables() where it packs tables of its own), refresh_weights(), _state_tensors(), _chunk() (which issues every launch through `self._call`, so that
they can be counted), _clear(idx) and flush()."""
import torch

from .._lib import SehipError, call, stream_scope


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


class ChunkStreamer:
    UNCOUNTED_LAUNCHES = 0           # launches of a chunk beyond one per library call

    def __init__(self, model, streams=1, chunk_frames=1, graph=False):
        dev = self.check_args(model, streams, chunk_frames)
        self.model, self.cfg, self.st, self.device = model, model.cfg, model.static, dev
        self.streams, self.chunk_frames, self.graph = streams, chunk_frames, bool(graph)
        self.launches = 0            # launches of one chunk (counted when the chain first runs or is captured)
        self.chunks = 0              # chunks run: its low bit is the host's mirror of `phase`
        self._call, self._graph, self._epoch = call, None, None
        self.delay, self.chunk_samples, self.state_bytes = self._sizes()
        self._tables()
        self._alloc()
        self._bind()
        self._sync_model()

    @classmethod
    def check_args(cls, model, streams=1, chunk_frames=1):
        """The constructor's refusals (before any launch): model type, the subclass's configuration, streams, chunk_frames, device.
        Returns the model's device."""
        who = cls.__name__
        if not isinstance(model, cls.MODEL):
            raise SehipError(f"{who}: model must be a sehip.model.{cls.MODEL.__name__}, got {type(model).__name__}")
        cls._check_cfg(model.cfg)
        for name, v in (("streams", streams), ("chunk_frames", chunk_frames)):
            if not isinstance(v, int) or isinstance(v, bool) or v < 1:
                raise SehipError(f"{who}: {name}={v!r} must be an integer >= 1")
        dev = model.flat_params.device
        if dev.type != "cuda":
            raise SehipError(f"{who}: model is on {dev}: the HIP path needs a gfx950 GPU (no CPU fallback); call model.to('cuda') first")
        return dev

    def _tables(self):
        """packing tables a subclass builds itself, before its buffers (none by default: the plan's tables are copied with the buffers)"""

    def _sync_model(self):
        if self._epoch != self.model.storage_epoch:
            if self.model.flat_params.device != self.device:
                raise SehipError(f"{type(self).__name__}: model moved from {self.device} to {self.model.flat_params.device}; build a new streamer")
            self.refresh_weights()
            self._graph = None          # (captured launches hold pointers into the old flat parameters)
            self._epoch = self.model.storage_epoch

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

    def _run(self, x):
        self.xin.copy_(x)
        if self.graph:
            if self._graph is None:
                self._graph = self._capture()
            self._graph.replay()
        elif self.launches:
            self._chunk()
        else:
            self._counted_chunk()
        self.chunks += 1
        return self.out.clone()

    def feed(self, x):
        """x of the static input's shape (`xin`), fp32 on the model's device -> a copy of the static output (`out`): the offline output
        of the samples fed so far, delayed by `delay` samples."""
        check_feed_input(type(self).__name__, x, self.xin.shape, self.SHAPE_WORDS, self.device)
        with torch.no_grad(), stream_scope():
            self._sync_model()
            return self._run(x)

    def reset(self, which=None):
        """Starts afresh all streams (which=None) or those of an index list / bool mask [S] (_clear says what that means); the other
        streams are untouched."""
        with torch.no_grad():
            self._clear(parse_which(type(self).__name__, which, self.streams, self.device))
