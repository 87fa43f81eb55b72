"""The host side that the chunked streamers share (conv_tasnet_stream.ConvTasNetStreamer, dccrn_stream.DCCRNStreamer).

The contract of a ``ChunkStreamer``: S concurrent streams, Kc frames per chunk.  Every piece of state that a launch both reads and
renews is held twice and one device word `phase` names the current half, so no launch overwrites what it reads and a chunk is ONE chain
of launches on the current stream with the same arguments every time: graph=True captures it once (torch.cuda.graph, after one eager
pass) and feed() copies into a static input and replays.  reset(which) starts some streams afresh and leaves the others untouched.

A subclass names its model class (MODEL) and the words for feed()'s shape (SHAPE_WORDS) and provides _check_cfg(cfg), _sizes(),
_alloc(), _bind() (and _tables() where it packs tables of its own), refresh_weights(), _state_tensors(), _chunk() (which issues every launch through `self._call`, so that
they can be counted), _clear(idx) and flush().

``StreamCore`` is the part of it that knows no model (running, counting, capturing, feeding and resetting a chunk); ``ChunkStreamer`` adds
the model: its configuration, its flat parameters and the re-packing when their storage moves.  sehip.ha.AmplifyStreamer, which has no
model, sits on the core alone."""
from .._lib import SehipError
from ..streamcore import StreamCore, check_feed_input, parse_which  # noqa: F401


class ChunkStreamer(StreamCore):
    def __init__(self, model, streams=1, chunk_frames=1, graph=False):
        dev = self.check_args(model, streams, chunk_frames)
        self.model, self.cfg, self.st = model, model.cfg, model.static
        self._init_core(streams, graph, dev)
        self.chunk_frames, self._epoch = chunk_frames, None
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

    def _before_chunk(self):
        self._sync_model()
