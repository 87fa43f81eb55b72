"""The one cache of device buffers that ops, metric and loss keep per shape, and the one spelling of a device that keys it."""
import torch


def canonical_device(device):
    """torch.device with the index spelled out, so that 'cuda' and 'cuda:0' name one cache entry"""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def _capturing():
    """(torch raises from is_current_stream_capturing() where no GPU is visible, and host-side callers build workspaces on 'cpu')"""
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


class CaptureAwareCache:
    """get(key, make, *args) -> the value stored under `key`, or make(*args), which is stored unless the current stream is recording
    a graph: a buffer born inside a capture lives in that graph's pool, so it serves that recording only and the next caller makes its
    own.  A caller that records into a hipGraph therefore asks for its buffers BEFORE the capture begins; the recording then allocates
    nothing but its results.  (make's arguments are passed through so that a hit on the hot path builds no closure.)"""

    def __init__(self):
        self.store = {}

    def get(self, key, make, *args):
        value = self.store.get(key)
        if value is None:
            value = make(*args)
            if not _capturing():
                self.store[key] = value
        return value
