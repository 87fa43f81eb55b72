"""CPU: the host code the chunked streamers share (sehip.model.streamer): reset()'s `which` parser, on CPU tensors.  No GPU calls."""
import pytest
import torch


def test_parse_which():
    """None, an index list, a long tensor, an empty list and a bool mask give a long index tensor on the device asked for; a mask of
    another shape, a negative index and an index equal to `streams` are refused under the calling class's name"""
    from sehip import SehipError
    from sehip.model.streamer import parse_which
    cpu = torch.device("cpu")
    parse = lambda which: parse_which("SomeStreamer", which, 3, cpu)
    for which, want in ((None, [0, 1, 2]), ([0, 2], [0, 2]), (torch.tensor([2, 1]), [2, 1]), ([], []), (torch.tensor([True, False, True]), [0, 2]),
                        ([False, False, False], []), (1, [1]), (torch.tensor([[0], [1]], dtype=torch.int32), [0, 1])):
        idx = parse(which)
        assert idx.dtype == torch.long and idx.device == cpu and idx.dim() == 1 and idx.tolist() == want, which
    for which in (torch.tensor([True, False]), torch.ones(1, 3, dtype=torch.bool)):
        with pytest.raises(SehipError, match=r"SomeStreamer\.reset: which as a bool mask must have shape \[3\], got \[" + str(which.shape[0])):
            parse(which)
    for which in ([-1], [0, 3], torch.tensor([3])):
        with pytest.raises(SehipError, match=r"SomeStreamer\.reset: which holds a stream index outside \[0, 3\)"):
            parse(which)
