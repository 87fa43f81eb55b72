"""What the GPU tests of the chunked streamers share (test_gpu_ctn_stream.py, test_gpu_dccrn_stream.py): direct library calls, canary
bands around a state buffer, bit comparison."""
import torch

PAD = 64                       # canary elements on either side of a guarded buffer


def lib_call(name, *a):
    from sehip._lib import call
    call(name, *a)


def cs():
    return torch.cuda.current_stream().cuda_stream


class Guarded:
    """a tensor between two canary bands inside one allocation"""

    def __init__(self, t):
        t = t.contiguous()
        self.canary = {torch.float32: 1234.5, torch.bfloat16: -77.0, torch.int32: 0x5a5a5a5}[t.dtype]
        self.full = torch.full((t.numel() + 2 * PAD,), self.canary, dtype=t.dtype, device="cuda")
        self.t = self.full[PAD:PAD + t.numel()].view(t.shape)
        self.t.copy_(t)

    @property
    def ptr(self):
        return self.t.data_ptr()

    def intact(self):
        return bool((self.full[:PAD] == self.canary).all()) and bool((self.full[-PAD:] == self.canary).all())


def bits(t):
    return t.contiguous().view(torch.int16) if t.dtype == torch.bfloat16 else t.contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b.to(a.device)))
