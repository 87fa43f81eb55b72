"""Compressor of the hearing-aid stage (the reference's src/ha/compressor.py CompressorTorch) on the device.

The reference pulls every row to the host and walks it sample by sample; here the level detector and the gain recurrence are a
float64 reduce-then-scan (csrc/hearing_aid.hip; formula in include/sehip.h) and nothing leaves the device.  The gain is a constant
of the backward pass, as in the reference: d(signal) = d(out) * gain.
"""
import torch

from .. import _lib
from .._lib import SehipError, call, ptr, stream
from .amplifier import check_signal


class _Compress(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, comp, soft_clip):
        rows, n = z.shape
        z = z.contiguous()
        doubles = _lib.lib().sehip_ha_compressor_ws_doubles(rows, n, comp.win_len)
        if doubles <= 0:
            raise SehipError(f"compressor: no workspace for rows={rows}, n={n}, W={comp.win_len} (rows <= 65535, n <= 2^30, W >= 1)")
        ws = torch.empty(doubles, device=z.device, dtype=torch.float64)
        gain = torch.empty_like(z)
        out = torch.empty_like(z)
        call("sehip_ha_compressor_fwd", ptr(z), rows, n, comp.win_len, float(comp.threshold), float(comp.attack), float(comp.release),
             float(comp.attenuation), int(bool(soft_clip)), ptr(ws), ptr(gain), ptr(out), stream())
        ctx.save_for_backward(out, gain)
        ctx.soft_clip = int(bool(soft_clip))
        ctx.mark_non_differentiable(gain)
        return out, gain

    @staticmethod
    def backward(ctx, dout, _dgain):
        out, gain = ctx.saved_tensors
        dout = dout.contiguous()
        dz = torch.empty_like(out)
        call("sehip_ha_compressor_bwd", ptr(dout), ptr(out), ptr(gain), out.numel(), ctx.soft_clip, ptr(dz), stream())
        return dz, None, None


def compress_rows(z, comp, soft_clip=False):
    """z [rows, n] fp32 on the device -> (out, gain), both [rows, n]: out = z * gain (tanh of it with soft_clip), gain the fp32
    value of the float64 recurrence.  Differentiable with respect to z with the gain held constant."""
    check_signal(z, 2, "CompressorTorch")
    return _Compress.apply(z, comp, soft_clip)


class CompressorTorch:
    def __init__(self, fs=44100, attack=5, release=20, threshold=1, attenuation=0.0001, rms_buffer_size=0.2, makeup_gain=1):
        """attack / release in milliseconds; rms_buffer_size in seconds (the level window is int(rms_buffer_size * fs) samples);
        makeup_gain is stored and unused, as in the reference."""
        self.fs = fs
        self.rms_buffer_size = rms_buffer_size
        self.set_attack(attack)
        self.set_release(release)
        self.threshold = threshold
        self.attenuation = attenuation
        self.eps = 1e-8
        self.makeup_gain = makeup_gain
        self.win_len = int(self.rms_buffer_size * self.fs)
        if self.win_len < 1:
            raise SehipError(f"CompressorTorch: rms_buffer_size * fs = {self.rms_buffer_size} * {self.fs} gives a window of "
                             f"W = {self.win_len} < 1 samples")

    def set_attack(self, t_msec):
        self.attack = 1 / (t_msec / 1000) / self.fs

    def set_release(self, t_msec):
        self.release = 1 / (t_msec / 1000) / self.fs

    def process(self, signal):
        """signal [B, S, n] fp32 on the device -> [B, S, n], every row times its gain; no host round trip"""
        check_signal(signal, 3, "CompressorTorch.process")
        b, s, n = signal.shape
        out, _ = compress_rows(signal.reshape(b * s, n), self, soft_clip=False)
        return out.reshape(b, s, n)
