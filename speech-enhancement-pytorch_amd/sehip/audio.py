"""The reference's src/audio.py: channel conversion and the hearing-aid chain (NAL-R FIR, compressor, tanh) on the device."""
import numpy as np
import torch

from .ha.amplifier import NALRTorch, check_signal, fir_apply, stored_to_filter_order
from .ha.compressor import CompressorTorch, compress_rows


def convert_audio_channels(wav, channels=2):
    """[..., src_channels, length] -> [..., channels, length] (src/audio.py:6-31, from facebookresearch/denoiser): the same count
    passes through, channels=1 takes the mean, a mono source is expanded (a view), a wider source keeps its first channels;
    fewer-but-not-mono raises ValueError.  Torch view operations only."""
    *shape, src_channels, length = wav.shape
    if src_channels == channels:
        return wav
    if channels == 1:
        return wav.mean(dim=-2, keepdim=True)
    if src_channels == 1:
        return wav.expand(*shape, channels, length)
    if src_channels >= channels:
        return wav[..., :channels, :]
    raise ValueError('The audio file has less channels than requested but is not mono.')


def amplify_torch(signal: torch.Tensor, enhancer: NALRTorch, compressor: CompressorTorch, audiogram, soft_clip=True):
    """signal [B, S, 2, n] fp32 on the device -> [B, S, 2, n + nfir]: per ear NAL-R FIR, compressor, tanh (with soft_clip).
    audiogram: the dict the reference indexes ('audiogram_cfs', 'audiogram_levels_l', 'audiogram_levels_r').

    Reference quirk, reproduced: src/audio.py:49 moves the LEFT ear's taps to the device a second time where it means the right
    ear's, so the right channel is filtered with the left ear's filter.  The right ear's filter is still designed (a ValueError of
    its audiogram is raised as in the reference) and then not used.

    Both ears are rows of one FIR launch and one compressor pass.  Differentiable with respect to the signal; the compressor's gain
    is a constant of the backward pass (the reference rebuilds it from a detached array): d(signal) = FIR^T(d(out) * (1 - out^2) *
    gain).  The device copy of the taps is cached in `enhancer` per audiogram, so a repeated call issues kernels only."""
    check_signal(signal, 4, "amplify_torch")
    if signal.shape[2] != 2:
        raise ValueError(f"amplify_torch: signal of shape {tuple(signal.shape)}; axis 2 holds the two ears")
    cfs = np.array(audiogram["audiogram_cfs"])
    levels = np.array([audiogram["audiogram_levels_l"], audiogram["audiogram_levels_r"]])
    left = enhancer.build_on(levels[0], cfs, signal.device)
    enhancer.build_on(levels[1], cfs, signal.device)              # designed and, as in the reference, not used
    taps = stored_to_filter_order(left, "amplify_torch")
    b, s, _, n = signal.shape
    filtered = fir_apply(signal.reshape(b * s * 2, n), taps)
    out, _ = compress_rows(filtered, compressor, soft_clip=soft_clip)
    return out.reshape(b, s, 2, n + taps.shape[-1] - 1)
