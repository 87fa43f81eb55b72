"""julius.resample_frac in front of the device data path (src/dataset.py:117-122, :354-359), the parts that need no GPU: the
interpolation table of sehip.ops.resample_kernels against the oracle's restatement (oracle/demucs_oracle.py), the output length,
the argument checks of the C ABI (made before any HIP call), and DeviceBatcher's `rates` keyword as far as the host goes."""
import types

import numpy as np
import pytest
import torch

RATIOS = ((48000, 16000), (44100, 16000), (16000, 44100), (22050, 16000), (1, 2), (2, 1))


@pytest.mark.parametrize("old_sr,new_sr", RATIOS)
def test_table_matches_the_oracle(old_sr, new_sr):
    from oracle import demucs_oracle as O
    from sehip import ops
    ref, ref_width, ref_old, ref_new = O.resample_kernels(old_sr, new_sr)
    table, width, old, new = ops.resample_kernels(old_sr, new_sr)
    assert (width, old, new) == (ref_width, ref_old, ref_new)
    assert table.dtype == torch.float32 and tuple(table.shape) == (new, 2 * width + old) and table.is_contiguous()
    assert float((table - ref).abs().max()) <= 2e-7
    assert float((table.double().sum(1) - 1.0).abs().max()) <= 1e-6
    assert ops.resample_kernels(old_sr, new_sr)[0] is table                         # cached per reduced ratio
    assert ops.resample_kernels(old_sr * 3, new_sr * 3)[0] is table


@pytest.mark.parametrize("old_sr,new_sr", RATIOS[:3])
def test_output_length(old_sr, new_sr):
    from sehip import _lib, ops
    lib = _lib.lib()
    for n in range(1, 2001):
        assert lib.sehip_resample_out_len(n, old_sr, new_sr) == int(new_sr * n / old_sr)
    assert ops.resample_out_len(264600, old_sr, new_sr) == int(new_sr * 264600 / old_sr)
    assert lib.sehip_resample_out_len(10, 0, 1) < 0 and lib.sehip_resample_out_len(-1, 3, 1) < 0


def test_argument_errors_are_reported_before_any_hip_call():
    from sehip import _lib
    lib = _lib.lib()
    buf = (torch.zeros(8), torch.zeros(2, dtype=torch.int64))                        # host memory: never dereferenced
    p, o = buf[0].data_ptr(), buf[1].data_ptr()
    assert lib.sehip_resample_frac(p, o, 1, p, 6, 2, 52, p, o, None) != 0
    assert b"not reduced" in lib.sehip_last_error()
    assert lib.sehip_resample_frac(p, o, 1, p, 1025, 1, 26, p, o, None) != 0
    assert b"1024" in lib.sehip_last_error()
    assert lib.sehip_resample_frac(p, o, 1, p, 3, 1025, 26, p, o, None) != 0
    assert b"1024" in lib.sehip_last_error()
    assert lib.sehip_resample_frac(p, o, 0, p, 3, 1, 77, p, o, None) != 0
    assert b"rows" in lib.sehip_last_error()
    assert lib.sehip_resample_frac(p, o, 1, p, 3, 1, 0, p, o, None) != 0
    assert b"width" in lib.sehip_last_error()
    with pytest.raises(_lib.SehipError):
        _lib.call("sehip_resample_frac", p, o, 1, p, 4, 2, 51, p, o, None)


def test_resample_frac_has_no_cpu_fallback():
    from sehip import ops
    from sehip._lib import SehipError
    x = torch.zeros(2, 100)
    with pytest.raises(SehipError):
        ops.resample_frac(x, 48000, 16000)
    assert ops.resample_frac(x, 16000, 16000) is x                                   # same rate: nothing to do, on any device


def _batcher(**kw):
    from sehip.data import DeviceBatcher
    return DeviceBatcher(types.SimpleNamespace(segment=0.25, sample_rate=16000), device="cpu", **kw)


def test_rates_keyword_reaches_the_gpu_requirement():
    """a SehipError from require_gpu, not a TypeError: the keyword exists and the host part of the call runs through"""
    from sehip._lib import SehipError
    items = [(torch.zeros(1, 30000), torch.zeros(1, 1, 30000), "u0")]
    with pytest.raises(SehipError, match="needs a gfx950 GPU"):
        _batcher()(items, rates=48000)
    with pytest.raises(SehipError, match="needs a gfx950 GPU"):
        _batcher()(items, rates=[44100])
    with pytest.raises(SehipError, match="rates"):
        _batcher()(items, rates=[48000, 48000])


def test_crop_starts_follow_the_resampled_lengths():
    from oracle import demucs_oracle as O
    raw = [70000, 9000, 52345, 48001, 16000]
    rates = [48000, 44100, 44100, 48000, 16000]
    ref_len = [int(O.resample_frac(torch.zeros(1, n), r, 16000).shape[-1]) for n, r in zip(raw, rates)]
    b = _batcher(sample_length=8000)
    assert b.resampled_lengths(raw, rates) == ref_len
    assert b.resampled_lengths(raw, None) == raw and b.resampled_lengths(raw[:2], 48000) == [70000 // 3, 3000]
    np.random.seed(11)
    got = b.draw_starts(b.resampled_lengths(raw, rates))
    np.random.seed(11)
    want = [int(np.random.randint(max(n, 8000) - 8000 + 1)) for n in ref_len]
    assert got == want and any(got)
    from sehip.data import plan_batch
    plan = plan_batch(b.resampled_lengths(raw, rates), b.seg, 8000, True, got)
    assert [p[2] for p in plan] == [2] * len(raw)


class _RecordingRng:
    def __init__(self):
        self.highs = []

    def randint(self, high):
        self.highs.append(int(high))
        return high - 1


def test_call_draws_its_crop_starts_from_the_resampled_lengths():
    """__call__(items, rates=...) itself: the host part runs up to require_gpu, and by then it has drawn one start per utterance,
    in order, against floor(n * 16000 / rate) -- not against the raw length"""
    from sehip._lib import SehipError
    from sehip.data import DeviceBatcher
    raw, rates = [70000, 9000, 52345, 30000], [48000, 44100, 44100, 16000]
    items = [(torch.zeros(1, n), torch.zeros(1, 1, n), f"u{i}") for i, n in enumerate(raw)]
    rng = _RecordingRng()
    b = DeviceBatcher(types.SimpleNamespace(segment=0.25, sample_rate=16000), sample_length=8000, device="cpu", rng=rng)
    with pytest.raises(SehipError, match="needs a gfx950 GPU"):
        b(items, rates=rates)
    resampled = [70000 // 3, int(16000 * 9000 / 44100), int(16000 * 52345 / 44100), 30000]
    assert rng.highs == [max(n, 8000) - 8000 + 1 for n in resampled]
    assert rng.highs != [max(n, 8000) - 8000 + 1 for n in raw]


def test_an_utterance_that_resamples_to_nothing_is_refused():
    from sehip._lib import SehipError
    items = [(torch.zeros(1, 2), torch.zeros(1, 1, 2), "two samples")]
    with pytest.raises(SehipError, match="leave nothing"):
        _batcher()(items, rates=48000)
    with pytest.raises(SehipError, match="needs a gfx950 GPU"):
        _batcher()(items)                                        # at the target rate nothing changes: the old path takes it
