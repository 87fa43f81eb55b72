"""julius.resample_frac chunk by chunk on the device (csrc/resample_stream.hip, sehip.ResampleStreamer) against the offline entry
(ops.resample_frac) and the float64 formula (tests/resample_stream_ref.py).

  Bits:    cat(feeds)[..., delay:] + flush(tail) has the BITS of ops.resample_frac on the concatenated input: every streamed sample is
           summed by one thread in the order of the offline kernel that serves the ratio (phase / decim / direct, csrc/resample_plan.h).
  float64: independently of the offline entry, every streamed sample is within (K + 2) * 2^-24 * sum_k |h[p][k]| |x_k| of the float64
           formula with the same fp32 table -- the error of a K-term fp32 dot product in any summation order (each product and each
           addition, or each fused step, rounds once, relative 2^-24 of a partial sum of at most that magnitude; the bound
           tests/test_gpu_resample.py holds the offline kernels to).

All cases use streams=2, channels=2 with different data in the four rows, and feed at least three ring lengths of frames so that the
ring wraps.  A case is a few hundred tiny launches at most; the float64 reference of a case is computed once."""
import numpy as np
import pytest
import torch

import ha_ref as R
import resample_stream_ref as SR

pytestmark = pytest.mark.gpu

#          ratio            offline kernel  Dq
RATIOS = (((48000, 16000), "decim", 26),
          ((16000, 48000), "phase", 26),
          ((44100, 16000), "phase", 1),
          ((16000, 44100), "phase", 1),
          ((22050, 16000), "phase", 1),
          ((2, 1), "decim", 26),
          ((1, 2), "phase", 26),
          ((16000, 11025), "direct", 1))
CASES = [(ratio, kind, dq, C) for ratio, kind, dq in RATIOS for C in ((1, 3, 7) if dq == 1 else (1, 5, 32, 100))]
T_TANH = 2.0 ** -22      # tests/test_gpu_ha_stream.py's gate of the streamed hearing-aid stage against offline amplify_torch
_cache = {}


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _streamer(ratio, C, **kw):
    from sehip import ResampleStreamer
    return ResampleStreamer(ratio[0], ratio[1], streams=2, channels=2, chunk_frames=C, **kw)


def _frames_for(st):
    """whole frames that wrap the ring three times"""
    return 3 * -(-(st.history + st.chunk_in) // st.in_block) + 2


def _stream(st, x, sizes, r, flush=True):
    """feeds the whole frames of x [2, 2, n] in pieces of `sizes` frames and flushes the last r samples -> (cat(feeds), flushed)"""
    old = st.in_block
    whole = (x.shape[-1] - r) // old
    assert whole * old + r == x.shape[-1]
    outs, i = [], 0
    for f in SR.pieces(whole, sizes):
        outs.append(st.feed(x[:, :, i:i + f * old]))              # (a strided view: feed() copies it into its static input)
        i += f * old
    feeds = torch.cat(outs, -1) if outs else torch.zeros(2, 2, 0, device=x.device)
    if not flush:
        return feeds, None
    return feeds, st.flush(x[:, :, i:].contiguous() if r else None)


def _input(ratio, n, seed=0):
    return torch.from_numpy(SR.signal(4, n, 1000 * seed + n % 997 + ratio[0] % 89)).reshape(2, 2, n).cuda()


def _offline(x, ratio):
    from sehip import ops
    return ops.resample_frac(x, *ratio)


def _check(st, ratio, kind, x, feeds, tail, what):
    """zero prefix, lengths, the bits of the offline entry, and the float64 gate"""
    from sehip import _lib
    D, n = st.delay, x.shape[-1]
    want = _offline(x, ratio)
    assert _lib.lib().sehip_last_kernel().decode().startswith("resample_" + kind), what
    assert not bool(feeds[..., :D].any()), what                                            # exact zeros
    assert tail.shape[-1] == want.shape[-1] - max(feeds.shape[-1] - D, 0), (what, tail.shape, want.shape, feeds.shape)
    got = torch.cat((feeds[..., D:], tail), -1)
    assert _bits(got, want), (what, int((got.view(torch.int32) != want.view(torch.int32)).sum()), float((got - want).abs().max()))
    key = (ratio, n, float(x[0, 0, :4].sum()))
    if key not in _cache:
        table, width, old, new = SR.tables(*ratio)
        _cache[key] = SR.offline(x.reshape(4, n).cpu().double().numpy(), table, old, new, width)
    y64, mag = _cache[key]
    err = np.abs(got.reshape(4, -1).cpu().double().numpy() - y64)
    bound = SR.bound(mag, 2 * st.width + st.in_block)
    assert bool((err <= bound).all()), (what, float((err / np.maximum(bound, 1e-300)).max()))
    return float((err / np.maximum(bound, 1e-300)).max())


# ---- 1, 2: the bits of offline and the float64 gate -----------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio,kind,dq,C", CASES)
def test_streamed_is_offline_to_the_bit(ratio, kind, dq, C):
    st = _streamer(ratio, C)
    assert (st.delay_frames, st.delay, st.chunk_in, st.chunk_out) == (dq, dq * st.out_block, C * st.in_block, C * st.out_block)
    old, frames = st.in_block, _frames_for(st)
    for r in sorted({0, 1, old - 1} & set(range(old))):
        x = _input(ratio, frames * old + r)
        feeds, tail = _stream(st, x, (C,), r)                     # (the same object again: flush() leaves every stream fresh)
        worst = _check(st, ratio, kind, x, feeds, tail, (ratio, C, r))
        print(f"[resample stream {st.in_block}->{st.out_block} C={C} r={r}] {frames} frames, worst error / bound {worst:.4f}")


@pytest.mark.parametrize("ratio,kind,dq,C", (((44100, 16000), "phase", 1, 3), ((48000, 16000), "decim", 26, 32), ((16000, 48000), "phase", 26, 5),
                                             ((16000, 11025), "direct", 1, 3)))
def test_ragged_feeds(ratio, kind, dq, C):
    st = _streamer(ratio, C)
    old, frames = st.in_block, _frames_for(st)
    x = _input(ratio, frames * old + old - 1, seed=1)
    feeds, tail = _stream(st, x, (1, C, 2, C), old - 1)
    _check(st, ratio, kind, x, feeds, tail, (ratio, "ragged"))


@pytest.mark.parametrize("ratio,kind,C", (((48000, 16000), "decim", 600), ((44100, 16000), "phase", 7), ((16000, 44100), "phase", 3)))
def test_a_chunk_of_several_workgroup_tiles(ratio, kind, C):
    from sehip import _lib
    st = _streamer(ratio, C)
    old, frames = st.in_block, _frames_for(st)
    frames += -frames % C                                         # whole chunks: every launch has C frames
    x = _input(ratio, frames * old, seed=2)
    feeds, _ = _stream(st, x, (C,), 0, flush=False)
    note = _lib.lib().sehip_last_kernel().decode()
    assert note.startswith("resample_stream")
    ft, tiles = int(note.split("ft=")[1].split()[0]), int(note.split("tiles=")[1].split()[0])
    assert C > 2 * ft and tiles == -(-C // ft) >= 3, note
    _check(st, ratio, kind, x, feeds, st.flush(), (ratio, note))


def test_a_window_beyond_the_lds_is_read_from_global_memory():
    """1024 -> 3: K = 18362 taps, a window of 72 KB: no LDS staging; offline this ratio lands on resample_direct_kernel"""
    from sehip import _lib
    ratio, C = (1024, 3), 2
    st = _streamer(ratio, C)
    assert 4 * (2 * st.width + st.in_block) > 64 * 1024 and st.delay_frames == 9
    old, frames = st.in_block, _frames_for(st)
    x = _input(ratio, frames * old + 5, seed=3)
    feeds, _ = _stream(st, x[..., :frames * old], (C,), 0, flush=False)
    note = _lib.lib().sehip_last_kernel().decode()
    assert note.startswith("resample_stream order=direct") and note.endswith("lds=0"), note
    _check(st, ratio, "direct", x, feeds, st.flush(x[..., frames * old:].contiguous()), (ratio, note))


# ---- 3: edges ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio,kind,dq", RATIOS)
def test_edges(ratio, kind, dq):
    st = _streamer(ratio, 5)
    old = st.in_block
    empty = st.flush()
    assert tuple(empty.shape) == (2, 2, 0) and empty.is_cuda and st.chunks == 0           # nothing fed: empty, no launch
    for r in sorted({0, old - 1}):
        x = _input(ratio, old + r, seed=4)                        # one frame (fewer than dq for the 26-frame ratios) and a tail
        feeds, tail = _stream(st, x, (1,), r)
        assert feeds.shape[-1] == st.out_block and not bool(feeds.any())
        want = _offline(x, ratio)
        assert _bits(tail, want), (ratio, r, tail.shape, want.shape)                       # the whole offline output from flush alone
    if old > 1:                                                   # a tail alone
        x = _input(ratio, old - 1, seed=5)
        assert _bits(st.flush(x), _offline(x, ratio))
    frames = dq + 7                                               # after all these flushes: a second utterance on the same object
    x = _input(ratio, frames * old, seed=6)
    feeds, tail = _stream(st, x, (5,), 0)
    _check(st, ratio, kind, x, feeds, tail, (ratio, "second utterance"))


# ---- 4: reset(which) ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio,C,cut", (((44100, 16000), 3, 6), ((48000, 16000), 5, 40)))
def test_reset_of_one_stream(ratio, C, cut):
    outs = {}
    for form in ("list", "mask"):
        st = _streamer(ratio, C)
        old, D = st.in_block, st.delay
        frames = cut + C * -(-(st.delay_frames + 2 * C) // C)
        x = _input(ratio, frames * old, seed=7)
        first, _ = _stream(st, x[..., :cut * old], (C,), 0, flush=False)
        st.reset([0] if form == "list" else torch.tensor([True, False]))
        rest, _ = _stream(st, x[..., cut * old:], (C,), 0, flush=False)
        tail = st.flush()
        outs[form] = torch.cat((first, rest, tail), -1)
        run_on = outs[form][1, :, D:]
        assert _bits(run_on, _offline(x[1], ratio))                                        # stream 1: its whole input
        after = torch.cat((rest, tail), -1)[0]
        assert not bool(after[:, :D].any())
        assert _bits(after[:, D:], _offline(x[0, :, cut * old:].contiguous(), ratio))      # stream 0: what it was fed after the reset
        assert _bits(first[0, :, D:], _offline(x[0], ratio)[:, :cut * st.out_block - D])   # and before it, the uninterrupted run
    assert _bits(outs["list"], outs["mask"])


# ---- 5: graph and launches ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio,kind,C", (((44100, 16000), "phase", 5), ((16000, 44100), "phase", 5), ((48000, 16000), "decim", 32),
                                          ((16000, 48000), "phase", 32)))
def test_graph_replay_and_repeated_runs_give_the_same_bits(ratio, kind, C):
    probe = _streamer(ratio, C)
    old, frames = probe.in_block, _frames_for(probe)
    frames += -frames % C
    r = old - 1
    x = _input(ratio, frames * old + r, seed=8)
    eager = _stream(_streamer(ratio, C), x, (C,), r)
    again = _stream(_streamer(ratio, C), x, (C,), r)
    st = _streamer(ratio, C, graph=True)
    graphed = _stream(st, x, (C,), r)
    assert _bits(eager[0], again[0]) and _bits(eager[1], again[1])
    assert _bits(eager[0], graphed[0]) and _bits(eager[1], graphed[1])
    assert 1 <= st.launches <= 2 and st.chunks >= frames // C
    assert st.state_bytes == sum(t.numel() * t.element_size() for t in st._state_tensors())
    _check(st, ratio, kind, x, graphed[0], graphed[1], (ratio, "graph"))
    feeds, tail = _stream(st, x, (C,), r)                         # the captured chunk again, after a flush
    assert _bits(feeds, eager[0]) and _bits(tail, eager[1])
    from sehip import SehipError
    with pytest.raises(SehipError, match="graph=True"):
        st.feed(x[..., :old])


# ---- 6: the chain it exists for ---------------------------------------------------------------------------------------------------------
def test_microphone_to_hearing_aid_chain():
    """44.1 kHz -> 16 kHz -> (the enhancer's place) -> 44.1 kHz -> NAL-R, compressor, tanh; 12 chunks of 50 ms"""
    from sehip import ResampleStreamer
    from sehip.audio import amplify_torch
    from sehip.ha import AmplifyStreamer, CompressorTorch, NALRTorch
    from sehip.ha.amplifier import stored_to_filter_order
    c = R.CHAIN
    amp, comp, gram = NALRTorch(c["nfir"], 44100), CompressorTorch(fs=44100, **c["compressor"]), c["audiogram"]
    left = stored_to_filter_order(amp.build(np.array(gram["audiogram_levels_l"]), np.array(gram["audiogram_cfs"])).cuda(), "test")
    down = ResampleStreamer(44100, 16000, streams=2, channels=2, chunk_frames=5)
    up = ResampleStreamer(16000, 44100, streams=2, channels=2, chunk_frames=5)
    ha = AmplifyStreamer.from_taps(left.reshape(1, -1).contiguous(), torch.zeros(4, dtype=torch.int32).cuda(), comp, streams=2, chunk_samples=2205)
    assert (down.chunk_in, down.chunk_out, up.chunk_in, up.chunk_out) == (2205, 800, 800, 2205)
    x = _input((44100, 16000), 12 * 2205, seed=9)
    zs, us, outs = [], [], []
    for i in range(12):
        zs.append(down.feed(x[..., i * 2205:(i + 1) * 2205]))
        us.append(up.feed(zs[-1]))
        outs.append(ha.feed(us[-1]))
    z, u, out = torch.cat(zs, -1), torch.cat(us, -1), torch.cat(outs, -1)
    assert not bool(z[..., :160].any()) and _bits(z[..., 160:], _offline(x, (44100, 16000))[..., :z.shape[-1] - 160])
    want_u = torch.cat((torch.zeros(2, 2, 441).cuda(), _offline(z, (16000, 44100))), -1)[..., :u.shape[-1]]
    assert _bits(u, want_u)
    off = amplify_torch(u[:, None], amp, comp, gram, soft_clip=True)[:, 0][..., :u.shape[-1]]
    off_plain = amplify_torch(u[:, None], amp, comp, gram, soft_clip=False)[:, 0][..., :u.shape[-1]]
    mag = off_plain.double().abs()
    worst = float(((out.double() - off.double()).abs() - mag * 2.0 ** -22).max())
    print(f"[resample stream chain] worst |streamed - offline| - |offline| 2^-22 = {worst:.3e} (gate {T_TANH:.3e})")
    assert bool(((out.double() - off.double()).abs() <= mag * 2.0 ** -22 + T_TANH).all())
