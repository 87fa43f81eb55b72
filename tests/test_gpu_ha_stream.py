"""The hearing-aid stage chunk by chunk on the device (csrc/ha_stream.hip, sehip.ha.AmplifyStreamer) against offline fir_apply /
compress_rows / amplify_torch, tests/ha_ref.py in float64 and the recorded reference call.

The gates are tests/test_gpu_ha.py's: gain within 2^-23 relative of the fp32 rounding of the float64 recurrence, product within
|z c| 2^-22, with tanh T_TANH = 2^-22 more, the chain against the recorded reference at ACT_TOL = 5e-5.  The filtered signal is held to
the BITS of offline fir_apply on the whole input.  Where two device results that each meet the gates are compared with each other
(streamed against offline amplify_torch) the same bounds hold between them: the gains are roundings of float64 values 1e-12 apart, so at
most one ulp (<= 2^-23 relative) apart; the products then differ by at most |z c| (2^-23 + 2 x 2^-24); tanh has slope <= 1 and the device's
tanh is within 1.52 x 2^-24 of float64's on both sides (test_gpu_ha.py's measurement), 3.04 x 2^-24 < T_TANH together.

Every case runs a few hundred tiny launches at most; float64 oracles are computed once per case and shared."""
import os

import numpy as np
import pytest
import torch

import ha_ref as R
import ha_stream_ref as SR
from util import rel_err

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACT_TOL = 5e-5
T_TANH = 2.0 ** -22
CHAIN_MARGIN = 1e-5      # (test_gpu_ha.py's: the oracle's levels come from the float64 FIR, the device's from its fp32 one)
_cache = {}


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _compressor(W, fs=SR.COMP_FS):
    from sehip.ha import CompressorTorch
    comp = CompressorTorch(fs=fs, **R.CHAIN["compressor"])
    comp.win_len = W
    return comp


def _pieces(n_total, sizes):
    """piece lengths (cycled through `sizes`) that add up to n_total"""
    out, k = [], 0
    while sum(out) < n_total:
        out.append(min(sizes[k % len(sizes)], n_total - sum(out)))
        k += 1
    return out


def _stream(st, x, pieces, flush=True):
    """feeds x [S, 2, n] piece by piece (and flushes) -> (out, filtered, gain), each the concatenation over the pieces (and the tail)"""
    outs, filt, gain, i = [], [], [], 0
    for n in pieces:
        outs.append(st.feed(x[:, :, i:i + n]))                    # (a strided view: feed() copies it into its static input)
        filt.append(st.filtered)
        gain.append(st.gain)
        i += n
    assert i == x.shape[-1]
    if flush:
        outs.append(st.flush())
        filt.append(st.filtered)
        gain.append(st.gain)
    return torch.cat(outs, -1), torch.cat(filt, -1), torch.cat(gain, -1)


def _gates(z64, gain, out, st, what, clipped=None):
    """tests/test_gpu_ha.py's gates on rows [R, n]: gain, product (soft_clip=False output) and, with `clipped`, tanh"""
    want32 = st["gain"].astype(np.float32).astype(np.float64)
    prod = z64 * st["gain"]
    gerr = np.abs(gain.double().cpu().numpy() - want32) / np.abs(want32)
    perr = np.abs(out.double().cpu().numpy() - prod)
    print(f"[ha stream {what}] worst gain error {gerr.max() / 2.0 ** -23:.3f} x 2^-23, worst product error "
          f"{(perr / np.maximum(np.abs(prod) * 2.0 ** -22, 1e-300)).max():.3f} x bound")
    assert bool((gerr <= 2.0 ** -23).all()), (what, int(gerr.argmax()), float(gerr.max()))
    assert bool((perr <= np.abs(prod) * 2.0 ** -22).all()), (what, int(perr.argmax()))
    if clipped is not None:
        terr = np.abs(clipped.double().cpu().numpy() - np.tanh(prod))
        print(f"[ha stream {what}] worst |out - tanh64| = {terr.max():.3e}")
        assert bool((terr <= np.abs(prod) * 2.0 ** -22 + T_TANH).all()), (what, int(terr.argmax()), float(terr.max()))


# ---- 1: FIR bits ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,C", ((1, 7), (2, 1), (33, 8), (33, 32), (33, 100), (221, 64), (1025, 64), (1025, 3000)))
def test_filtered_signal_has_the_bits_of_offline_fir(K, C):
    from sehip.ha import AmplifyStreamer, fir_apply
    W = 5
    g = torch.Generator().manual_seed(300 + K + C)
    taps = (torch.randn(2, K, generator=g) / K ** 0.5).cuda()
    row_set = torch.tensor([0, 1, 0, 1], dtype=torch.int32).cuda()
    ring = max(K - 1 + C, W - 1 + C)
    n_total = 3 * ring + (C // 2 + 1 if C > 1 else 0)             # every ring wraps more than once; a ragged last piece
    x = (0.3 * torch.randn(2, 2, n_total, generator=g) + 0.05).cuda()
    st = AmplifyStreamer.from_taps(taps, row_set, _compressor(W), streams=2, chunk_samples=C)
    assert st.delay == 0 and st.group_delay == (K - 1) // 2 and st.chunk_samples == C
    pieces = _pieces(n_total, (C,))
    assert n_total > 3 * (K - 1 + C) - 1 and (C == 1 or pieces[-1] < C)
    out, filt, _ = _stream(st, x, pieces)
    want = fir_apply(x.reshape(4, n_total), taps, row_set).reshape(2, 2, n_total + K - 1)
    assert tuple(out.shape) == tuple(filt.shape) == (2, 2, n_total + K - 1)
    assert _bits(filt, want), (K, C, int((filt != want).sum()))
    assert st.launches == 3 and st.chunks == len(pieces) + -(-(K - 1) // C)
    assert st.state_bytes == 4 * (16 + 4 * (K - 1 + C) + 4 * (W - 1 + C))


# ---- 2, 3: compressor against float64 ---------------------------------------------------------------------------------------------
def _comp_case(W, n):
    key = ("comp", W, n)
    if key not in _cache:
        z, cfg = SR.comp_signal(W, n), SR.comp_cfg(W)
        _cache[key] = (z, cfg, R.compress(z.numpy(), cfg, soft_clip=False, loop=True, direct_level=True))
    return _cache[key]


def _identity_streamer(W, C, soft_clip, **kw):
    from sehip.ha import AmplifyStreamer
    return AmplifyStreamer.from_taps(torch.ones(1, 1).cuda(), torch.zeros(4, dtype=torch.int32).cuda(), _compressor(W), streams=2, chunk_samples=C,
                                     soft_clip=soft_clip, **kw)


@pytest.mark.parametrize("W,n,C", SR.COMP_CASES + (SR.LONG_CASE,))
def test_compressor_against_float64(W, n, C):
    """identity filter (K = 1, tap 1.0): the level fed to the oracle is the input's own.  The last case is the long stream (400 chunks):
    the same gates at every sample -- nothing but c is carried, so nothing grows."""
    from sehip.ha import compress_rows
    z, cfg, st64 = _comp_case(W, n)
    m, crossings, share = SR.input_checks(st64["level"], cfg["threshold"])
    print(f"[ha stream W={W} n={n} C={C}] level margin {m:.3e}, {share:.1%} above the threshold, {crossings} crossings")
    assert m >= R.MIN_MARGIN, "the INPUT is at fault (a level too close to the threshold), not the kernel"
    assert crossings >= 2 and 0.05 < share < 0.95
    x = z.cuda().reshape(2, 2, n)
    pieces = _pieces(n, (C,))
    plain, filt, gain = _stream(_identity_streamer(W, C, False), x, pieces)
    clipped, _, gain_c = _stream(_identity_streamer(W, C, True), x, pieces)
    assert _bits(filt, x) and _bits(gain, gain_c) and tuple(plain.shape) == (2, 2, n)
    _gates(st64["fir"], gain.reshape(4, n), plain.reshape(4, n), st64, f"W={W} n={n} C={C}", clipped.reshape(4, n))
    _, off_gain = compress_rows(z.cuda(), _compressor(W), soft_clip=False)
    print(f"[ha stream W={W} n={n} C={C}] samples whose gain differs from offline compress_rows: "
          f"{int((off_gain != gain.reshape(4, n)).sum())} of {4 * n}")


# ---- 4: streams and reset -----------------------------------------------------------------------------------------------------------
def test_streams_are_independent_and_reset_touches_only_its_stream():
    from sehip.ha import AmplifyStreamer, NALRTorch
    amp, comp, C, chunks, cut = NALRTorch(32, 16000), _compressor(64), 32, 10, 5
    grams = [dict(audiogram_cfs=R.CFS, audiogram_levels_l=R.AUDIOGRAMS[a], audiogram_levels_r=R.AUDIOGRAMS[b])
             for a, b in (("docstring", "severe"), ("severe", "mild_low"), ("mild_low", "docstring"))]
    g = torch.Generator().manual_seed(41)
    x = (0.05 * torch.randn(3, 2, chunks * C, generator=g)).cuda()
    pieces = [C] * chunks
    whole = _stream(AmplifyStreamer(amp, comp, grams, streams=3, chunk_samples=C), x, pieces, flush=False)
    for s in range(3):
        alone = _stream(AmplifyStreamer(amp, comp, grams[s], streams=1, chunk_samples=C), x[s:s + 1], pieces, flush=False)
        for a, b in zip(alone, whole):
            assert _bits(a[0], b[s]), s
    st = AmplifyStreamer(amp, comp, grams, streams=3, chunk_samples=C)
    first = _stream(st, x[:, :, :cut * C], pieces[:cut], flush=False)
    st.reset([1])
    rest = _stream(st, x[:, :, cut * C:], pieces[cut:], flush=False)
    fresh = _stream(AmplifyStreamer(amp, comp, grams[1], streams=1, chunk_samples=C), x[1:2, :, cut * C:], pieces[cut:], flush=False)
    for a, b, c, w in zip(first, rest, fresh, whole):
        got = torch.cat((a, b), -1)
        assert _bits(got[0], w[0]) and _bits(got[2], w[2])        # untouched streams: the uninterrupted run
        assert _bits(b[1], c[0])                                  # stream 1 continues as a fresh streamer does
    assert not _bits(rest[1][1], whole[1][1, :, cut * C:])        # (and not as before: its filter history is gone)
    st.reset(torch.tensor([False, False, True]))                  # a bool mask; and all streams
    st.reset()
    for a, w in zip(_stream(st, x, pieces, flush=False), whole):
        assert _bits(a, w)


# ---- 5: flush -----------------------------------------------------------------------------------------------------------------------
def test_flush_gives_the_offline_tail_and_a_fresh_streamer():
    from sehip.ha import AmplifyStreamer, fir_apply
    K, C, W, n = 221, 64, 64, 1000                                # nfir = 220 > C: four zero chunks, the first 220 samples kept
    g = torch.Generator().manual_seed(52)
    taps = (torch.randn(1, K, generator=g) / K ** 0.5).cuda()
    x = SR.comp_signal(W, n).cuda().reshape(2, 2, n)
    st = AmplifyStreamer.from_taps(taps, torch.zeros(4, dtype=torch.int32).cuda(), _compressor(W), streams=2, chunk_samples=C, soft_clip=False)
    pieces = _pieces(n, (C,))
    out, filt, gain = _stream(st, x, pieces)
    z = fir_apply(x.reshape(4, n), taps)
    assert tuple(out.shape) == (2, 2, n + K - 1) and _bits(filt.reshape(4, -1), z)
    cfg = SR.comp_cfg(W)
    st64 = R.compress(z.cpu().numpy(), cfg, soft_clip=False, loop=True, direct_level=True)      # the oracle on the device's own z
    m, crossings, share = SR.input_checks(st64["level"], cfg["threshold"])
    assert m >= R.MIN_MARGIN and crossings >= 2 and 0.05 < share < 0.95, (m, crossings, share)
    _gates(st64["fir"], gain.reshape(4, -1), out.reshape(4, -1), st64, "flush K=221 C=64 (tail included)")
    again = _stream(st, x, pieces)                                # after flush(): a new streamer's bits
    assert all(_bits(a, b) for a, b in zip(again, (out, filt, gain)))
    # nfir = 0: an empty tail, and a fresh streamer after it
    st0 = _identity_streamer(W, C, False)
    a = st0.feed(x[:, :, :C].contiguous())
    tail = st0.flush()
    assert tuple(tail.shape) == (2, 2, 0) and tail.is_cuda and tuple(st0.filtered.shape) == (2, 2, 0)
    assert _bits(st0.feed(x[:, :, :C].contiguous()), a)


# ---- 6, 7: graph, chain -------------------------------------------------------------------------------------------------------------
def _chain_objects():
    from sehip.ha import CompressorTorch, NALRTorch
    c = R.CHAIN
    return NALRTorch(c["nfir"], c["fs"]), CompressorTorch(fs=c["fs"], **c["compressor"]), c["audiogram"]


def _golden():
    if "chain" not in _cache:
        with np.load(os.path.join(ROOT, "tests", "golden", "ha_chain.npz")) as z:
            _cache["chain"] = {k: z[k] for k in z.files}
    return _cache["chain"]


def test_graph_replay_and_repeated_runs_give_the_same_bits():
    from sehip import _lib
    from sehip.ha import AmplifyStreamer
    amp, comp, gram = _chain_objects()
    x = torch.from_numpy(_golden()["signal"][:, 0, :, :640]).cuda().contiguous()
    pieces = [64] * 10
    eager = _stream(AmplifyStreamer(amp, comp, gram, streams=2, chunk_samples=64), x, pieces)
    again = _stream(AmplifyStreamer(amp, comp, gram, streams=2, chunk_samples=64), x, pieces)
    st = AmplifyStreamer(amp, comp, gram, streams=2, chunk_samples=64, graph=True)
    graphed = _stream(st, x, pieces)
    assert st.launches == 3 and st._graph is not None
    for e, a, gr in zip(eager, again, graphed):
        assert _bits(e, a) and _bits(e, gr)
    with pytest.raises(_lib.SehipError, match="graph=True"):
        st.feed(x[:, :, :63].contiguous())
    was = _lib.lib().sehip_get_deterministic()
    try:
        for mode in (1, 0):
            _lib.call("sehip_set_deterministic", mode)
            for e, a in zip(eager, _stream(st, x, pieces)):       # (the same captured chunk, after its flush)
                assert _bits(e, a), mode
            for e, a in zip(eager, _stream(AmplifyStreamer(amp, comp, gram, streams=2, chunk_samples=64), x, pieces)):
                assert _bits(e, a), mode
    finally:
        _lib.call("sehip_set_deterministic", was)


def test_streamed_chain_matches_the_reference_and_offline_amplify_torch():
    from sehip.audio import amplify_torch
    from sehip.ha import AmplifyStreamer, compress_rows
    fx = _golden()
    assert float(fx["margin"]) >= CHAIN_MARGIN
    amp, comp, gram = _chain_objects()
    sig = torch.from_numpy(fx["signal"]).cuda()                   # [2, 1, 2, 4000]
    x = sig[:, 0].contiguous()
    off = amplify_torch(sig, amp, comp, gram, soft_clip=True)[:, 0]
    off_plain = amplify_torch(sig, amp, comp, gram, soft_clip=False)[:, 0]
    for what, sizes in (("C=64", (64,)), ("ragged", (1, 64, 17, 33, 50, 2, 63))):
        pieces = _pieces(4000, sizes)
        out, filt, gain = _stream(AmplifyStreamer(amp, comp, gram, streams=2, chunk_samples=64), x, pieces)
        plain, filt_p, gain_p = _stream(AmplifyStreamer(amp, comp, gram, streams=2, chunk_samples=64, soft_clip=False), x, pieces)
        assert tuple(out.shape) == (2, 2, 4032) and _bits(filt, filt_p) and _bits(gain, gain_p)
        e = rel_err(out.cpu(), fx["out"][:, 0])
        print(f"[ha stream chain {what}] {len(pieces)} pieces, vs reference {e:.3e}")
        assert e < ACT_TOL and rel_err(plain.cpu(), fx["comp"][:, 0]) < ACT_TOL
        # against offline amplify_torch on the device: gain (offline's, from compress_rows on the same filtered bits), product, tanh
        off_rows, off_gain = compress_rows(filt.reshape(4, 4032), comp, soft_clip=False)
        assert _bits(off_rows.reshape(2, 2, 4032), off_plain)
        assert bool(((gain.reshape(4, 4032).double() - off_gain.double()).abs() <= off_gain.double() * 2.0 ** -23).all()), what
        mag = off_plain.double().abs()
        assert bool(((plain.double() - off_plain.double()).abs() <= mag * 2.0 ** -22).all()), what
        assert bool(((out.double() - off.double()).abs() <= mag * 2.0 ** -22 + T_TANH).all()), what
        gerr = ((plain.double() - off_plain.double()).abs() / mag.clamp_min(1e-300))[filt.abs() > 1e-3]
        print(f"[ha stream chain {what}] worst |streamed - offline| / |offline| of the product {float(gerr.max()) / 2.0 ** -23:.3f} x 2^-23")


# ---- 8: ears ------------------------------------------------------------------------------------------------------------------------
def test_right_ear_uses_the_left_filter_unless_it_gets_its_own():
    from sehip.ha import AmplifyStreamer, fir_apply
    from sehip.ha.amplifier import stored_to_filter_order
    amp, comp, gram = _chain_objects()
    x = torch.from_numpy(_golden()["signal"][:, 0, :, :320]).cuda().contiguous()
    left = stored_to_filter_order(amp.build(gram["audiogram_levels_l"], gram["audiogram_cfs"]).cuda(), "test")
    right = stored_to_filter_order(amp.build(gram["audiogram_levels_r"], gram["audiogram_cfs"]).cuda(), "test")
    assert not torch.equal(left, right)
    pieces = [64] * 5
    _, quirk, _ = _stream(AmplifyStreamer(amp, comp, gram, streams=2, chunk_samples=64), x, pieces)
    _, own, _ = _stream(AmplifyStreamer(amp, comp, gram, streams=2, chunk_samples=64, own_right_filter=True), x, pieces)
    by_left = fir_apply(x.reshape(4, 320), left).reshape(2, 2, 352)
    by_right = fir_apply(x.reshape(4, 320), right).reshape(2, 2, 352)
    assert _bits(quirk, by_left)                                  # both ears through the LEFT ear's taps (src/audio.py:49)
    assert _bits(own[:, 0], by_left[:, 0]) and _bits(own[:, 1], by_right[:, 1])
    assert not _bits(own[:, 1], quirk[:, 1])
    # behind a mono enhancer: convert_audio_channels' expanded VIEW is fed as it is and gives the bits of a contiguous copy
    from sehip.audio import convert_audio_channels
    mono = convert_audio_channels(x[:, :1], 2)
    assert not mono.is_contiguous()
    a = _stream(AmplifyStreamer(amp, comp, gram, streams=2, chunk_samples=64), mono, pieces)
    b = _stream(AmplifyStreamer(amp, comp, gram, streams=2, chunk_samples=64), mono.contiguous(), pieces)
    assert all(_bits(p, q) for p, q in zip(a, b)) and _bits(a[0][:, 0], a[0][:, 1])
