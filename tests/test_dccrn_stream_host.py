"""CPU: chunked streaming of DCCRN -- the restatement tests/dccrn_stream_ref.py (history rows, the lag per decoder level, the spectrum
ring, the hop-periodic window energy, the `end` rule) against the offline oracle, the closed forms of delay and state_bytes, the
refusals of sehip.model.DCCRNStreamer, and the sehip_dcs_* entry points (declared, bound, argument validation before any HIP call).
No GPU calls."""
import os
import re

import pytest
import torch

import dccrn_stream_ref as SR
from oracle import dccrn_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOPS = 21
GEOMETRIES = [(400, 100), (320, 160), (512, 128)]
ENTRY_POINTS = ("sehip_dcs_analysis", "sehip_dcs_norm_hist", "sehip_dcs_lstm_carry", "sehip_dcs_synthesis", "sehip_dcs_mark_end",
                "sehip_dcs_advance")
# fp32 re-ordering only (see test_restatement_equals_offline)
GATE = 5e-7


def _cfg(win_len, win_inc, **kw):
    kw = dict(dict(rnn_layers=2, rnn_units=128, kernel_num=[16] * 6, masking_mode="E"), **kw)
    return O.DCCRNConfig(win_len=win_len, win_inc=win_inc, length=HOPS * win_inc, **kw)


def _signals(win_inc, seed=0):
    """S = 2 different signals: noise, and a chirp-like tone under weaker noise"""
    g = torch.Generator().manual_seed(seed)
    n = HOPS * win_inc
    t = torch.arange(n, dtype=torch.float32)
    a = 0.1 * torch.randn(n, generator=g)
    b = 0.2 * torch.sin(2e-2 * t + 3e-6 * t * t) + 0.02 * torch.randn(n, generator=g)
    return torch.stack([a, b])[:, None]


_OFFLINE = {}


def _offline(geo, mode="E"):
    """(cfg, parameters, signals, offline output) of a geometry: computed once, shared, never written"""
    if (geo, mode) not in _OFFLINE:
        cfg = _cfg(*geo, masking_mode=mode)
        p = SR.make_params(cfg)
        x = _signals(geo[1])
        with torch.no_grad():
            off = O.dccrn_forward(p, x, cfg, training=False)
        _OFFLINE[(geo, mode)] = (cfg, p, x, off)
    return _OFFLINE[(geo, mode)]


@pytest.mark.parametrize("geo", GEOMETRIES)
@pytest.mark.parametrize("Kc", [1, 3, 7])
def test_restatement_equals_offline(geo, Kc):
    """cat(feeds)[..., D:] + flush == O.dccrn_forward(training=False, length=N), NoSim, fp32, S = 2.

    The two differ by fp32 re-ordering only (a convolution over Kc + 1 frames instead of T, one overlap-add sum per chunk).  Measured
    on the CPU, max |difference| over the nine cases: 5.6e-8 .. 1.27e-7 against an offline rms of 1.8e-2 .. 3.1e-2 (4e-6 of the rms at
    most: a few fp32 epsilons, 6e-8, of intermediate values of order 1).  Gate: max |difference| < GATE = 5e-7 absolute, 4 x the
    largest measured value (one bf16 rounding of such an output would be 1e-4).  The bf16 gates of the
    GPU tests do not apply here."""
    cfg, p, x, off = _offline(geo)
    with torch.no_grad():
        ref = SR.StreamRef(p, cfg, 2, Kc)
        out, tail = SR.run_stream(ref, x)
    D = ref.delay
    assert D == (6 + geo[0] // geo[1] - 1) * geo[1] and tuple(out.shape) == tuple(x.shape) and tuple(tail.shape) == (2, 1, D)
    assert float(out[..., :D].abs().max()) == 0.0                                      # the delay: exact zeros
    full = torch.cat([out[..., D:], tail], -1)
    dev = float((full - off).abs().max())
    print(f"geo {geo} Kc {Kc}: max |stream - offline| {dev:.3e}, offline rms {float(off.pow(2).mean().sqrt()):.3e}")
    assert float(off[0].abs().max()) > 1e-3 and float(off[1].abs().max()) > 1e-3 and not torch.equal(off[0], off[1])
    assert dev < GATE
    assert float((tail - off[..., -D:]).abs().max()) < GATE                            # (the tail alone: a wrong tail cannot hide)
    assert ref.pos == [0, 0] and float(ref.tail.abs().max()) == 0.0                    # flush resets


@pytest.mark.parametrize("mode", ["C", "R"])
def test_restatement_masking_modes(mode):
    cfg, p, x, off = _offline((400, 100), mode)
    with torch.no_grad():
        out, tail = SR.run_stream(SR.StreamRef(p, cfg, 2, 3), x)
    assert float((torch.cat([out[..., 900:], tail], -1) - off).abs().max()) < GATE


def test_restatement_real_batchnorm_and_three_layers():
    cfg = _cfg(400, 100, use_cbn=False, rnn_layers=3, kernel_num=[16, 16, 32, 32, 64, 64])
    p, x = SR.make_params(cfg), _signals(100, seed=4)
    with torch.no_grad():
        off = O.dccrn_forward(p, x, cfg, training=False)
        out, tail = SR.run_stream(SR.StreamRef(p, cfg, 2, 7), x)
    assert float((torch.cat([out[..., 900:], tail], -1) - off).abs().max()) < GATE


def test_zeros_instead_of_flush_do_not_reproduce_the_tail():
    """Offline, the frames past the end of the clip are ABSENT (the t + 1 tap of every decoder layer contributes nothing); frames of
    silence still carry biases and BatchNorm shifts.  Feeding D zero samples instead of flush() therefore misses the last hops by
    orders of magnitude more than the gate: the `end` rule is needed."""
    cfg, p, x, off = _offline((400, 100))
    with torch.no_grad():
        ref = SR.StreamRef(p, cfg, 2, 3)
        SR.run_stream(ref, x, flush=False)
        fed = torch.cat([ref.feed(torch.zeros(2, 1, 300)) for _ in range(3)], -1)
    want = off[..., -900:]
    assert float((fed[..., :300] - want[..., :300]).abs().max()) < GATE                # (hops whose frames all lie inside the clip)
    dev = float((fed[..., -600:] - want[..., -600:]).abs().max())
    print(f"zeros instead of flush: max deviation over the last 6 hops {dev:.3e}")
    assert dev > 1000 * GATE


def test_partial_reset():
    """resetting stream 1 of 2 in mid-clip: that stream continues as a fresh one, stream 0 does not notice"""
    cfg, p, x, _ = _offline((400, 100))
    n = 300
    with torch.no_grad():
        a, plain, fresh = (SR.StreamRef(p, cfg, 2, 3) for _ in range(3))
        for j in range(3):
            assert torch.equal(a.feed(x[..., j * n:(j + 1) * n]), plain.feed(x[..., j * n:(j + 1) * n]))
        a.reset(torch.tensor([False, True]))
        for j in range(3, 7):
            ya, yp, yf = (r.feed(x[..., j * n:(j + 1) * n]) for r in (a, plain, fresh))
            assert torch.equal(ya[0], yp[0]) and torch.equal(ya[1], yf[1])
        assert a.pos == [21, 12] and not torch.equal(ya[1], yp[1])


def test_delay_and_state_bytes_closed_forms():
    from sehip.model import DCCRN
    from sehip.model import dccrn_stream as DS
    for (wl, wi), want in zip(GEOMETRIES, (900, 1120, 1152)):
        assert DS.delay_of(wl, wi) == SR.delay_of(wl, wi) == want
    kn = [16, 32, 64, 128, 256, 256]
    m = DCCRN(length=1600)
    for S in (1, 3):
        per = (2 * 300 * 4) * 2 + 2 * 6 * 257 * 8 + 2 * 1024                                            # carry, tail, ring, encoder input row
        per += 2 * 2 * (6 * 128 * 16 + 5 * 64 * 32 + 4 * 32 * 64 + 3 * 16 * 128 + 2 * 8 * 256 + 1 * 4 * 256)   # encoder outputs 0 .. 5
        per += 2 * 2 * 4 * 256 + 2 * 2 * (8 * 256 + 16 * 128 + 32 * 64 + 64 * 32 + 128 * 16)             # projection, decoder outputs 0 .. 4
        per += 2 * 4 * 64 * 6 + 8                                                                       # two layers of (h, c); pos, end
        assert DS.state_bytes_of(m.cfg, S) == S * per + 4 == SR.state_bytes_of(kn, 2, 128, 400, 100, S)
    cfg = _cfg(320, 160, rnn_layers=3, rnn_units=64)
    m2 = DCCRN(rnn_layers=3, rnn_units=64, win_len=320, win_inc=160, kernel_num=[16] * 6, length=1600)
    assert DS.state_bytes_of(m2.cfg, 2) == SR.StreamRef(SR.make_params(cfg), cfg, 2, 4).state_bytes


def test_refusals_name_the_reason():
    from sehip import SehipError
    from sehip.model import DCCRN, DCCRNStreamer
    from sehip.model.dccrn_stream import check_feed_input
    kw = dict(kernel_num=[16] * 6, length=1600)
    with pytest.raises(SehipError, match="use_clstm=False"):
        DCCRNStreamer(DCCRN(use_clstm=False, **kw))
    with pytest.raises(SehipError, match="win_len=400 is not a multiple of win_inc=150"):
        DCCRNStreamer(DCCRN(win_len=400, win_inc=150, **kw))
    with pytest.raises(SehipError, match="model must be a sehip.model.DCCRN, got Linear"):
        DCCRNStreamer(torch.nn.Linear(2, 2))
    m = DCCRN(**kw)
    with pytest.raises(SehipError, match="model is on cpu"):
        DCCRNStreamer(m)
    with pytest.raises(SehipError, match="streams=0"):
        DCCRNStreamer(m, streams=0)
    with pytest.raises(SehipError, match="streams=2.0"):
        DCCRNStreamer(m, streams=2.0)
    with pytest.raises(SehipError, match="chunk_frames=-1"):
        DCCRNStreamer(m, chunk_frames=-1)
    with pytest.raises(SehipError, match="streams=True"):
        DCCRNStreamer(m, streams=True)
    with pytest.raises(SehipError, match="chunk_frames=True"):
        DCCRNStreamer(m, chunk_frames=True)
    dev =torch.device("cuda", 0)
    with pytest.raises(SehipError, match=r"x must have shape .*\[2, 1, 300\], got \[2, 300\]"):
        check_feed_input(torch.zeros(2, 300), 2, 300, dev)
    with pytest.raises(SehipError, match="dtype torch.float32, got torch.float64"):
        check_feed_input(torch.zeros(2, 1, 300, dtype=torch.float64), 2, 300, dev)
    with pytest.raises(SehipError, match="x must be on device cuda:0.*got cpu"):
        check_feed_input(torch.zeros(2, 1, 300), 2, 300, dev)
    with pytest.raises(SehipError, match="x must be a tensor"):
        check_feed_input([0.0], 2, 300, dev)


def test_entry_points_declared_and_bound():
    from sehip import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sehip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(sehip_[a-z0-9_]+)\s*\(", text))
    lib = _lib.lib()
    for name in ENTRY_POINTS:
        assert name in declared and name in _lib.declared_symbols() and hasattr(lib, name), name


def test_entry_points_validate_before_any_hip_call():
    from sehip import _lib
    lib = _lib.lib()
    err = lambda: lib.sehip_last_error()
    one = 16          # any non-null address: the checks come before the first HIP call, nothing is dereferenced
    pick = lambda k, names: [k.get(n, d) for n, d in names]
    an = lambda **k: lib.sehip_dcs_analysis(*pick(k, (("x", one), ("carry", one), ("phase", one), ("window", one), ("S", 2), ("Kc", 3),
                                                      ("win", 400), ("hop", 100), ("spec", one), ("ring", one), ("enc", one),
                                                      ("ehist", one), ("stream", None))))
    assert an(x=None) != 0 and b"null pointer" in err()
    assert an(S=0) != 0 and b"streams" in err()
    assert an(Kc=0) != 0 and b"chunk_frames" in err()
    assert an(hop=150) != 0 and b"multiple of win_inc" in err()
    assert an(win=514, hop=257) != 0 and b"<= 512" in err()
    nh = lambda **k: lib.sehip_dcs_norm_hist(*pick(k, (("y", one), ("coef", one), ("slope", one), ("hist", one), ("phase", one), ("pos", one),
                                                       ("end", one), ("lag", 0), ("S", 2), ("Kc", 3), ("H", 1), ("F", 8), ("Cr", 8),
                                                       ("z", one), ("stream", None))))
    assert nh(hist=None) != 0 and b"null pointer" in err()
    assert nh(slope=None) != 0 and b"without a PReLU slope" in err()
    assert nh(Cr=6) != 0 and b"multiple of 4" in err()
    assert nh(H=0) != 0 and b"history rows" in err()
    assert nh(lag=7) != 0 and b"lag=7" in err()
    assert lib.sehip_dcs_lstm_carry(one, one, 2, 3, 48, None) != 0 and b"32, 64, 96 or 128" in err()
    assert lib.sehip_dcs_lstm_carry(None, one, 2, 3, 64, None) != 0 and b"null pointer" in err()
    sy = lambda **k: lib.sehip_dcs_synthesis(*pick(k, (("spec", one), ("ring", one), ("mask", one), ("window", one), ("inv", one), ("tail", one),
                                                       ("phase", one), ("pos", one), ("end", one), ("S", 2), ("Kc", 3), ("win", 400),
                                                       ("hop", 100), ("mode", 0), ("frames", one), ("out", one), ("stream", None))))
    assert sy(tail=None) != 0 and b"null pointer" in err()
    assert sy(mode=3) != 0 and b"masking mode" in err()
    assert sy(hop=30) != 0 and b"multiple of win_inc" in err()
    assert lib.sehip_dcs_mark_end(one, None, 2, 3, None) != 0 and b"null pointer" in err()
    assert lib.sehip_dcs_mark_end(one, one, 2, -1, None) != 0 and b"extra" in err()
    assert lib.sehip_dcs_advance(None, one, 2, 3, None) != 0 and b"null pointer" in err()
    assert lib.sehip_dcs_advance(one, one, 0, 3, None) != 0 and b"streams" in err()
    with pytest.raises(_lib.SehipError, match="masking mode"):
        _lib.call("sehip_dcs_synthesis", one, one, one, one, one, one, one, one, one, 2, 3, 400, 100, 5, one, one, None)
