"""CPU: chunked streaming of ConvTasNet(causal=True, norm_type='cLN') -- the restatement tests/ctn_stream_ref.py against the offline
restatement and the reference's recorded output (tests/golden/convtasnet_variants_causal_cln.npz), partial reset, the refusals of
sehip.model.ConvTasNetStreamer, state_bytes, and the sehip_ctns_* entry points (declared, bound, argument validation before any HIP
call).  No GPU calls."""
import os
import re

import pytest
import torch

import ctn_stream_ref as SR
import ctn_variants_ref as V
from util import load_golden, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(C=2, **V.FIXTURE_KW)
H = V.FIXTURE_KW["L"] // 2
ENTRY_POINTS = ("sehip_ctns_encoder", "sehip_ctns_dwconv", "sehip_ctns_decoder", "sehip_ctns_advance")


@pytest.fixture(scope="module")
def golden():
    g = load_golden("convtasnet_variants_causal_cln.npz")
    p32 = {k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd.")}
    p64 = {k: v.double() for k, v in p32.items()}
    mix = torch.from_numpy(g["mix"])
    with torch.no_grad():
        off64 = V.variants_forward(p64, mix.double(), causal=True, norm_type="cLN", **KW)
    return dict(g=g, p32=p32, p64=p64, mix=mix, off64=off64)


@pytest.mark.parametrize("Kc", [1, 3, 8, 67])
def test_restatement_equals_offline(golden, Kc):
    """Kc = 8 does not divide the 201 hops: a prefix is fed, and the network being causal, the offline output of the whole signal
    restricted to that prefix is the expected value."""
    mix, off = golden["mix"].double(), golden["off64"]
    assert mix.shape[-1] == V.FIXTURE_T == 201 * H
    with torch.no_grad():
        out, tail = SR.run_stream(lambda kc: SR.StreamRef(golden["p64"], 2, kc, **KW), mix, Kc, H)
    n = out.shape[-1]
    assert n == (201 // Kc) * Kc * H and tuple(out.shape[:3]) == (2, 2, 1) and tuple(tail.shape) == (2, 2, 1, H)
    assert float(out[..., :H].abs().max()) == 0.0                                     # the delay: exact zeros
    scale = float(off.abs().max())
    assert float((out[..., H:] - off[..., :n - H]).abs().max()) < 1e-12 * max(scale, 1.0)
    if n == V.FIXTURE_T:      # the whole signal was fed: flush is the end of the offline output
        assert float((tail - off[..., n - H:]).abs().max()) < 1e-12 * max(scale, 1.0)
        full = torch.cat([out[..., H:], tail], dim=-1)
        assert rel_err(full.float(), golden["g"]["est"]) < 2e-5                       # the reference's own fp32 output (the noise
        #                                                                               tests/test_ctn_variants_host.py allows)
    else:                     # a prefix: the tail is the second half of the last frame alone, the next frame has not been added
        assert float(tail.abs().max()) > 0.0


def test_restatement_fp32_equals_reference_output(golden):
    with torch.no_grad():
        out, tail = SR.run_stream(lambda kc: SR.StreamRef(golden["p32"], 2, kc, **KW), golden["mix"], 3, H)
    assert out.dtype == torch.float32
    assert rel_err(torch.cat([out[..., H:], tail], dim=-1), golden["g"]["est"]) < 2e-5


def test_partial_reset(golden):
    """resetting stream 1 of 2 in mid-signal: that stream continues as a fresh streamer would, stream 0 does not notice"""
    mix, Kc = golden["mix"].double(), 5
    n = Kc * H
    with torch.no_grad():
        a = SR.StreamRef(golden["p64"], 2, Kc, **KW)
        plain = SR.StreamRef(golden["p64"], 2, Kc, **KW)
        fresh = SR.StreamRef(golden["p64"], 2, Kc, **KW)
        for j in range(6):
            ya, yp = a.feed(mix[..., j * n:(j + 1) * n]), plain.feed(mix[..., j * n:(j + 1) * n])
            assert torch.equal(ya, yp)
        a.reset([1])
        for j in range(6, 12):
            ya, yp = a.feed(mix[..., j * n:(j + 1) * n]), plain.feed(mix[..., j * n:(j + 1) * n])
            yf = fresh.feed(mix[..., j * n:(j + 1) * n])
            assert torch.equal(ya[0], yp[0])
            assert float((ya[1] - yf[1]).abs().max()) < 1e-12
            assert j > 6 or not torch.equal(ya[1], yp[1])          # (the un-reset stream still carries its past there)
        mask = torch.tensor([False, True])
        a.reset(mask)
        assert a.pos.tolist() == [-1 + 12 * Kc, -1] and float(a.carry[1].abs().max()) == 0.0 and float(a.carry[0].abs().max()) > 0.0


def test_refusals_name_the_argument():
    from sehip import SehipError
    from sehip.model import ConvTasNet, ConvTasNetStreamer
    from sehip.model.conv_tasnet_stream import check_feed_input
    kw = dict(sources=["a", "b"], **V.FIXTURE_KW)
    with pytest.raises(SehipError, match="causal=False"):
        ConvTasNetStreamer(ConvTasNet(**kw, causal=False, norm_type="cLN"))
    with pytest.raises(SehipError, match="norm_type='gLN'.*statistics span the whole clip"):
        ConvTasNetStreamer(ConvTasNet(**kw, causal=True, norm_type="gLN"))
    m = ConvTasNet(**kw, causal=True, norm_type="cLN")
    with pytest.raises(SehipError, match="model is on cpu"):
        ConvTasNetStreamer(m)
    with pytest.raises(SehipError, match="streams=0"):
        ConvTasNetStreamer(m, streams=0)
    with pytest.raises(SehipError, match="chunk_frames=-1"):
        ConvTasNetStreamer(m, chunk_frames=-1)
    with pytest.raises(SehipError, match="streams=True"):
        ConvTasNetStreamer(m, streams=True)
    with pytest.raises(SehipError, match="chunk_frames=True"):
        ConvTasNetStreamer(m, chunk_frames=True)
    with pytest.raises(SehipError, match="model must be"):
        ConvTasNetStreamer(torch.nn.Linear(2, 2))
    dev = torch.device("cuda", 0)
    with pytest.raises(SehipError, match=r"x must have shape .*\[2, 1, 12\], got \[2, 1, 16\]"):
        check_feed_input(torch.zeros(2, 1, 16), 2, 1, 12, dev)
    with pytest.raises(SehipError, match="dtype torch.float32, got torch.float64"):
        check_feed_input(torch.zeros(2, 1, 12, dtype=torch.float64), 2, 1, 12, dev)
    with pytest.raises(SehipError, match="x must be on device cuda:0.*got cpu"):
        check_feed_input(torch.zeros(2, 1, 12), 2, 1, 12, dev)
    with pytest.raises(SehipError, match="x must be a tensor"):
        check_feed_input([0.0], 2, 1, 12, dev)


def test_state_bytes_formula(golden):
    from sehip.model import ConvTasNet
    from sehip.model.conv_tasnet_stream import state_bytes_of
    kw = V.FIXTURE_KW
    m = ConvTasNet(sources=["a", "b"], **kw, causal=True, norm_type="cLN")
    rows = kw["R"] * (kw["P"] - 1) * (2 ** kw["X"] - 1)                  # sum over the blocks of (P - 1) 2^x
    for S in (1, 3):
        want = S * (2 * (1 * H * 4 + rows * kw["H"] * 2 + 2 * 1 * H * 4) + 4) + 4
        assert state_bytes_of(m.cfg, S) == want == SR.StreamRef(golden["p32"], S, 4, **KW).state_bytes
    c4 = ConvTasNet(sources=["a", "b"], audio_channels=1, causal=True, norm_type="cLN")      # N=128 L=40 B=128 H=256 P=3 X=7 R=2
    assert state_bytes_of(c4.cfg, 1) == 2 * (20 * 4 + 2 * 2 * 127 * 256 * 2 + 2 * 20 * 4) + 8


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
    enc = lambda **k: lib.sehip_ctns_encoder(*[k.get(n, d) for n, d in (("x", one), ("carry", one), ("phase", one), ("U", one), ("gamma", one),
                                                                         ("beta", one), ("S", 2), ("ac", 1), ("Kc", 3), ("N", 32), ("L", 8),
                                                                         ("w", one), ("cln", one), ("stream", None))])
    assert enc(x=None) != 0 and b"null pointer" in err()
    assert enc(N=36) != 0 and b"multiple of 8" in err()
    assert enc(L=7) != 0 and b"L must be even" in err()
    assert enc(S=0) != 0 and b"streams" in err()
    assert enc(Kc=0) != 0 and b"chunk_frames" in err()
    assert enc(N=512, L=40) != 0 and b"LDS" in err()
    dw = lambda **k: lib.sehip_ctns_dwconv(*[k.get(n, d) for n, d in (("h1", one), ("hist", one), ("phase", one), ("pos", one), ("slope", one),
                                                                       ("gamma", one), ("beta", one), ("Wd", one), ("P", 3), ("dil", 1), ("S", 2),
                                                                       ("Kc", 3), ("C", 96), ("h2", one), ("stream", None))])
    assert dw(hist=None) != 0 and b"null pointer" in err()
    assert dw(C=100) != 0 and b"multiple of 8" in err()
    assert dw(C=520) != 0 and b"multiple of 8" in err()
    assert dw(P=4) != 0 and b"3, 5 or 7" in err()
    assert dw(dil=0) != 0 and b"dilation" in err()
    assert dw(Kc=0) != 0 and b"chunk_frames" in err()
    dec = lambda **k: lib.sehip_ctns_decoder(*[k.get(n, d) for n, d in (("w", one), ("mask", one), ("V", one), ("tail", one), ("phase", one),
                                                                         ("pos", one), ("S", 2), ("Kc", 3), ("N", 32), ("L", 8), ("ac", 1),
                                                                         ("Cs", 2), ("out", one), ("stream", None))])
    assert dec(tail=None) != 0 and b"null pointer" in err()
    assert dec(N=20) != 0 and b"multiple of 8" in err()
    assert dec(Cs=0) != 0 and b"bad sizes" in err()
    assert dec(N=512, L=40) != 0 and b"LDS" in err()
    assert lib.sehip_ctns_advance(None, one, 2, 3, None) != 0 and b"null pointer" in err()
    assert lib.sehip_ctns_advance(one, one, 0, 3, None) != 0 and b"streams" in err()
    with pytest.raises(_lib.SehipError, match="3, 5 or 7"):
        _lib.call("sehip_ctns_dwconv", one, one, one, one, one, one, one, one, 4, 1, 2, 3, 96, one, None)
