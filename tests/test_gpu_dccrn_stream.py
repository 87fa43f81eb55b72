"""GPU: chunked streaming of DCCRN -- csrc/dccrn_stream.hip and sehip.model.DCCRNStreamer.

Kernel level: the analysis against float64 on its own operands and, bit for bit, against sehip_stft_fwd on carry | chunk; the
normalise-with-history launch bit for bit against sehip_cbn_apply and against copies; the carried-state recurrence (sehip_lstm_fwd_chunk
on Kc + 1 steps + sehip_dcs_lstm_carry) bit for bit against sehip_lstm_fwd; the synthesis against float64 on its own operands, with the
`end` mark.  Whole model: 21 hops fed in chunks against the float64 oracle (gate: twice the Bf16Sim oracle's own deviation) and, recorded,
against the offline model.eval()(x) delayed by D.  Bit stability (two streamers, graph replay, S = 3 against S = 1, partial reset,
flush-then-reuse) and no interference with the model's own train step.  Canary bands around the state buffers of the kernel tests.

Measured on an MI355X: analysis worst 3.9e-8 .. 5.8e-8 of the absolute addends (bound 2.98e-6), synthesis
5.2e-8 .. 8.4e-8 (bound 5.78e-6); whole model 2.095e-3 from float64 for every Kc (sim_dev 2.073e-3, gate 4.146e-3), flush tail alone
1.466e-3 (gate 2.817e-3), 2.216e-4 from the offline HIP output (not bit-identical: the offline plan's convolutions run on other kernels
of the engine); everything else bit-exact.
"""
import pytest
import torch

import dccrn_stream_ref as SR
import frontend_ref as FR
from oracle import dccrn_oracle as O
from stream_util import Guarded, cs, lib_call, same_bits
from util import rel_err

pytestmark = pytest.mark.gpu

GEOMETRIES = [(400, 100), (320, 160), (512, 128)]
LA = 6
NO_END = 2 ** 31 - 1
# operation counts (roundings along the path of one addend), each times 2^-24 of the sum of the absolute addends:
#   analysis: 1 window product + 9 butterfly additions + 10 complex twiddle products of 3 roundings + 10 rounded twiddle constants
FFT_OPS = 50
#   synthesis: the mask (mode E: two square roots, tanh, four divisions, the products: <= 16), the inverse transform (FFT_OPS), the two
#   correction sums over the frame (tree sums, depth 9 + 6, + 5 for combining them), window and scale (3), R + 1 additions of the
#   overlap-add, the reciprocal window energy and its product (2)
SYN_OPS = 16 + FFT_OPS + 20 + 3 + 6 + 2


# ------------------------------------------------------------------------------------------------------------------
# 1. kernels
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("win,hop", GEOMETRIES)
@pytest.mark.parametrize("S", [1, 3])
def test_analysis_kernel(win, hop, S):
    """Frames k of carry | chunk: every bin within FFT_OPS 2^-24 sum_n |x_n w_n| of float64 on the same operands; the spectrum and the
    bf16 encoder rows bit-identical to sehip_stft_fwd's rows of carry | chunk (the transform, the window product and the packing are
    shared device code: frame k of the chunk is frame k + R - 1 of that signal, whose zero padding it never touches); the next carry
    is the last win - hop samples bit for bit, the next ring the last 6 rows of ring | chunk, row 0 of the encoder input the carried
    row; the current halves and the canary bands are intact.  Kc below, at and above the ring depth, both phases, a fresh stream (zero
    carry) and a later call."""
    pad, R = win - hop, win // hop
    g = torch.Generator().manual_seed(win + S)
    window = torch.from_numpy(FR.ops.window_of("hann", win)).cuda()
    w64 = window.double().cpu()
    worst = 0.0
    for Kc in (1, 3, 13):
        for ph in (0, 1):
            for fresh in (True, False):
                carry = Guarded(torch.zeros(2, S, pad) if fresh else torch.randn(2, S, pad, generator=g))
                ring = Guarded(torch.randn(2, S, LA, 257, 2, generator=g))
                ehist = Guarded(torch.randn(2, S, 256, 2, generator=g).bfloat16())
                phase = Guarded(torch.tensor([ph], dtype=torch.int32))
                x = torch.randn(S, Kc * hop, generator=g).cuda()
                spec, enc = Guarded(torch.zeros(S, Kc, 257, 2)), Guarded(torch.zeros(S, 1 + Kc, 256, 2, dtype=torch.bfloat16))
                c0, r0, e0 = carry.t.clone(), ring.t.clone(), ehist.t.clone()
                lib_call("sehip_dcs_analysis", x.data_ptr(), carry.ptr, phase.ptr, window.data_ptr(), S, Kc, win, hop, spec.ptr, ring.ptr,
                         enc.ptr, ehist.ptr, cs())
                cat = torch.cat([c0[ph], x], -1).contiguous()                      # [S][pad + Kc hop]
                T = FR.frames_of(cat.shape[-1], win, hop)
                sp0 = torch.zeros(S, T, 257, 2, device="cuda")
                en0 = torch.zeros(S, T, 256, 2, dtype=torch.bfloat16, device="cuda")
                lib_call("sehip_stft_fwd", cat.data_ptr(), window.data_ptr(), S, cat.shape[-1], win, hop, 512, sp0.data_ptr(), en0.data_ptr(), cs())
                torch.cuda.synchronize()
                key = (Kc, ph, fresh)
                assert same_bits(spec.t, sp0[:, R - 1:R - 1 + Kc]) and same_bits(enc.t[:, 1:], en0[:, R - 1:R - 1 + Kc]), key
                fr = cat.double().cpu().unfold(-1, win, hop) * w64                   # [S][Kc][win]
                a, _, _ = FR.bases(win)
                want = FR._bins((cat.double().cpu().unfold(-1, win, hop)) @ a.t())
                add = fr.abs().sum(-1)[..., None, None]
                err = float(((spec.t.double().cpu() - want).abs() / (add + 1e-30)).max())
                worst = max(worst, err)
                assert err < FFT_OPS * 2.0 ** -24, (key, err)
                assert same_bits(carry.t[ph ^ 1], cat[:, -pad:]) and same_bits(carry.t[ph], c0[ph]), key
                rows = torch.cat([r0[ph], spec.t], 1)
                assert same_bits(ring.t[ph ^ 1], rows[:, -LA:]) and same_bits(ring.t[ph], r0[ph]), key
                assert same_bits(enc.t[:, 0], e0[ph]) and same_bits(ehist.t[ph ^ 1], enc.t[:, -1]) and same_bits(ehist.t[ph], e0[ph]), key
                assert all(b.intact() for b in (carry, ring, ehist, phase, spec, enc)) and int(phase.t) == ph
    print(f"analysis {win}/{hop} S={S}: worst error {worst:.2e} of the absolute addends (bound {FFT_OPS * 2.0 ** -24:.2e})")


@pytest.mark.parametrize("Cr,F,H", [(8, 8, 6), (8, 128, 1), (32, 4, 1), (128, 4, 2)])
def test_norm_hist_kernel(Cr, F, H):
    """chunk rows bit-identical to sehip_cbn_apply on the same rows; history rows and the next history bit-identical copies; Kc below and
    above the history depth; a row at or past `end` is a zero row; coef = NULL copies"""
    S = 3
    g = torch.Generator().manual_seed(Cr + F + H)
    coef = torch.randn(Cr, 16, generator=g).cuda()
    slope = torch.tensor([0.2], device="cuda")
    for Kc in (1, 13):
        for ph in (0, 1):
            for lag, identity in ((0, False), (3, False), (0, True)):
                pos_l, end_l = [0, 7, 40], [NO_END, 7 + Kc // 2 - lag, NO_END]      # stream 1: the chunk rows from Kc // 2 on are absent
                hist = Guarded(torch.randn(2, S, H, F, 2 * Cr, generator=g).bfloat16())
                pos, end = Guarded(torch.tensor(pos_l, dtype=torch.int32)), Guarded(torch.tensor(end_l, dtype=torch.int32))
                phase = Guarded(torch.tensor([ph], dtype=torch.int32))
                y = torch.randn(S, Kc, F, 2 * Cr, generator=g).bfloat16().cuda()
                z = Guarded(torch.full((S, H + Kc, F, 2 * Cr), 9.0, dtype=torch.bfloat16))
                h0 = hist.t.clone()
                lib_call("sehip_dcs_norm_hist", y.data_ptr(), None if identity else coef.data_ptr(), None if identity else slope.data_ptr(),
                         hist.ptr, phase.ptr, pos.ptr, end.ptr, lag, S, Kc, H, F, Cr, z.ptr, cs())
                want = y.clone()
                if not identity:
                    lib_call("sehip_cbn_apply", y.data_ptr(), coef.data_ptr(), slope.data_ptr(), S * Kc * F, Cr, want.data_ptr(), cs())
                torch.cuda.synchronize()
                for k in range(Kc):
                    if pos_l[1] + k - lag >= end_l[1]:
                        want[1, k] = 0
                assert Kc == 1 or float(want[1, -1].abs().max()) == 0.0
                key = (Kc, ph, lag, identity)
                assert same_bits(z.t[:, H:], want) and same_bits(z.t[:, :H], h0[ph]), key
                assert same_bits(hist.t[ph ^ 1], z.t[:, -H:]) and same_bits(hist.t[ph], h0[ph]), key
                assert all(b.intact() for b in (hist, pos, end, phase, z)) and pos.t.tolist() == pos_l and int(phase.t) == ph


@pytest.mark.parametrize("H", [32, 64])
@pytest.mark.parametrize("B", [1, 5])
def test_recurrence_with_carried_state(H, B):
    """T = 12 steps split 1 + 4 + 7, each part as the streamer runs it (sehip_lstm_fwd_chunk over steps [1, Kc + 1) of Kc + 1-step buffers
    whose step 0 is the carried state, then sehip_dcs_lstm_carry): the bits of sehip_lstm_fwd over T = 12.  B = 5: a ragged batch tile."""
    T, Bp = 12, (B + 3) // 4 * 4
    g = torch.Generator().manual_seed(H + B)
    pre = [(0.5 * torch.randn(B, T, 8 * H, generator=g)).cuda() for _ in range(2)]
    whh = (torch.randn(2, 4 * H, H, generator=g) / H ** 0.5).bfloat16().cuda()
    h0 = torch.zeros(4, B, T, H, dtype=torch.bfloat16, device="cuda")
    g0 = torch.zeros(4, Bp, T, 4 * H, dtype=torch.bfloat16, device="cuda")
    c0 = torch.zeros(4, Bp, T, H, device="cuda")
    lib_call("sehip_lstm_fwd", pre[0].data_ptr(), pre[1].data_ptr(), whh.data_ptr(), B, T, H, h0.data_ptr(), g0.data_ptr(), c0.data_ptr(), cs())
    hc = cc = None
    t0 = 0
    for Kc in (1, 4, 7):
        h = Guarded(torch.zeros(4, B, Kc + 1, H, dtype=torch.bfloat16))
        c = Guarded(torch.zeros(4, Bp, Kc + 1, H))
        gt = torch.zeros(4, Bp, Kc + 1, 4 * H, dtype=torch.bfloat16, device="cuda")
        if hc is not None:               # the state carried into this part: step 0 of its buffers
            h.t[:, :, 0] = hc
            c.t.view(4, Bp // 4, Kc + 1, 4 * H)[:, :, 0] = cc
        p = [torch.zeros(B, Kc + 1, 8 * H, device="cuda") for _ in range(2)]
        for q in range(2):
            p[q][:, 1:] = pre[q][:, t0:t0 + Kc]
        lib_call("sehip_lstm_fwd_chunk", p[0].data_ptr(), p[1].data_ptr(), whh.data_ptr(), B, Kc + 1, H, 1, Kc + 1, h.ptr, gt.data_ptr(), c.ptr, cs())
        torch.cuda.synchronize()
        assert same_bits(h.t[:, :, 1:], h0[:, :, t0:t0 + Kc]), (Kc, "h")
        lib_call("sehip_dcs_lstm_carry", h.ptr, c.ptr, B, Kc, H, cs())
        torch.cuda.synchronize()
        hc, cc = h.t[:, :, 0].clone(), c.t.view(4, Bp // 4, Kc + 1, 4 * H)[:, :, 0].clone()
        assert same_bits(hc, h0[:, :, t0 + Kc - 1]) and same_bits(cc, c0.view(4, Bp // 4, T, 4 * H)[:, :, t0 + Kc - 1]), (Kc, "carry")
        assert h.intact() and c.intact()
        t0 += Kc
    assert float(h0.float().abs().max()) > 0.05


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("win,hop", [(400, 100), (320, 160)])
def test_synthesis_kernel(mode, win, hop):
    """Every output sample against float64 on the same operands (spectrum rows of ring | chunk, masks, the fp32 window and reciprocal
    window energy, the carried tail): |error| <= SYN_OPS 2^-24 of the sum of the absolute addends, where a frame's sample n has the
    addends w[n] / 256 * sum_k (|er_k| + |ei_k|) (1 + 2 win / (512 + win)) (the transform's terms and the rank-2 correction's).  A first
    call (pos 0: every frame has a negative index: zeros, and the tail stays zero), a call whose first blocks have a negative index, a
    later call, and a call under the `end` mark: frames >= end add nothing."""
    from sehip import ops
    S, Kc, pad, R = 3, 5, win - hop, win // hop
    g = torch.Generator().manual_seed(win + mode)
    window = torch.from_numpy(ops.window_of("hann", win)).cuda()
    inv = torch.from_numpy(ops.inv_window_energy(win, hop, 2 * R, hop, "hann")).cuda()
    _, syn, _ = FR.bases(win)
    worst = 0.0
    for pos_l, end_l, ph in (([0, 0, 0], [NO_END] * 3, 0), ([4, 8, 11], [NO_END] * 3, 1), ([40, 41, 42], [NO_END, 37, 36], 0)):
        first = pos_l == [0, 0, 0]
        tail = Guarded(torch.zeros(2, S, pad) if first else 0.1 * torch.randn(2, S, pad, generator=g))
        ring = Guarded(torch.randn(2, S, LA, 257, 2, generator=g))
        pos, end = Guarded(torch.tensor(pos_l, dtype=torch.int32)), Guarded(torch.tensor(end_l, dtype=torch.int32))
        phase = Guarded(torch.tensor([ph], dtype=torch.int32))
        spec = torch.randn(S, Kc, 257, 2, generator=g).cuda()
        mask = (0.7 * torch.randn(S, Kc, 256, 2, generator=g)).cuda()
        frames, out = Guarded(torch.zeros(S, Kc, win)), Guarded(torch.full((S, Kc * hop), 7.0))
        t0 = tail.t.clone()
        lib_call("sehip_dcs_synthesis", spec.data_ptr(), ring.ptr, mask.data_ptr(), window.data_ptr(), inv.data_ptr(), tail.ptr, phase.ptr,
                 pos.ptr, end.ptr, S, Kc, win, hop, mode, frames.ptr, out.ptr, cs())
        torch.cuda.synchronize()
        rows = torch.cat([ring.t[ph], spec], 1)[:, :Kc].double().cpu()                  # spectrum of frame pos - 6 + k
        est = FR.apply_mask(rows, mask.double().cpu(), mode)                            # [S][Kc][514]
        fr64 = est @ syn                                                                # [S][Kc][win]
        mag = (est[..., 1:257].abs().sum(-1) + est[..., 258:].abs().sum(-1)) / 256.0 * (1 + 2 * win / (512 + win))
        add_fr = mag[..., None] * window.double().cpu()
        acc = torch.cat([t0[ph].double().cpu(), torch.zeros(S, Kc * hop, dtype=torch.float64)], 1)
        add = acc.abs()
        for s in range(S):
            for k in range(Kc):
                f = pos_l[s] - LA + k
                if 0 <= f < end_l[s]:
                    acc[s, k * hop:k * hop + win] += fr64[s, k]
                    add[s, k * hop:k * hop + win] += add_fr[s, k]
        i64 = inv.double().cpu().repeat(Kc)
        want, wadd = acc[:, :Kc * hop] * i64, add[:, :Kc * hop] * i64
        for s in range(S):
            for k in range(Kc):
                if pos_l[s] - LA - (R - 1) + k < 0:
                    want[s, k * hop:(k + 1) * hop] = 0
                    assert float(out.t[s, k * hop:(k + 1) * hop].abs().max()) == 0.0      # exact zeros before the delay has passed
        err = float(((out.t.double().cpu() - want.clamp(-1, 1)).abs() / (wadd + 1e-30)).max())
        terr = float(((tail.t[ph ^ 1].double().cpu() - acc[:, Kc * hop:]).abs() / (add[:, Kc * hop:] + 1e-30)).max())
        worst = max(worst, err, terr)
        assert err < SYN_OPS * 2.0 ** -24 and terr < SYN_OPS * 2.0 ** -24, (pos_l, err, terr)
        if first:
            assert float(out.t.abs().max()) == 0.0 and float(tail.t.abs().max()) == 0.0
        else:
            assert float(out.t.abs().max()) > 1e-3
        if end_l[1] != NO_END:           # stream 2: every frame of the chunk is >= end: nothing is added, the next tail is empty
            assert Kc * hop >= pad and float(tail.t[ph ^ 1, 2].abs().max()) == 0.0 and float(frames.t[2].abs().max()) == 0.0
            assert float(out.t[2, pad:].abs().max()) == 0.0 and float(out.t[2, :pad].abs().max()) > 0.0
        assert same_bits(tail.t[ph], t0[ph])
        assert all(b.intact() for b in (tail, ring, pos, end, phase, frames, out)) and pos.t.tolist() == pos_l
    print(f"synthesis mode {mode} {win}/{hop}: worst error {worst:.2e} of the absolute addends (bound {SYN_OPS * 2.0 ** -24:.2e})")


def test_advance_and_mark_end():
    pos, end = Guarded(torch.tensor([0, 5, 9], dtype=torch.int32)), Guarded(torch.full((3,), NO_END, dtype=torch.int32))
    phase = Guarded(torch.tensor([1], dtype=torch.int32))
    lib_call("sehip_dcs_mark_end", pos.ptr, end.ptr, 3, 3, cs())
    lib_call("sehip_dcs_advance", pos.ptr, phase.ptr, 3, 7, cs())
    torch.cuda.synchronize()
    assert pos.t.tolist() == [7, 12, 16] and end.t.tolist() == [3, 8, 12] and int(phase.t) == 0
    assert pos.intact() and end.intact() and phase.intact()


# ------------------------------------------------------------------------------------------------------------------
# 2. whole model
# ------------------------------------------------------------------------------------------------------------------
HOPS = 21
_CASE = {}


def case(geo=(400, 100), mode="E", widths=(16,) * 6, use_cbn=True, S=2, rnn=(2, 128)):
    """(model kwargs, oracle cfg, parameters, signals, float64 oracle output, sim_dev over the clip, sim_dev over the last D samples):
    computed once per configuration, shared, never written"""
    key = (geo, mode, widths, use_cbn, S, rnn)
    if key not in _CASE:
        kw = dict(rnn_layers=rnn[0], rnn_units=rnn[1], win_len=geo[0], win_inc=geo[1], kernel_num=list(widths), masking_mode=mode, use_cbn=use_cbn,
                  length=HOPS * geo[1])
        cfg = O.DCCRNConfig(**kw)
        p = SR.make_params(cfg)
        g = torch.Generator().manual_seed(11)
        n = HOPS * geo[1]
        t = torch.arange(n, dtype=torch.float32)
        x = torch.stack([0.1 * torch.randn(n, generator=g) + 0.2 * torch.sin((0.01 + 0.013 * s) * t) for s in range(S)])[:, None]
        D = SR.delay_of(*geo)
        with torch.no_grad():
            p64 = {k: (v.double() if v.is_floating_point() else v) for k, v in p.items()}
            torch.set_default_dtype(torch.float64)          # (the oracle builds its overlap-add identity in the default dtype)
            try:
                want = O.dccrn_forward(p64, x.double(), cfg, training=False, bases=SR.bases64(cfg))
            finally:
                torch.set_default_dtype(torch.float32)
            sim = O.dccrn_forward(p, x, cfg, training=False, sim=O.Bf16Sim)
        _CASE[key] = (kw, cfg, p, x, want, rel_err(sim, want), rel_err(sim[..., -D:], want[..., -D:]))
    return _CASE[key]


def build(kw, p):
    from sehip.model import DCCRN
    m = DCCRN(**kw)
    missing = m.load_state_dict(p, strict=False)
    assert all(k.startswith(("stft.", "istft.")) for k in missing.missing_keys) and not missing.unexpected_keys
    return m.cuda().eval()


def stream_all(st, x, flush=True):
    n = st.chunk_samples
    outs = [st.feed(x[..., j * n:(j + 1) * n].contiguous()) for j in range(x.shape[-1] // n)]
    return torch.cat(outs, -1), (st.flush() if flush else None)


@pytest.mark.parametrize("Kc", [1, 3, 7, 21])
def test_whole_model_vs_float64(Kc):
    """cat(feeds)[..., D:] + flush against the float64 oracle (NoSim, training=False): relative L2 deviation <= 2 sim_dev, sim_dev the
    Bf16Sim oracle's own deviation from float64 (computed here); the flush tail alone meets the same gate over the last D samples, so a
    wrong tail cannot hide in the clip's norm; the first D samples are exact zeros.  Recorded: the deviation from the offline HIP
    model.eval()(x) delayed by D (the offline plan runs its convolutions on other kernels of the engine, whose choice depends on the
    geometry and the row count, so bit identity is not asserted)."""
    from sehip.model import DCCRNStreamer
    kw, cfg, p, x, want, sim_dev, sim_tail = case()
    model = build(kw, p)
    st = DCCRNStreamer(model, streams=2, chunk_frames=Kc)
    out, tail = stream_all(st, x.cuda())
    D = st.delay
    assert D == 900 and tuple(out.shape) == (2, 1, HOPS * 100) and tuple(tail.shape) == (2, 1, D)
    assert float(out[..., :D].abs().max()) == 0.0
    full = torch.cat([out[..., D:], tail], -1).cpu()
    dev, tdev = rel_err(full, want), rel_err(tail.cpu(), want[..., -D:])
    with torch.no_grad():
        off = model(x.cuda()).cpu()
    odev = rel_err(full, off)
    print(f"Kc {Kc}: stream vs float64 {dev:.3e} (sim_dev {sim_dev:.3e}, gate {2 * sim_dev:.3e}); tail {tdev:.3e} (sim {sim_tail:.3e}, "
          f"gate {2 * sim_tail:.3e}); vs offline HIP {odev:.3e} (offline vs float64 {rel_err(off, want):.3e}); {st.launches} launches per chunk")
    assert dev <= 2 * sim_dev and tdev <= 2 * sim_tail
    assert st.pos.tolist() == [0, 0] and st.end.tolist() == [NO_END] * 2              # flush resets


@pytest.mark.parametrize("geo,mode,widths,use_cbn,rnn", [((320, 160), "C", (16,) * 6, True, (2, 128)), ((512, 128), "R", (16,) * 6, True, (2, 128)),
                                                         ((400, 100), "E", (16, 16, 32, 32, 64, 64), False, (2, 128)),
                                                         ((400, 100), "E", (16,) * 6, True, (3, 64)), ((400, 100), "E", (16,) * 6, True, (1, 192))])
def test_whole_model_other_configurations(geo, mode, widths, use_cbn, rnn):
    """the other frame geometries and masking modes, wider layers, the real BatchNorm (use_cbn=False), three LSTM layers of hidden size 32
    and one of 96: the same gates, Kc = 3"""
    from sehip.model import DCCRNStreamer
    kw, cfg, p, x, want, sim_dev, sim_tail = case(geo, mode, widths, use_cbn, rnn=rnn)
    st = DCCRNStreamer(build(kw, p), streams=2, chunk_frames=3)
    out, tail = stream_all(st, x.cuda())
    D = st.delay
    assert float(out[..., :D].abs().max()) == 0.0
    dev = rel_err(torch.cat([out[..., D:], tail], -1).cpu(), want)
    tdev = rel_err(tail.cpu(), want[..., -D:])
    print(f"{geo} {mode} {widths} cbn={use_cbn} rnn={rnn}: stream vs float64 {dev:.3e} (gate {2 * sim_dev:.3e}); tail {tdev:.3e} (gate {2 * sim_tail:.3e})")
    assert dev <= 2 * sim_dev and tdev <= 2 * sim_tail


# ------------------------------------------------------------------------------------------------------------------
# 3. bit stability, no interference
# ------------------------------------------------------------------------------------------------------------------
def test_bit_stability():
    """two streamers; graph replay against eager, also after a flush; stream s of S = 3 against S = 1; Kc = 7 against Kc = 3; partial reset
    and flush-then-reuse against fresh streamers (the engine's kernel choice does not depend on the row count at these widths)"""
    from sehip.model import DCCRNStreamer
    kw, cfg, p, x, _, _, _ = case(S=3)
    model = build(kw, p)
    xc = x.cuda()
    a, b = DCCRNStreamer(model, streams=3, chunk_frames=3), DCCRNStreamer(model, streams=3, chunk_frames=3)
    oa, ta = stream_all(a, xc)
    ob, tb = stream_all(b, xc)
    assert same_bits(oa, ob) and same_bits(ta, tb)
    gr = DCCRNStreamer(model, streams=3, chunk_frames=3, graph=True)
    og, tg = stream_all(gr, xc)
    assert same_bits(og, oa) and same_bits(tg, ta)
    og2, tg2 = stream_all(gr, xc)                                                      # after a flush: the same clip again
    oa2, ta2 = stream_all(a, xc)                                                       # flush-then-reuse against the first pass
    assert same_bits(og2, oa) and same_bits(tg2, ta) and same_bits(oa2, oa) and same_bits(ta2, ta)
    for s in range(3):
        one = DCCRNStreamer(model, streams=1, chunk_frames=3)
        o1, t1 = stream_all(one, xc[s:s + 1])
        assert same_bits(o1, oa[s:s + 1]) and same_bits(t1, ta[s:s + 1]), s
    o7, t7 = stream_all(DCCRNStreamer(model, streams=3, chunk_frames=7), xc)           # another chunk size: the same bits at these widths
    assert same_bits(o7, oa) and same_bits(t7, ta)
    # partial reset: streams 0 and 2 restart in mid-clip and equal fresh streams; stream 1 does not notice
    n = a.chunk_samples
    for j in range(3):
        a.feed(xc[..., j * n:(j + 1) * n].contiguous())
    a.reset([0, 2])
    fresh = DCCRNStreamer(model, streams=3, chunk_frames=3)
    for j in range(3, 7):
        ya = a.feed(xc[..., j * n:(j + 1) * n].contiguous())
        yf = fresh.feed(xc[..., j * n:(j + 1) * n].contiguous())
        assert same_bits(ya[0], yf[0]) and same_bits(ya[2], yf[2]) and same_bits(ya[1], oa[1, :, j * n:(j + 1) * n]), j
    assert a.pos.tolist() == [12, 21, 12]
    a.reset(torch.tensor([True, True, True]))
    assert a.pos.tolist() == [0, 0, 0]


def test_capture_in_mid_clip_and_launch_count():
    """A graphed streamer whose graph is dropped after three chunks (the model's flat storage is re-created, so _sync_model derives the
    weights again and forgets the captured chain) captures again with streams in mid-clip: the eager pass before the capture must leave
    every state tensor as it was, so every later chunk and the flush have the bits of an eager streamer fed the same clip.  Launches
    per chunk: 36 + 4 per LSTM layer, the values of the streamer before ChunkStreamer counted them."""
    from sehip.model import DCCRN, DCCRNStreamer
    kw, cfg, p, x, _, _, _ = case()
    model, xc, n = build(kw, p), x.cuda(), 300
    eager, gr = DCCRNStreamer(model, streams=2, chunk_frames=3), DCCRNStreamer(model, streams=2, chunk_frames=3, graph=True)
    assert eager.launches == gr.launches == 0
    want, tail = stream_all(eager, xc)
    for j in range(HOPS // 3):
        if j == 3:
            first, epoch = gr._graph, model.storage_epoch
            model.cuda()
            assert first is not None and model.storage_epoch != epoch
        assert same_bits(gr.feed(xc[..., j * n:(j + 1) * n].contiguous()), want[..., j * n:(j + 1) * n]), j
    assert gr._graph is not None and gr._graph is not first
    assert same_bits(gr.flush(), tail) and float(tail.abs().max()) > 0
    assert eager.launches == gr.launches == 44
    for layers, launches in ((1, 40), (3, 48)):
        st = DCCRNStreamer(DCCRN(**dict(kw, rnn_layers=layers)).cuda().eval(), streams=2, chunk_frames=3)
        st.feed(xc[..., :n].contiguous())
        assert st.launches == launches, layers


def test_no_interference_with_the_models_own_step():
    """model(x) in train mode and the gradients of a deterministic step are bit-identical with a streamer feeding between forward and
    backward; running statistics and num_batches_tracked are unchanged by feed / flush; refresh_weights() follows in-place changes"""
    from sehip._lib import call
    from sehip.model import DCCRNStreamer
    kw, cfg, p, x, _, _, _ = case()
    xc = x.cuda()
    call("sehip_set_deterministic", 1)
    try:
        def step(with_stream):
            model = build(kw, p).set_deterministic(True).train()
            st = DCCRNStreamer(model, streams=2, chunk_frames=3) if with_stream else None
            y = model(xc)
            if st is not None:
                st.feed(xc[..., :300].contiguous())
            y.pow(2).mean().backward()
            if st is not None:
                st.feed(xc[..., 300:600].contiguous())
            torch.cuda.synchronize()
            return y.detach().clone(), model.flat_grads.clone(), model._bflat.clone(), model._nbt.clone(), model, st
        y0, g0, b0, n0, _, _ = step(False)
        y1, g1, b1, n1, model, st = step(True)
    finally:
        call("sehip_set_deterministic", 0)
    assert same_bits(y0, y1) and same_bits(g0, g1) and same_bits(b0, b1) and torch.equal(n0, n1)
    assert float(g0.abs().max()) > 0 and int(n1.max()) == 1
    st.flush()
    assert same_bits(model._bflat, b1) and torch.equal(model._nbt, n1)
    # in-place parameter change: after refresh_weights() the streamer computes what a new streamer computes (the packed weights, biases
    # and BatchNorm records are the streamer's own copies; the PReLU slopes are read in place)
    model.eval()
    st2 = DCCRNStreamer(model, streams=2, chunk_frames=3)
    before, _ = stream_all(st2, xc, flush=False)
    st2.reset()
    with torch.no_grad():
        model.flat_params.mul_(1.01)
    st2.refresh_weights()
    after, _ = stream_all(st2, xc, flush=False)
    fresh, _ = stream_all(DCCRNStreamer(model, streams=2, chunk_frames=3), xc, flush=False)
    assert not same_bits(after, before) and same_bits(after, fresh)
