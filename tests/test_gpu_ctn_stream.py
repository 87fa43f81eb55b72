"""GPU: chunked streaming of ConvTasNet(causal=True, norm_type='cLN') -- csrc/tasnet_stream.hip and sehip.model.ConvTasNetStreamer.

Kernel level: the stream encoder and the depthwise step against the offline entry points run on carry | chunk / history | chunk, bit
for bit, with canary bands around every state buffer; the decoder against float64 on its own operands.  Whole model: the golden
mixture fed in chunks against float64 `variants_forward` and against the offline `model(mix)`, both delayed by L/2.  Bit stability
(two streamers, graph replay, S = 3 against S = 1), partial reset, flush-then-reuse, and no interference with the model's own step.

Measured on an MI355X: test_whole_model_vs_reference's docstring and DESIGN.md section 15 (whole model: 8.19e-3 from float64 against a
gate of 1.73e-2, bit-identical to the offline output; decoder: worst error / bound 0.037 ... 0.080; everything else bit-exact).
"""
import pytest
import torch

import ctn_variants_ref as V
from stream_util import Guarded, cs, lib_call, same_bits
from util import load_golden, rel_err

pytestmark = pytest.mark.gpu

ULP_TOL = 2.0 ** -8 * 1.02
FIX = V.FIXTURE_KW
H_HOP = FIX["L"] // 2


# ------------------------------------------------------------------------------------------------------------------
# 1. kernels
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,L,ac", [(32, 8, 1), (72, 10, 2), (512, 16, 1)])
def test_encoder_bit_exact(N, L, ac):
    """against sehip_ctn_encoder_fwd (its wave-per-frame kernel at these widths) on carry | chunk"""
    h, S = L // 2, 3
    g = torch.Generator().manual_seed(N + L)
    U = (0.3 * torch.randn(N, ac, L, generator=g)).cuda()
    gamma, beta = (1 + 0.2 * torch.randn(N, generator=g)).cuda(), (0.2 * torch.randn(N, generator=g)).cuda()
    for Kc in (1, 3, 13):
        for ph in (0, 1):
            carry = Guarded(torch.randn(2, S, ac, h, generator=g))
            phase = Guarded(torch.tensor([ph], dtype=torch.int32))
            x = torch.randn(S, ac, Kc * h, generator=g).cuda()
            w, cln = Guarded(torch.zeros(S, Kc, N)), Guarded(torch.zeros(S, Kc, N, dtype=torch.bfloat16))
            before = carry.t.clone()
            lib_call("sehip_ctns_encoder", x.data_ptr(), carry.t.data_ptr(), phase.t.data_ptr(), U.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                     S, ac, Kc, N, L, w.t.data_ptr(), cln.t.data_ptr(), cs())
            cat = torch.cat([before[ph], x], dim=-1).contiguous()
            w0, cln0 = torch.zeros(S, Kc, N, device="cuda"), torch.zeros(S, Kc, N, dtype=torch.bfloat16, device="cuda")
            lib_call("sehip_ctn_encoder_fwd", cat.data_ptr(), U.data_ptr(), gamma.data_ptr(), beta.data_ptr(), S, ac, (Kc + 1) * h, N, L,
                     w0.data_ptr(), cln0.data_ptr(), cs())
            torch.cuda.synchronize()
            assert same_bits(w.t, w0) and same_bits(cln.t, cln0), (Kc, ph)
            assert float(w0.abs().max()) > 0
            assert same_bits(carry.t[ph], before[ph]) and same_bits(carry.t[ph ^ 1], x[..., -h:]), (Kc, ph)
            assert carry.intact() and phase.intact() and w.intact() and cln.intact() and int(phase.t) == ph


@pytest.mark.parametrize("C,P", [(96, 3), (96, 5), (512, 3), (512, 5)])
def test_dwconv_step_bit_exact(C, P):
    """against sehip_ctn_cln_dwconv_fwd (causal) on history | chunk, cut at the row of global frame 0; C = 96: lane groups of 16 with
    four idle lanes, C = 512: a full wave; Kc below, between and above the history lengths; pos: a fresh stream (phantom frame), a
    stream whose early taps fall before frame 0, a stream far from its start"""
    S = 3
    g = torch.Generator().manual_seed(C + P)
    slope = torch.tensor([0.25], device="cuda")
    gamma, beta = (1 + 0.3 * torch.randn(C, generator=g)).cuda(), (0.3 * torch.randn(C, generator=g)).cuda()
    Wd = (0.5 * torch.randn(C, P, generator=g)).cuda()
    for dil in (1, 8):
        HR = (P - 1) * dil
        for Kc in (1, 3, 13):
            for ph in (0, 1):
                pos_l = [-1, 2, 1000]
                hist = Guarded(torch.randn(2, S, HR, C, generator=g).bfloat16())
                pos = Guarded(torch.tensor(pos_l, dtype=torch.int32))
                phase = Guarded(torch.tensor([ph], dtype=torch.int32))
                h1 = torch.randn(S, Kc, C, generator=g).bfloat16().cuda()
                h2 = Guarded(torch.full((S, Kc, C), 9.0, dtype=torch.bfloat16))
                before = hist.t.clone()
                lib_call("sehip_ctns_dwconv", h1.data_ptr(), hist.t.data_ptr(), phase.t.data_ptr(), pos.t.data_ptr(), slope.data_ptr(),
                         gamma.data_ptr(), beta.data_ptr(), Wd.data_ptr(), P, dil, S, Kc, C, h2.t.data_ptr(), cs())
                torch.cuda.synchronize()
                for s in range(S):
                    cat = torch.cat([before[ph, s], h1[s]], dim=0)                   # [HR + Kc][C]; row r is global frame pos + r - HR
                    r0 = min(max(HR - pos_l[s], 0), HR + Kc)                          # the row of global frame 0
                    want = torch.zeros(Kc, C, dtype=torch.bfloat16, device="cuda")    # frames before 0: every tap absent
                    if HR + Kc - r0 > 0:
                        src = cat[r0:].contiguous()
                        ref = torch.zeros_like(src)
                        lib_call("sehip_ctn_cln_dwconv_fwd", src.data_ptr(), slope.data_ptr(), gamma.data_ptr(), beta.data_ptr(), Wd.data_ptr(),
                                 P, dil, 1, 1, src.shape[0], C, ref.data_ptr(), cs())
                        first = max(r0, HR)                                           # first chunk row with a frame index >= 0
                        want[first - HR:] = ref[first - r0:]
                    torch.cuda.synchronize()
                    assert same_bits(h2.t[s], want), (dil, Kc, ph, s)
                    assert same_bits(hist.t[ph ^ 1, s], cat[Kc:]) and same_bits(hist.t[ph, s], before[ph, s]), (dil, Kc, ph, s)
                assert hist.intact() and pos.intact() and phase.intact() and h2.intact()
                assert pos.t.tolist() == pos_l and int(phase.t) == ph


@pytest.mark.parametrize("ac,softmax", [(1, False), (2, False), (1, True), (2, True)])
def test_decoder_vs_float64(ac, softmax):
    """every output sample = upper half of the frame before (or the tail) + lower half of its own frame, fp32 dot products of N terms:
    |error| <= (N + 2) 2^-24 sum |terms| per sample; a first call (phantom frame, zero tail) and a later one"""
    N, L, S, Kc = 32, 8, 2, 5
    Cs = 3 if softmax else 2
    h = L // 2
    g = torch.Generator().manual_seed(10 * ac + Cs)
    V_ = (0.3 * torch.randn(ac * L, N, generator=g)).cuda()
    for pos_l, ph in (([-1, -1], 0), ([4, -1], 1), ([9, 14], 1)):
        w = torch.randn(S, Kc, N, generator=g).abs().cuda()
        score = torch.randn(S, Kc, Cs * N, generator=g).bfloat16().cuda()
        mask = score
        if softmax:
            mask = torch.zeros_like(score)
            lib_call("sehip_ctn_mask_softmax_fwd", score.data_ptr(), S * Kc, Cs, N, mask.data_ptr(), cs())
        tail0 = torch.randn(2, S, Cs, ac, h, generator=g)
        for s in range(S):
            if pos_l[s] < 0:
                tail0[:, s] = 0
        tail = Guarded(tail0)
        pos, phase = Guarded(torch.tensor(pos_l, dtype=torch.int32)), Guarded(torch.tensor([ph], dtype=torch.int32))
        out = Guarded(torch.full((S, Cs, ac, Kc * h), float("nan")))
        before = tail.t.clone()
        lib_call("sehip_ctns_decoder", w.data_ptr(), mask.data_ptr(), V_.data_ptr(), tail.t.data_ptr(), phase.t.data_ptr(), pos.t.data_ptr(),
                 S, Kc, N, L, ac, Cs, out.t.data_ptr(), cs())
        torch.cuda.synchronize()
        valid = torch.tensor([[float(p + i >= 0) for i in range(Kc)] for p in pos_l], dtype=torch.float64, device="cuda")
        m64 = mask.double().clamp(min=0).view(S, Kc, Cs, N)
        sw = w.double()[:, :, None, :] * m64 * valid[:, :, None, None]                       # [S, Kc, Cs, N]
        terms = sw[:, :, :, None, :] * V_.double()[None, None, None]                         # [S, Kc, Cs, ac*L, N]
        fr = terms.sum(-1).view(S, Kc, Cs, ac, L).permute(0, 2, 3, 1, 4)                     # [S, Cs, ac, Kc, L]
        mag = terms.abs().sum(-1).view(S, Kc, Cs, ac, L).permute(0, 2, 3, 1, 4)
        t64 = before[ph].double()
        prev = torch.cat([t64.unsqueeze(3), fr[..., :-1, h:]], dim=3)
        pmag = torch.cat([t64.abs().unsqueeze(3), mag[..., :-1, h:]], dim=3)
        want = (prev + fr[..., :h]).reshape(S, Cs, ac, Kc * h)
        bound = (N + 2) * 2.0 ** -24 * (pmag + mag[..., :h]).reshape(S, Cs, ac, Kc * h)
        err = (out.t.double() - want).abs()
        assert not bool(torch.isnan(out.t).any())
        print(f"ctns_decoder ac={ac} softmax={softmax} pos={pos_l}: worst error / bound {float((err / (bound + 1e-300)).max()):.3f}")
        assert bool((err <= bound).all()), (pos_l, float((err - bound).max()))
        terr = (tail.t[ph ^ 1].double() - fr[..., -1, h:]).abs()
        assert bool((terr <= (N + 2) * 2.0 ** -24 * mag[..., -1, h:]).all())
        assert same_bits(tail.t[ph], before[ph])
        for s in range(S):
            if pos_l[s] == -1:                      # first call: the phantom frame adds nothing
                assert same_bits(out.t[s, ..., :h], torch.zeros_like(out.t[s, ..., :h]))
        assert tail.intact() and pos.intact() and phase.intact() and out.intact()


def test_advance():
    pos, phase = Guarded(torch.tensor([-1, 7, 300] * 100, dtype=torch.int32)), Guarded(torch.tensor([0], dtype=torch.int32))
    for k in (1, 2):
        lib_call("sehip_ctns_advance", pos.t.data_ptr(), phase.t.data_ptr(), 300, 13, cs())
        torch.cuda.synchronize()
        assert pos.t.tolist() == [-1 + 13 * k, 7 + 13 * k, 300 + 13 * k] * 100 and int(phase.t) == k & 1
    assert pos.intact() and phase.intact()


# ------------------------------------------------------------------------------------------------------------------
# 2. whole model
# ------------------------------------------------------------------------------------------------------------------
_CACHE = {}


def fixture():
    """the golden model on the GPU, its mixture, float64 `variants_forward`, the offline model(mix) and sim_dev -- computed once"""
    if not _CACHE:
        from sehip.model import ConvTasNet
        g = load_golden("convtasnet_variants_causal_cln.npz")
        sd = {k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd.")}
        model = ConvTasNet(sources=["None", "None"], **FIX, causal=True, norm_type="cLN")
        model.load_state_dict(sd)
        model = model.cuda().train()
        mix = torch.from_numpy(g["mix"])
        kw = dict(C=2, causal=True, norm_type="cLN", **FIX)
        with torch.no_grad():
            ref64 = V.variants_forward({k: v.double() for k, v in sd.items()}, mix.double(), **kw)
            sim = V.variants_forward(sd, mix, sim=V.Bf16Sim, **kw)
            offline = model(mix.cuda()).cpu()
        _CACHE.update(model=model, mix=mix, ref64=ref64, offline=offline, sim_dev=rel_err(sim, ref64))
    return _CACHE


def stream_all(st, mix):
    """feeds mix [S, ac, T] in whole chunks -> (concatenated outputs, flush) on the CPU"""
    n = st.chunk_samples
    outs = [st.feed(mix[..., j * n:(j + 1) * n].contiguous()) for j in range(mix.shape[-1] // n)]
    return torch.cat(outs, dim=-1).cpu(), st.flush().cpu()


@pytest.mark.parametrize("Kc", [1, 3, 8, 67])
def test_whole_model_vs_reference(Kc):
    """Gate (as test_whole_chain_vs_reference_vectors reasons): the relative L2 deviation from float64 `variants_forward`, and from the
    offline `model(mix)` delayed by h, is below 2 x sim_dev, the deviation of the bf16-storage restatement computed here.
    Measured on an MI355X: sim_dev 8.637e-3 (gate 1.727e-2); vs float64 8.194e-3 (Kc = 1, 3, 67), 8.195e-3 (Kc = 8, a prefix of 200
    frames); vs offline 0 at every Kc (bit-identical); the offline output itself is 8.194e-3 from float64."""
    from sehip.model import ConvTasNetStreamer
    f = fixture()
    st = ConvTasNetStreamer(f["model"], streams=2, chunk_frames=Kc)
    assert st.delay == H_HOP
    out, tail = stream_all(st, f["mix"].cuda())
    n = out.shape[-1]
    assert n == (201 // Kc) * Kc * H_HOP and float(out[..., :H_HOP].abs().max()) == 0.0
    got = out[..., H_HOP:]
    if n == V.FIXTURE_T:
        got = torch.cat([got, tail], dim=-1)
    m = got.shape[-1]
    e_ref, e_off = rel_err(got, f["ref64"][..., :m]), rel_err(got, f["offline"][..., :m])
    print(f"ConvTasNetStreamer Kc={Kc}: vs float64 {e_ref:.3e}, vs offline model(mix) {e_off:.3e}; sim_dev {f['sim_dev']:.3e} "
          f"(offline vs float64 {rel_err(f['offline'], f['ref64']):.3e})")
    assert e_ref < 2 * f["sim_dev"] and e_off < 2 * f["sim_dev"]


def signals(S, frames, seed=5):
    g = torch.Generator().manual_seed(seed)
    return (0.3 * torch.randn(S, 1, frames * H_HOP, generator=g)).cuda()


def test_two_streamers_and_graph_replay_are_bit_identical():
    from sehip.model import ConvTasNetStreamer
    model, Kc = fixture()["model"], 5
    x = signals(2, 6 * Kc)
    a, b = ConvTasNetStreamer(model, 2, Kc), ConvTasNetStreamer(model, 2, Kc)
    gr = ConvTasNetStreamer(model, 2, Kc, graph=True)
    (ya, ta), (yb, tb), (yg, tg) = stream_all(a, x), stream_all(b, x), stream_all(gr, x)
    assert float(ya.abs().max()) > 0 and same_bits(ya, yb) and same_bits(ta, tb)
    assert same_bits(ya, yg) and same_bits(ta, tg)
    yg2, tg2 = stream_all(gr, x)                    # after the flush: the captured chunk again, from a fresh state
    assert same_bits(ya, yg2) and same_bits(ta, tg2)


def test_stream_of_three_equals_stream_alone():
    """products are row-independent at equal Kc: stream s of S = 3 is the same signal alone at S = 1, bit for bit"""
    from sehip.model import ConvTasNetStreamer
    model, Kc = fixture()["model"], 4
    x = signals(3, 8 * Kc, seed=6)
    y3, t3 = stream_all(ConvTasNetStreamer(model, 3, Kc), x)
    for s in range(3):
        y1, t1 = stream_all(ConvTasNetStreamer(model, 1, Kc), x[s:s + 1].contiguous())
        assert same_bits(y3[s:s + 1], y1) and same_bits(t3[s:s + 1], t1), s


def test_partial_reset_and_flush_then_reuse():
    from sehip.model import ConvTasNetStreamer
    model, Kc = fixture()["model"], 3
    n = Kc * H_HOP
    x = signals(2, 12 * Kc, seed=7)
    a, plain, fresh = (ConvTasNetStreamer(model, 2, Kc) for _ in range(3))
    for j in range(6):
        assert same_bits(a.feed(x[..., j * n:(j + 1) * n].contiguous()), plain.feed(x[..., j * n:(j + 1) * n].contiguous()))
    a.reset(torch.tensor([False, True]))
    assert a.pos.tolist() == [6 * Kc - 1, -1]
    for j in range(6, 12):
        c = x[..., j * n:(j + 1) * n].contiguous()
        ya, yp, yf = a.feed(c), plain.feed(c), fresh.feed(c)
        assert same_bits(ya[0], yp[0]) and same_bits(ya[1], yf[1]), j
        assert j > 6 or not same_bits(ya[1], yp[1])
    a.reset([0])
    assert a.pos.tolist() == [-1, 6 * Kc - 1]
    # flush, then the same signal again: what a fresh streamer gives
    assert float(plain.flush().abs().max()) > 0 and plain.pos.tolist() == [-1, -1]
    y1, t1 = stream_all(plain, x)
    y2, t2 = stream_all(ConvTasNetStreamer(model, 2, Kc), x)
    assert same_bits(y1, y2) and same_bits(t1, t2) and float(t1.abs().max()) > 0


def test_feed_refusals_and_state_bytes_on_device():
    from sehip import SehipError
    from sehip.model import ConvTasNetStreamer
    from sehip.model.conv_tasnet_stream import state_bytes_of
    model = fixture()["model"]
    st = ConvTasNetStreamer(model, streams=2, chunk_frames=3)
    held = sum(t.numel() * t.element_size() for t in [st.pos, st.phase, st.carry, st.tail] + st.hist)
    assert st.state_bytes == state_bytes_of(model.cfg, 2) == held
    with pytest.raises(SehipError, match="x must have shape"):
        st.feed(torch.zeros(2, 1, 16, device="cuda"))
    with pytest.raises(SehipError, match="dtype torch.float32"):
        st.feed(torch.zeros(2, 1, 12, device="cuda", dtype=torch.float64))
    with pytest.raises(SehipError, match="x must be on device"):
        st.feed(torch.zeros(2, 1, 12))
    assert st.pos.tolist() == [-1, -1]


def private_model(mask="relu"):
    """a model with the fixture's parameters that a test may change or move (the shared one stays as it is)"""
    from sehip.model import ConvTasNet
    model = ConvTasNet(sources=["None", "None"], **FIX, causal=True, norm_type="cLN", mask_nonlinear=mask)
    model.load_state_dict(fixture()["model"].state_dict())
    return model.cuda()


@pytest.mark.parametrize("mask", ["relu", "softmax"])
def test_capture_in_mid_clip_and_launch_count(mask):
    """A graphed streamer whose graph is dropped after three chunks (the model's flat storage is re-created, so _sync_model packs the
    weights again and forgets the captured chain) captures again with streams in mid-clip: the eager pass before the capture must
    leave pos, phase, carry, history and tail as they were, so every later chunk and the flush have the bits of an eager streamer fed
    the same clip.  Both count the 4 R X + 5 launches of a chunk (+ 1 with the softmax mask)."""
    from sehip.model import ConvTasNetStreamer
    S, Kc, n = 2, 3, 3 * H_HOP
    model = private_model(mask)
    x = signals(S, 8 * Kc, seed=11)
    eager, gr = ConvTasNetStreamer(model, S, Kc), ConvTasNetStreamer(model, S, Kc, graph=True)
    assert eager.launches == gr.launches == 0
    want, tail = stream_all(eager, x)
    for j in range(8):
        if j == 3:
            first, epoch = gr._graph, model.storage_epoch
            model.cuda()
            assert first is not None and model.storage_epoch != epoch
        assert same_bits(gr.feed(x[..., j * n:(j + 1) * n].contiguous()), want[..., j * n:(j + 1) * n]), j
    assert gr._graph is not None and gr._graph is not first
    assert same_bits(gr.flush(), tail) and float(tail.abs().max()) > 0
    assert eager.launches == gr.launches == 4 * FIX["R"] * FIX["X"] + 5 + (mask == "softmax")


def test_refresh_weights_follows_the_parameters():
    """the product weights are packed at construction and on refresh_weights(), not per chunk"""
    from sehip.model import ConvTasNetStreamer
    model = private_model()
    x = signals(1, 8, seed=8)
    st = ConvTasNetStreamer(model, 1, 8)
    y0 = st.feed(x).clone()
    st.reset()
    with torch.no_grad():
        model.separator.network[1].weight.mul_(0.5)          # the bottleneck product's weight
    y1 = st.feed(x).clone()
    st.reset()
    assert same_bits(y0, y1)                                 # still the packed copy
    st.refresh_weights()
    y2 = st.feed(x).clone()
    assert not same_bits(y0, y2)
    st2 = ConvTasNetStreamer(model, 1, 8)
    assert same_bits(st2.feed(x), y2)


def test_no_interference_with_the_models_own_step():
    """model(x), and one training step's gradients, with a streamer feeding between forward and backward: the same bits"""
    from sehip.model import ConvTasNetStreamer
    f = fixture()
    model, mix = f["model"], f["mix"].cuda()
    G = torch.from_numpy(load_golden("convtasnet_variants_causal_cln.npz")["G"]).cuda()

    def step(streamer):
        model.zero_grad(set_to_none=True)
        est = model(mix)
        keep = est.detach().clone()
        if streamer is not None:
            streamer.feed(signals(2, streamer.chunk_frames, seed=9))
        est.backward(G)
        torch.cuda.synchronize()
        return keep, model.flat_grads.detach().clone()

    from sehip.utils import set_deterministic
    set_deterministic(True)          # (the schedule in which two steps of the model have the same bits in the first place)
    try:
        e0, g0 = step(None)
        st = ConvTasNetStreamer(model, 2, 7)
        st.feed(signals(2, 7, seed=10))
        e1, g1 = step(st)
        e2, g2 = step(None)
    finally:
        set_deterministic(False)
    assert same_bits(e0, e1) and same_bits(g0, g1) and same_bits(e0, e2) and same_bits(g0, g2)
    assert float(g0.abs().max()) > 0
