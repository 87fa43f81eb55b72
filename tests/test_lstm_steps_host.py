"""CPU: the float64 step reference of tests/lstm_steps_ref.py against torch.nn.LSTM / autograd / the DCCRN oracle, its record decoder
against a brute-force index table, and the evidence that the gates of tests/test_gpu_lstm_steps.py separate a correct kernel from a
subtly wrong one: a numpy emulation of the kernels' arithmetic (fp32 accumulation, 1 / (1 + exp(-x)) and 1 - 2 / (1 + exp(2 x)) in fp32,
bf16 round-to-nearest-even at the stored points; csrc/lstm.hip, csrc/lstm2.hip) passes every gate on every input of the GPU tests, and
each of seven planted faults fails at least one at (B, T) = (5, 17)."""
import numpy as np
import pytest
import torch

import lstm_steps_ref as R

D = torch.float64


# ---- the reference against torch ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [32, 64])
@pytest.mark.parametrize("T", [1, 2, 9])
def test_free_running_reference_equals_nn_lstm_and_autograd(H, T):
    B, I = 3, 5
    torch.manual_seed(7 + H + T)
    lstm = torch.nn.LSTM(I, H).double()
    x = torch.randn(T, B, I, dtype=D, requires_grad=True)
    pre = (x @ lstm.weight_ih_l0.t() + lstm.bias_ih_l0 + lstm.bias_hh_l0).transpose(0, 1)      # [B, T, 4 H]
    # the same graph as nn.LSTM's, built from `pre`, so that autograd also yields d loss / d pre
    y, _ = lstm(x)
    whh = lstm.weight_hh_l0.detach()[None]
    gates, c, h = R.fwd_free(pre.detach()[None], whh)
    assert (h[0].transpose(0, 1) - y.detach()).abs().max() < 1e-10
    dy = torch.randn(T, B, H, dtype=D)
    (dx,) = torch.autograd.grad(y, x, dy, retain_graph=True)
    dpre = R.bwd_steps(gates, c, dy.transpose(0, 1)[None], whh)[0]                            # [B, T, 4 H]
    assert (dpre.transpose(0, 1) @ lstm.weight_ih_l0.detach() - dx).abs().max() < 1e-10       # input gradient
    # the implied dpre itself: autograd through the explicit recurrence
    p = pre.detach().clone().requires_grad_(True)
    hh, cc, outs = torch.zeros(B, H, dtype=D), torch.zeros(B, H, dtype=D), []
    for t in range(T):
        _, cc, hh = R.cell(p[:, t] + hh @ whh[0].t(), cc)
        outs.append(hh)
    (dp,) = torch.autograd.grad(torch.stack(outs, 0), p, dy)
    assert (torch.stack(outs, 0) - y.detach()).abs().max() < 1e-10
    assert (dpre - dp).abs().max() < 1e-10
    # and recomputed step by step from its own (exact) records the reference reproduces itself
    g2, c2, h2 = R.fwd_steps(pre.detach()[None], whh, h, c)
    assert (g2 - gates).abs().max() < 1e-12 and (c2 - c).abs().max() < 1e-12 and (h2 - h).abs().max() < 1e-12
    assert (R.bwd_steps(gates, c, dy.transpose(0, 1)[None], whh, dpre[None]) - dpre[None]).abs().max() < 1e-12


def test_complex_wiring_and_signs_equal_the_oracle_for_two_stacked_layers():
    from oracle.dccrn_oracle import complex_lstm
    B, T, H = 3, 6, 32
    g = torch.Generator().manual_seed(5)
    p = {}
    for layer, I in ((0, 10), (1, H)):
        for which in ("real_lstm", "imag_lstm"):
            q = f"l{layer}.{which}."
            p[q + "weight_ih_l0"] = torch.randn(4 * H, I, generator=g, dtype=D) * 0.3
            p[q + "weight_hh_l0"] = torch.randn(4 * H, H, generator=g, dtype=D) * 0.3
            p[q + "bias_ih_l0"] = torch.randn(4 * H, generator=g, dtype=D) * 0.1
            p[q + "bias_hh_l0"] = torch.randn(4 * H, generator=g, dtype=D) * 0.1
    xr = torch.randn(T, B, 10, generator=g, dtype=D, requires_grad=True)
    xi = torch.randn(T, B, 10, generator=g, dtype=D, requires_grad=True)
    m_r, m_i = complex_lstm(xr, xi, p, "l0.", False)
    o_r, o_i = complex_lstm(m_r, m_i, p, "l1.", False)
    stack = lambda layer, key: torch.stack([p[f"l{layer}.{w}.{key}"] for w in ("real_lstm", "imag_lstm")])
    wih1, whh1, wih2, whh2 = stack(0, "weight_ih_l0"), stack(0, "weight_hh_l0"), stack(1, "weight_ih_l0"), stack(1, "weight_hh_l0")
    b1 = stack(0, "bias_ih_l0") + stack(0, "bias_hh_l0")
    bias2 = stack(1, "bias_ih_l0") + stack(1, "bias_hh_l0")
    bt = lambda a: a.detach().transpose(0, 1)
    pre_r = torch.cat([bt(xr) @ wih1[l].t() + b1[l] for l in (0, 1)], -1)        # [B, T, 8 H]: columns lstm * 4 H + gate * H + unit
    pre_i = torch.cat([bt(xi) @ wih1[l].t() + b1[l] for l in (0, 1)], -1)
    g1, c1, h1 = R.fwd_free(R.combo_split(pre_r, pre_i, H), R.combo_weights(whh1))
    # (x2 without its bf16 rounding: the wiring is what is compared here)
    pre2 = torch.stack([x @ wih2[l].t() + bias2[l] for x in (h1[0] - h1[3], h1[2] + h1[1]) for l in (0, 1)])
    g2, c2, h2 = R.fwd_free(pre2, R.combo_weights(whh2))
    assert (h1[0] - h1[3] - bt(m_r)).abs().max() < 1e-10 and (h1[2] + h1[1] - bt(m_i)).abs().max() < 1e-10
    assert (h2[0] - h2[3] - bt(o_r)).abs().max() < 1e-10 and (h2[2] + h2[1] - bt(o_i)).abs().max() < 1e-10
    # pre2_of is the same wiring with the rounding: within one bf16 rounding of x2
    xr2, xi2 = R.x2_of(h1)
    assert ((xr2 - (h1[0] - h1[3])).abs() <= 2.0 ** -8 * (h1[0] - h1[3]).abs()).all()
    assert torch.equal(R.pre2_of(h1, wih2, bias2)[3], xi2 @ wih2[1].t() + bias2[1])
    # backward: the sign table through both layers
    da, db = torch.randn(T, B, H, generator=g, dtype=D), torch.randn(T, B, H, generator=g, dtype=D)
    gxr, gxi = torch.autograd.grad([o_r, o_i], [xr, xi], [da, db])
    dpre2 = R.bwd_steps(g2, c2, R.combo_dh(bt(da), bt(db)), R.combo_weights(whh2))
    dpre1 = R.bwd_steps(g1, c1, R.combo_dh(*R.dx2_of(dpre2, wih2)), R.combo_weights(whh1))
    assert (dpre1[0] @ wih1[0] + dpre1[1] @ wih1[1] - bt(gxr)).abs().max() < 1e-10
    assert (dpre1[2] @ wih1[0] + dpre1[3] @ wih1[1] - bt(gxi)).abs().max() < 1e-10


@pytest.mark.parametrize("H", R.HIDDEN)
def test_record_decoder_against_a_brute_force_index_table(H):
    C, B, T = 2, 6, 3
    tiles = 2
    rec = torch.arange(C * tiles * T * 4 * H * 4, dtype=torch.int64).reshape(C, tiles, T, 4 * H, 4)
    got = R.decode_records(rec.flatten(), C, B, T, H, width=4, padded=True)
    want = torch.full((C, tiles * 4, T, H, 4), -1, dtype=torch.int64)
    for combo in range(C):
        for tile in range(tiles):
            for w in range(H // 16):
                for lane in range(64):
                    m, ug = lane & 15, lane >> 4
                    bl, rs = m & 3, m >> 2
                    unit = 16 * w + 4 * ug + rs
                    assert (want[combo, tile * 4 + bl, :, unit] == -1).all()         # every (row, unit) pair exactly once
                    want[combo, tile * 4 + bl, :, unit] = rec[combo, tile, :, 64 * w + lane]
    assert (want >= 0).all() and torch.equal(got, want)
    assert torch.equal(R.decode_records(rec.flatten(), C, B, T, H, width=4), want[:, :B])


def test_bf16_rne_is_one_rounding_to_nearest_even():
    x = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -40, -0.3, 0.0, 3e-5], dtype=D)
    want = torch.tensor([1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -0.30078125, 0.0, float(torch.tensor(3e-5).bfloat16())], dtype=D)
    assert torch.equal(R.bf16_rne(x), want)
    y = torch.randn(4096, dtype=torch.float32)
    assert torch.equal(R.bf16_rne(y.double()), y.bfloat16().double())     # float32 inputs: torch's own conversion


# ---- numpy emulation of the kernels' arithmetic ----------------------------------------------------------------------------------------
F = np.float32


def bf16_np(x):
    u = np.ascontiguousarray(x, dtype=F).view(np.uint32)
    return ((u + (((u >> 16) & 1) + 0x7FFF)) & 0xFFFF0000).astype(np.uint32).view(F)


def sig(x):
    return F(1) / (F(1) + np.exp(-x))


def tnh(x):
    return F(1) - F(2) / (F(1) + np.exp(F(2) * x))


def emu_fwd(pre, whh, fault=None, true_B=None):
    """pre [C, B, T, 4 H], whh [C, 4 H, H] fp32 (bf16 values) -> h (bf16 values), gates (bf16 values), c fp32"""
    C, B, T, G = pre.shape
    H = G // 4
    h, c = np.zeros((C, B, H), F), np.zeros((C, B, H), F)
    hs, gs, cs = [], [], []
    whhT = np.ascontiguousarray(whh.transpose(0, 2, 1))
    with np.errstate(over="ignore"):
        for t in range(T):
            hp = hs[t - 2] if (fault == "h_from_t-2" and t == T // 2) else h
            z = pre[:, :, t] + np.matmul(hp, whhT)
            zi, zf, zg, zo = (z[..., k * H:(k + 1) * H].copy() for k in range(4))
            if fault == "f_g_swapped":
                zf[1], zg[1] = zg[1].copy(), zf[1].copy()
            i, f, g, o = sig(zi), sig(zf), tnh(zg), sig(zo)
            c = f * c + i * g
            h = bf16_np(o * tnh(c))
            if fault == "row_B-1_into_B-2":          # one workgroup (combo 2, the last tile) writes its clamped row one row too low
                h[2, B - 2] = h[2, B - 1]
            hs.append(h)
            gs.append(bf16_np(np.stack([i, f, g, o], -1)))
            cs.append(c)
    return np.stack(hs, 2), np.stack(gs, 2), np.stack(cs, 2)


def emu_bwd(gates, c, dh, whh, fault=None):
    """gates [C, B, T, H, 4] / c [C, B, T, H]: the forward's records; dh fp32 WITH the combo sign -> dpre (bf16 values) [C, B, T, 4 H]"""
    C, B, T, H = c.shape
    dc, rec = np.zeros((C, B, H), F), np.zeros((C, B, H), F)
    out = [None] * T
    with np.errstate(over="ignore"):
        for t in range(T - 1, -1, -1):
            i, f, g, o = (gates[:, :, t, :, k] for k in range(4))
            ct = c[:, :, t]
            cp = c[:, :, t - 1] if t > 0 else np.zeros_like(ct)
            if fault == "c[t]_for_c[t-1]":
                cp = ct
            dhv = dh[:, :, t] + rec
            tc = tnh(ct)
            d_o = dhv * tc
            dcv = dc + dhv * o * (F(1) - tc * tc)
            out[t] = bf16_np(np.concatenate([dcv * g * i * (F(1) - i), dcv * cp * f * (F(1) - f), dcv * i * (F(1) - g * g),
                                             d_o * o * (F(1) - o)], -1))
            dc = dcv * f
            rec = np.matmul(out[t], whh)
    return np.stack(out, 2)


def n_(t):
    return t.float().numpy()


def t_(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


def np_combo_dh(a, b, drop_sign=False):
    return np.stack([a, b, b, a if drop_sign else -a])


def emulate_lstm(d, real, fault=None):
    """the single-layer kernels on make_inputs(...): Figures of the forward and the backward"""
    H = d["H"]
    if real:
        pre, whh, dh = d["pre"][None], d["whh"], d["dh_a"][None]
    else:
        pre, whh, dh = R.combo_split(d["pre_r"], d["pre_i"], H), R.combo_weights(d["whh"]), R.combo_dh(d["dh_a"].float(), d["dh_b"].float())
    w_used = n_(whh).copy()
    if fault == "whh_row_x1.003":                    # unit 5 of one lstm (two combos), all four gates
        for k in range(4):
            w_used[1::2, k * H + 5] = bf16_np(w_used[1::2, k * H + 5]) * F(1.003)
    h, gates, c = emu_fwd(n_(pre), w_used, fault)
    dh_used = n_(dh)
    if fault == "combo_3_sign_dropped":
        dh_used = np_combo_dh(n_(d["dh_a"]), n_(d["dh_b"]), drop_sign=True)
    dpre = emu_bwd(gates, c, dh_used, w_used, fault)
    fig = R.Figures(f"B={d['B']} T={d['T']} H={H}")
    R.check_fwd(fig, "", pre, whh.double(), t_(h), t_(gates), t_(c))
    R.check_bwd(fig, "", t_(gates), t_(c), dh, whh.double(), t_(dpre))
    return fig


def emulate_lstm2(d, fault=None):
    H = d["H"]
    pre1 = R.combo_split(d["pre_r"], d["pre_i"], H)
    w1, w2, wi = n_(R.combo_weights(d["whh"])), n_(R.combo_weights(d["whh2"])), n_(d["wih2"])
    h1, g1, c1 = emu_fwd(n_(pre1), w1)
    x = [bf16_np(h1[0] - h1[3]), bf16_np(h1[2] + h1[1])]
    if fault == "layer2_reads_h1[t-1]":
        t = d["T"] // 2
        x = [np.concatenate([a[:, :t], a[:, t - 1:t], a[:, t + 1:]], 1) for a in x]
    b2 = n_(d["bias2"])
    pre2 = np.stack([np.matmul(x[part], wi[l].T) + b2[l] for part in (0, 1) for l in (0, 1)])
    h2, g2, c2 = emu_fwd(pre2, w2)
    dpre2 = emu_bwd(g2, c2, np_combo_dh(n_(d["dh_a"]), n_(d["dh_b"])), w2)
    dxr = np.matmul(dpre2[0], wi[0]) + np.matmul(dpre2[1], wi[1])
    dxi = np.matmul(dpre2[2], wi[0]) + np.matmul(dpre2[3], wi[1])
    dpre1 = emu_bwd(g1, c1, np_combo_dh(dxr, dxi), w1)
    fig = R.Figures(f"B={d['B']} T={d['T']}")
    R.check_lstm2_fwd(fig, pre1, d["whh"], d["whh2"], d["wih2"], d["bias2"], t_(h1), t_(g1), t_(c1), t_(h2), t_(g2), t_(c2))
    R.check_lstm2_bwd(fig, d["dh_a"], d["dh_b"], d["whh"], d["whh2"], d["wih2"], t_(g1), t_(c1), t_(g2), t_(c2), t_(dpre1), t_(dpre2))
    return fig


def clean_figures():
    """the emulation on every input of tests/test_gpu_lstm_steps.py (same seeds)"""
    figs = []
    for n, (B, T, H, s) in enumerate(R.lstm_cases()):
        figs.append(emulate_lstm(R.make_inputs(B, T, H, 100 + n, hh_scale=s), real=False))
    for n, (B, T, H, s) in enumerate(R.rlstm_cases()):
        figs.append(emulate_lstm(R.make_inputs(B, T, H, 200 + n, hh_scale=s, real=True), real=True))
    for n, (B, T, H, s) in enumerate(R.lstm2_cases()):
        for rep in range(2):
            figs.append(emulate_lstm2(R.make_inputs(B, T, H, 300 + 2 * n + rep, hh_scale=s, layers=2)))
    return figs


def test_clean_emulation_passes_every_gate_and_pins_the_share():
    figs = clean_figures()
    share = max(f.max_share() for f in figs)
    ratio = max(r["ratio"] for f in figs for r in f.rows if r["kind"] == "bf16")
    worst = max(r["worst"] for f in figs for r in f.rows if r["kind"] == "bf16")
    cacc = max(r["worst"] for f in figs for r in f.rows if r["kind"] == "f32")
    print(f"clean emulation, {len(figs)} cases: largest mismatch share {share:.6e} (cap {2 * share:.6e}), largest ratio {ratio:.4f}, "
          f"worst element {worst:.3e}, worst c element {cacc:.2e}")
    bad = [v for f in figs for v in f.violations()]
    assert not bad, "\n".join(bad)
    # the numbers written in lstm_steps_ref.py are the ones measured here
    assert R.SHARE_CLEAN == pytest.approx(share, rel=1e-3) and R.SHARE_CAP == 2 * R.SHARE_CLEAN


FAULTS = ["h_from_t-2", "f_g_swapped", "whh_row_x1.003", "row_B-1_into_B-2", "combo_3_sign_dropped", "c[t]_for_c[t-1]",
          "layer2_reads_h1[t-1]"]


@pytest.mark.parametrize("fault", FAULTS)
def test_planted_fault_fails_a_gate(fault):
    B, T, H = 5, 17, 64
    if fault == "layer2_reads_h1[t-1]":
        clean, broken = emulate_lstm2(R.make_inputs(B, T, H, 77, layers=2)), emulate_lstm2(R.make_inputs(B, T, H, 77, layers=2), fault)
    else:
        clean, broken = emulate_lstm(R.make_inputs(B, T, H, 77), False), emulate_lstm(R.make_inputs(B, T, H, 77), False, fault)
    assert not clean.violations(), clean.violations()
    bad = broken.violations()
    print(fault, "->", len(bad), "violations;", bad[0] if bad else None)
    assert bad, f"{fault} passed every gate:\n" + "\n".join(broken.lines())
