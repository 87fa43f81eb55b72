"""float64 restatement of ONE time step of the recurrent kernels (csrc/lstm.hip, csrc/lstm2.hip) -- TEST INFRASTRUCTURE ONLY.

The kernels store, at every step, everything the step read and wrote: h as bf16, the activated gates as bf16 records, c as fp32
records, the gate gradients dpre as bf16.  Every step can therefore be recomputed here from the operands the kernel itself read at
that step (h[t-1], c[t-1] as stored; the gate records; the stored dpre[t+1]) and nothing compounds: a stored bf16 value may differ
from the float64 result by ONE rounding, an fp32 record by its evaluation noise.  Only the cell-state gradient dc has no record; it is
carried in float64 down the reverse sweep (it is multiplied by f < 1 at every step: contractive).

Everything is in "combo form": a leading axis of C = 4 combos (combo = part * 2 + lstm: part 0 = real input, 1 = imaginary input;
lstm 0 = real_lstm, 1 = imag_lstm; src/model/dccrn.py:283-298) or C = 1 for the plain nn.LSTM of use_clstm=False.
    pre   [C, B, T, 4 H]   gate order i, f, g, o (PyTorch)          whh  [C, 4 H, H]
    h, c  [C, B, T, H]     gates [C, B, T, H, 4]                    dpre [C, B, T, 4 H]
The same functions run FREELY (feeding their own h / c / dpre forward) for tests/test_lstm_steps_host.py, which pins them against
torch.nn.LSTM, autograd and oracle.dccrn_oracle.complex_lstm.  tests/ctn_variants_ref.py is the precedent for a helper of this kind."""
import math

import torch

ULP_TOL = 2.0 ** -8 * 1.02    # worst element of a stored bf16 tensor: half an ulp at the bottom of a binade (the full-width files' figure)
RATIO_TOL = 1.1               # rms error / rms error of ONE ideal rounding of the reference.  An independent 0.1 % systematic error on top
                              # of one rounding reads sqrt(1.65^2 + 1^2) / 1.65 = 1.17; fp32 evaluation noise is 1e-3 of the rounding
ACC_TOL = 2e-5                # fp32-evaluated quantities (the c records)
# Share of elements that differ from bf16_rne(float64 result): a correctly rounding kernel differs only where its fp32 evaluation noise
# (~1e-7 relative; ~1e-7 ABSOLUTE for tanh = 1 - 2 / (1 + exp(2 x)) near zero) carries a value across a rounding boundary.  Measured on
# the clean numpy emulation of the kernels' arithmetic over every input of tests/test_gpu_lstm_steps.py
# (tests/test_lstm_steps_host.py::test_clean_emulation_passes_every_gate_and_pins_the_share): the largest share of any tensor of any case
# is SHARE_CLEAN = 1 element of the 256 of layer 2's h at (B, T) = (1, 1) -- typical tensors read 3e-5 (gates) ... 7e-4 (h of layer 2);
# the cap is twice that.
SHARE_CLEAN = 1.0 / 256
SHARE_CAP = 2 * SHARE_CLEAN
NBT = 4                       # batch rows per workgroup


def bf16_rne(x):
    """float64 -> nearest bf16 value (ties to even) as float64, in ONE rounding (through float32 it would be two)"""
    m, e = torch.frexp(x.double())
    return torch.ldexp(torch.round(m * 256.0) / 256.0, e)


# ---- record decoder ------------------------------------------------------------------------------------------------------------------
def thread_map(H):
    """(batch row in tile, unit) of each of the 4 H threads of a workgroup (csrc/lstm.hip:52-55)"""
    th = torch.arange(4 * H)
    lane, w = th & 63, th >> 6
    m, ug = lane & 15, lane >> 4
    return m & 3, 16 * w + 4 * ug + (m >> 2)


def decode_records(rec, C, B, T, H, width=1, padded=False):
    """records [C][tiles][T][4 H threads][width] -> [C, B, T, H, width] (padded: all 4 * tiles rows, the clamped ones included)"""
    tiles = (B + NBT - 1) // NBT
    bl, unit = thread_map(H)
    inv = torch.empty(NBT, H, dtype=torch.long)
    inv[bl, unit] = torch.arange(4 * H)
    r = rec.reshape(C, tiles, T, 4 * H, width)[:, :, :, inv]            # [C, tiles, T, 4, H, width]
    r = r.permute(0, 1, 3, 2, 4, 5).reshape(C, tiles * NBT, T, H, width)
    return r if padded else r[:, :B]


# ---- combo form ----------------------------------------------------------------------------------------------------------------------
def combo_split(a_r, a_i, H):
    """the per-part tensors [B, T, 2 * 4 H] (real part, imaginary part; columns lstm * 4 H + gate * H + unit) -> [4, B, T, 4 H]"""
    G = 4 * H
    return torch.stack([a_r[..., :G], a_r[..., G:], a_i[..., :G], a_i[..., G:]])


def combo_weights(w):
    """[2 lstm, ...] -> [4 combos, ...]"""
    return w[[0, 1, 0, 1]]


def combo_dh(dh_a, dh_b):
    """gradients of out_r = h[r,real] - h[i,imag] (dh_a) and out_i = h[i,real] + h[r,imag] (dh_b) -> per combo (csrc/lstm.hip:130-132)"""
    return torch.stack([dh_a, dh_b, dh_b, -dh_a])


# ---- the steps -----------------------------------------------------------------------------------------------------------------------
def cell(z, c_prev):
    """z [..., 4 H] pre-activations, c_prev [..., H] -> gates [..., H, 4], c, h"""
    zi, zf, zg, zo = z.chunk(4, -1)
    i, f, g, o = torch.sigmoid(zi), torch.sigmoid(zf), torch.tanh(zg), torch.sigmoid(zo)
    c = f * c_prev + i * g
    return torch.stack([i, f, g, o], -1), c, o * torch.tanh(c)


def _shift(a):
    """a[t - 1] along the T axis, zero at t = 0"""
    return torch.cat([torch.zeros_like(a[:, :, :1]), a[:, :, :-1]], 2)


def fwd_steps(pre, whh, h, c):
    """every step from the STORED h[t-1] (bf16 values) and c[t-1] (fp32 records): the exact gates, c[t], h[t]"""
    z = pre + torch.einsum("cbtk,cgk->cbtg", _shift(h), whh)
    return cell(z, _shift(c))


def fwd_free(pre, whh):
    """the same step, fed with its own h and c"""
    C, B, T, G = pre.shape
    h = pre.new_zeros(C, B, G // 4)
    c = h.clone()
    out = []
    for t in range(T):
        gates, c, h = cell(pre[:, :, t] + torch.einsum("cbk,cgk->cbg", h, whh), c)
        out.append((gates, c, h))
    return tuple(torch.stack(x, 2) for x in zip(*out))


def bwd_cell(gates, c, c_prev, dh, dc):
    """gates [..., H, 4] (the records the kernel re-reads), dh = incoming + recurrent, dc from step t + 1 -> dpre [..., 4 H], dc for t - 1"""
    i, f, g, o = gates.unbind(-1)
    tc = torch.tanh(c)
    dcv = dc + dh * o * (1 - tc * tc)
    dpre = torch.cat([dcv * g * i * (1 - i), dcv * c_prev * f * (1 - f), dcv * i * (1 - g * g), dh * tc * o * (1 - o)], -1)
    return dpre, dcv * f


def bwd_steps(gates, c, dh, whh, dpre_stored=None):
    """the reverse sweep.  dh [C, B, T, H]: the incoming gradient WITH the combo sign.  dpre_stored: the kernel's bf16 dpre, whose
    step t + 1 is the operand of W_hh^T at step t (None: free-running, the sweep's own)."""
    C, B, T, H = c.shape
    cp = _shift(c)
    dc = c.new_zeros(C, B, H)
    out = [None] * T
    for t in range(T - 1, -1, -1):
        dhv = dh[:, :, t]
        if t < T - 1:
            nxt = out[t + 1] if dpre_stored is None else dpre_stored[:, :, t + 1]
            dhv = dhv + torch.einsum("cbg,cgk->cbk", nxt, whh)
        out[t], dc = bwd_cell(gates[:, :, t], c[:, :, t], cp[:, :, t], dhv, dc)
    return torch.stack(out, 2)


# ---- the two stacked layers of csrc/lstm2.hip ----------------------------------------------------------------------------------------
def x2_of(h1):
    """layer 2's input from the stored h1 [4, B, T, H]: the complex combination as ONE bf16 tile per part -- the documented single
    extra rounding of csrc/lstm2.hip:9-11"""
    return bf16_rne(h1[0] - h1[3]), bf16_rne(h1[2] + h1[1])


def pre2_of(h1, wih2, bias2):
    """wih2 [2 lstm, 4 H, H] (bf16 values), bias2 [2, 4 H] fp32 = b_ih + b_hh -> layer 2's pre-gates [4, B, T, 4 H]"""
    xr, xi = x2_of(h1)
    return torch.stack([x @ wih2[l].t() + bias2[l] for x in (xr, xi) for l in (0, 1)])


def dx2_of(dpre2, wih2):
    """gradient of (x2_r, x2_i): the sum over the two lstms of W_ih2^T dpre2[t], from the STORED bf16 dpre2 [4, B, T, 4 H]"""
    return dpre2[0] @ wih2[0] + dpre2[1] @ wih2[1], dpre2[2] @ wih2[0] + dpre2[3] @ wih2[1]


# ---- gates ---------------------------------------------------------------------------------------------------------------------------
def bf16_gate(got, want64):
    """(worst element |got - want| / (|want| + 1e-3 rms(want)),  rms(got - want) / rms(bf16_rne(want) - want),  share of elements
    with got != bf16_rne(want)) and the flat index of the worst element"""
    got, want = got.double(), want64.double()
    rms = lambda a: float(a.pow(2).mean().sqrt())
    err = (got - want).abs()
    r = err / (want.abs() + 1e-3 * rms(want))
    ideal = bf16_rne(want)
    one = rms(ideal - want)
    ratio = rms(got - want) / one if one > 0 else (0.0 if float(err.max()) == 0 else math.inf)
    r = torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)
    return float(r.max()), ratio, float((got != ideal).double().mean()), int(r.argmax())


class Figures:
    """the measured figures of one case and what they violate"""

    def __init__(self, label):
        self.label, self.rows = label, []

    def bf16(self, name, got, want64):
        worst, ratio, share, at = bf16_gate(got, want64)
        self.rows.append(dict(name=name, kind="bf16", worst=worst, ratio=ratio, share=share, at=_where(at, want64.shape)))

    def f32(self, name, got, want64):
        """relative rms (the gate the c records are under) and, stricter, the worst single element over rms(want): one fp32 step is
        f * c + i * g with 1-ulp exp / rcp -- a few 1e-7 absolute on values of order 1, two orders below ACC_TOL"""
        got, want = got.double(), want64.double()
        scale = float(want.pow(2).mean().sqrt()) + 1e-300
        err = (got - want).abs()
        err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)
        self.rows.append(dict(name=name, kind="f32", rms=float(err.pow(2).mean().sqrt()) / scale, worst=float(err.max()) / scale,
                              at=_where(int(err.argmax()), want64.shape)))

    def violations(self, share_cap=None):
        cap = SHARE_CAP if share_cap is None else share_cap
        bad = []
        for r in self.rows:
            if r["kind"] == "bf16":
                checks = (("worst", ULP_TOL, False), ("ratio", RATIO_TOL, False), ("share", cap, True))
            else:
                checks = (("rms", ACC_TOL, False), ("worst", ACC_TOL, False))
            for key, tol, inclusive in checks:
                ok = r[key] <= tol if inclusive else r[key] < tol
                if not ok:
                    bad.append(f"{self.label} {r['name']}: {key} {r[key]:.3e} against {tol:.3e}, worst (combo, row, t, unit ...) {r['at']}")
        return bad

    def max_share(self):
        return max([r["share"] for r in self.rows if r["kind"] == "bf16"], default=0.0)

    def lines(self):
        out = []
        for r in self.rows:
            if r["kind"] == "bf16":
                out.append(f"{self.label} {r['name']}: worst {r['worst']:.3e} ratio {r['ratio']:.4f} share {r['share']:.2e}")
            else:
                out.append(f"{self.label} {r['name']}: c rel rms {r['rms']:.2e} worst {r['worst']:.2e}")
        return out


def _where(flat, shape):
    """(combo, row, t, unit[, gate]) of a flat index (for dpre the last entry is the column gate * H + unit)"""
    idx = []
    for n in reversed(shape):
        idx.append(flat % n)
        flat //= n
    return tuple(idx[::-1])


def check_fwd(fig, name, pre, whh, h, gates, c):
    """one recurrence, forward: the stored h / gate records / c records against every step recomputed from the stored operands"""
    wg, wc, wh = fwd_steps(pre.double(), whh.double(), h.double(), c.double())
    fig.bf16(name + "h", h, wh)
    fig.bf16(name + "gates", gates, wg)
    fig.f32(name + "c", c, wc)


def check_bwd(fig, name, gates, c, dh, whh, dpre):
    """one recurrence, backward: the stored dpre against the reverse sweep on the records, the signed dh and the stored dpre[t + 1]"""
    want = bwd_steps(gates.double(), c.double(), dh.double(), whh.double(), dpre.double())
    fig.bf16(name + "dpre", dpre, want)


def check_lstm2_fwd(fig, pre1, whh1, whh2, wih2, bias2, h1, gates1, c1, h2, gates2, c2):
    check_fwd(fig, "layer1 ", pre1, combo_weights(whh1), h1, gates1, c1)
    check_fwd(fig, "layer2 ", pre2_of(h1.double(), wih2.double(), bias2.double()), combo_weights(whh2), h2, gates2, c2)


def check_lstm2_bwd(fig, dh_a, dh_b, whh1, whh2, wih2, gates1, c1, gates2, c2, dpre1, dpre2):
    check_bwd(fig, "layer2 ", gates2, c2, combo_dh(dh_a.double(), dh_b.double()), combo_weights(whh2), dpre2)
    dxr, dxi = dx2_of(dpre2.double(), wih2.double())
    check_bwd(fig, "layer1 ", gates1, c1, combo_dh(dxr, dxi), combo_weights(whh1), dpre1)


# ---- inputs of the GPU tests (and of the CPU emulation that sets the mismatch cap) ----------------------------------------------------
LSTM_SHAPES = [(1, 1), (1, 2), (3, 7), (4, 8), (5, 9), (17, 16), (6, 17), (2, 41)]
WIDE_SHAPES = [(5, 9), (6, 17)]                     # also at hidden 32, 96, 128
RLSTM_SHAPES = [(1, 1), (5, 9), (6, 17)]            # each at hidden 32, 64, 96, 128
LSTM2_SHAPES = [(1, 1), (1, 2), (2, 3), (4, 8), (5, 9), (3, 12), (3, 13), (17, 16), (6, 25), (2, 41)]
HIDDEN = [32, 64, 96, 128]


def lstm_cases():
    """(B, T, hidden, recurrent-weight scale)"""
    return [(b, t, 64, 1.0) for b, t in LSTM_SHAPES] + [(b, t, h, 1.0) for h in (32, 96, 128) for b, t in WIDE_SHAPES] + [(5, 9, 64, 3.0)]


def rlstm_cases():
    return [(b, t, h, 1.0) for h in HIDDEN for b, t in RLSTM_SHAPES] + [(5, 9, 64, 3.0)]


def lstm2_cases():
    return [(b, t, 64, 1.0) for b, t in LSTM2_SHAPES] + [(5, 9, 64, 3.0)]


def make_inputs(B, T, H, seed, hh_scale=1.0, real=False, layers=1):
    """pre ~ N(0, 1) fp32; weights uniform in +-1/sqrt(H) as nn.LSTM initialises them (recurrent ones times hh_scale), as bf16;
    dh ~ N(0, 1) as bf16.  Complex: pre_r / pre_i [B, T, 8 H], whh [2, 4 H, H]; real: pre [B, T, 4 H], whh [1, 4 H, H]."""
    g = torch.Generator().manual_seed(seed)
    L, k, BF = (1 if real else 2), 1.0 / math.sqrt(H), torch.bfloat16
    uni = lambda *s: (torch.rand(*s, generator=g) * 2 - 1) * k
    d = dict(B=B, T=T, H=H)
    if real:
        d["pre"] = torch.randn(B, T, 4 * H, generator=g)
    else:
        d["pre_r"], d["pre_i"] = torch.randn(B, T, 8 * H, generator=g), torch.randn(B, T, 8 * H, generator=g)
    d["whh"] = (uni(L, 4 * H, H) * hh_scale).to(BF)
    d["dh_a"], d["dh_b"] = torch.randn(B, T, H, generator=g).to(BF), torch.randn(B, T, H, generator=g).to(BF)
    if layers == 2:
        d["whh2"] = (uni(L, 4 * H, H) * hh_scale).to(BF)
        d["wih2"] = uni(L, 4 * H, H).to(BF)
        d["bias2"] = uni(L, 4 * H) + uni(L, 4 * H)
    return d
