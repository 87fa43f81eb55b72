"""CPU: tests/desc_ref.py -- the float64 restatement of sehip_gemm_desc that tests/test_gpu_dccrn_products.py judges every DCCRN
product launch with -- proved before it judges a kernel: against the oracle's float64 convolutions and autograd at the headline widths
(oracle/dccrn_oracle.py: complex_conv2d, complex_deconv2d + complex_cat, complex_batchnorm + PReLU), the w_tiled order against the
plan's table builder, and the GPU test's gates against subtly wrong results (a dropped last frame, a tap shifted by one row, a 0.1 %
systematic error, one row missing from a fused sum) -- so that a green GPU run means something.  No GPU, nothing of libsehip."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import desc_ref as D
from oracle import dccrn_oracle as O
import dccrn_products_worker as W          # the GPU test's own gates (importing the module needs no GPU)
from dccrn_products_worker import F32_TOL

KW = dict(kernel_num=[16, 32, 64, 128, 256, 256], rnn_units=128, length=1200)
B, T = 2, 7
TOL = 1e-9
F64 = torch.float64


def rel(a, b):
    return float((a - b).norm() / (b.norm() + 1e-300))


@pytest.fixture(scope="module")
def ctx():
    from sehip import plan
    st = plan.DCCRNStatic(plan.DCCRNConfig(**KW))
    p = O.init_params(O.DCCRNConfig(**KW), seed=1)
    g = torch.Generator().manual_seed(2)
    for k in p:
        if k.endswith(".bias"):
            p[k] = 0.1 * torch.randn(p[k].shape, generator=g)
    p = {k: v.double() if v.is_floating_point() else v for k, v in p.items()}
    flat = torch.zeros(st.layout.n_params, dtype=F64)
    for name in st.layout.param_names:
        off, shape = st.layout.param_off[name]
        flat[off:off + p[name].numel()] = p[name].reshape(-1)
    kn = st.cfg.kernel_num
    geom = {"enc_in": (T, 256, 2), "mask": (T, 256, 2), "dmask": (T, 256, 2)}
    for i in range(6):
        for nm in ("y", "z", "dye", "dskip", "dz"):
            geom[f"{nm}{i}"] = (T, 256 >> (i + 1), kn[i + 1])
    for nm in ("P", "dP", "dz5l"):
        geom[nm] = (T, 4, kn[6])
    for j in range(5):
        idx = 6 - j
        for nm in ("yd", "zd", "dyd", "dzd"):
            geom[f"{nm}{j}"] = (T + 1, (256 >> idx) * 2, kn[idx - 1])
    return dict(st=st, p=p, flat=flat, g=g, geom=geom)


def cl(x):
    return x.detach().permute(0, 3, 2, 1).contiguous()      # [B,C,F,T] -> [B,T,F,C]


def rnd(ctx, *shape):
    return torch.randn(*shape, generator=ctx["g"], dtype=F64)


def product(ctx, name, bufs, ktab_edit=None, a_edit=None):
    """(tables, A, out) of one spec evaluated by desc_ref on CPU tensors bufs[name] = [B, Tst, F, C] float64"""
    st, spec = ctx["st"], ctx["st"].specs[name]
    g = D.from_spec(st, spec, ctx["geom"], B, T)
    if ktab_edit is not None:
        g["ktab"] = ktab_edit(g["ktab"].clone(), g)
    srcs = [(bufs[nm].reshape(-1),) + geo for (nm, _), geo in zip(spec.srcs, g["srcs"])]
    A = D.gather_A(srcs, g["ktab"], g["M"], g["K"], g["TT"], g["J"], g["fmul"])
    if a_edit is not None:
        A = a_edit(A, g)
    out = A @ D.plan_weights(spec, ctx["flat"])[:spec.N].t()
    bias = D.expected_bias(spec, ctx["flat"])
    if bias is not None:
        out = out + bias[None, :spec.N]
    return g, A, out


def scatter(ctx, name, g, out, into):
    """adds the product's columns into the destination tensors into[buffer name] (zeros elsewhere: parities add up)"""
    spec = ctx["st"].specs[name]
    for q, (cols, _, idx) in D.dst_index(g["dsts"], g["ntab"], g["M"], g["N"], g["Npad"], g["TT"], g["J"]).items():
        into[spec.dsts[q][0]].view(-1)[idx] += out[:, cols]


def conv_params(ctx, pre):
    p = ctx["p"]
    return [p[pre + "0.real_conv.weight"], p[pre + "0.real_conv.bias"], p[pre + "0.imag_conv.weight"], p[pre + "0.imag_conv.bias"]]


# ---- convolutions against the oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [0, 3])
def test_encoder_forward(ctx, i):
    """enc0.fwd reads the 2-channel spectrum through NARROW chunks (4 rows x 2 channels, `coff` valid rows); enc3.fwd is the first
    layer whose columns are re-ordered for the fused statistics' tiles"""
    kn = ctx["st"].cfg.kernel_num
    x = rnd(ctx, B, kn[i], 256 >> i, T)
    ref = O.complex_conv2d(x, *conv_params(ctx, f"encoder.{i}."))
    g, _, out = product(ctx, f"enc{i}.fwd", {"enc_in" if i == 0 else f"z{i - 1}": cl(x)})
    into = {f"y{i}": torch.zeros(B, *ctx["geom"][f"y{i}"], dtype=F64)}
    scatter(ctx, f"enc{i}.fwd", g, out, into)
    assert rel(into[f"y{i}"], cl(ref)) < TOL


def test_encoder_input_gradient_pair_with_residual(ctx):
    """enc2.dg0 / dg1: the two output-row parities of the input gradient, each adding the skip gradient `res` to its own rows"""
    i = 2
    kn = ctx["st"].cfg.kernel_num
    x = rnd(ctx, B, kn[i], 256 >> i, T).requires_grad_(True)
    y = O.complex_conv2d(x, *conv_params(ctx, f"encoder.{i}."))
    dy = rnd(ctx, *y.shape)
    (dx,) = torch.autograd.grad((y * dy).sum(), x)
    res = rnd(ctx, B, *ctx["geom"][f"dskip{i - 1}"])
    into = {f"dz{i - 1}": torch.zeros(B, *ctx["geom"][f"dz{i - 1}"], dtype=F64)}
    for par in (0, 1):
        name = f"enc{i}.dg{par}"
        assert ctx["st"].specs[name].res == f"dskip{i - 1}"
        g, _, out = product(ctx, name, {f"dye{i}": cl(dy)})
        (cols, _, idx), = D.dst_index(g["dsts"], g["ntab"], g["M"], g["N"], g["Npad"], g["TT"], g["J"]).values()
        out = out[:, cols] + res.view(-1)[idx]                  # laid out exactly like dst[0]
        into[f"dz{i - 1}"].view(-1)[idx] += out
    assert rel(into[f"dz{i - 1}"], cl(dx) + res) < TOL


@pytest.mark.parametrize("j", [0, 5])
def test_decoder_forward_pair(ctx, j):
    """two sources (complex_cat of the previous decoder output, stored with its dropped first frame in front, and the skip tensor);
    dec5: the fp32 mask layer, 2 of 16 columns valid, T of the T + 1 frames"""
    kn = ctx["st"].cfg.kernel_num
    idx = 6 - j
    c1, f_in = kn[idx], 256 >> idx
    a, skip = rnd(ctx, B, c1, f_in, T), rnd(ctx, B, c1, f_in, T)
    full = O.complex_deconv2d(O.complex_cat(a, skip), *conv_params(ctx, f"decoder.{j}."))
    s1 = "P" if j == 0 else f"zd{j - 1}"
    a_cl = cl(a)
    if j > 0:
        a_cl = torch.cat([torch.full((B, 1, f_in, c1), 7.0, dtype=F64), a_cl], 1)
    bufs = {s1: a_cl, f"z{5 - j}": cl(skip)}
    dname = "mask" if j == 5 else f"yd{j}"
    into = {dname: torch.zeros(B, *ctx["geom"][dname], dtype=F64)}
    for par in (0, 1):
        g, _, out = product(ctx, f"dec{j}.fwd{par}", bufs)
        if j == 5:
            assert g["N"] == 2 and g["Npad"] == 16
        scatter(ctx, f"dec{j}.fwd{par}", g, out, into)
    ref = cl(full)[:, 1:] if j == 5 else cl(full)
    assert rel(into[dname], ref) < TOL


def fold(ctx, spec, dW, dbias):
    """packed gradients -> flat parameter gradients through the spec's own entries (what the un-pack table does)"""
    from sehip.plan import enc_entry
    grads = torch.zeros(ctx["st"].layout.n_params, dtype=F64)
    e = torch.from_numpy(enc_entry(spec.widx, spec.wneg).astype(np.int64))
    ok = e >= 0
    grads.index_add_(0, e[ok] >> 1, torch.where((e[ok] & 1) == 1, -dW[ok], dW[ok]))
    for col in (0, 1):
        e = torch.from_numpy(spec.bias_pairs[:, col].astype(np.int64))
        ok = e >= 0
        grads.index_add_(0, e[ok] >> 1, torch.where((e[ok] & 1) == 1, -dbias[ok], dbias[ok]))
    return grads


def test_weight_gradient(ctx):
    """dW = dOut^T A, dbias = column sums of dOut (enc3), folded through the pack entries, against autograd of the oracle"""
    i = 3
    st, kn = ctx["st"], ctx["st"].cfg.kernel_num
    spec = st.specs[f"enc{i}.fwd"]
    x = rnd(ctx, B, kn[i], 256 >> i, T)
    ps = [t.clone().requires_grad_(True) for t in conv_params(ctx, f"encoder.{i}.")]
    y = O.complex_conv2d(x, *ps)
    dy = rnd(ctx, *y.shape)
    ref = torch.autograd.grad((y * dy).sum(), ps)
    g, A, _ = product(ctx, f"enc{i}.fwd", {f"z{i - 1}": cl(x)})
    (cols, _, idx), = D.dst_index(g["dsts"], g["ntab"], g["M"], g["N"], g["Npad"], g["TT"], g["J"]).values()
    dO = torch.zeros(g["M"], g["Npad"], dtype=F64)
    dO[:, cols] = cl(dy).view(-1)[idx]
    grads = fold(ctx, spec, dO.t() @ A, dO.sum(0))
    pre = f"encoder.{i}."
    for nm, r in zip(("0.real_conv.weight", "0.real_conv.bias", "0.imag_conv.weight", "0.imag_conv.bias"), ref):
        off, shape = st.layout.param_off[pre + nm]
        assert rel(grads[off:off + r.numel()].reshape(shape), r) < TOL, nm


# ---- the fused BatchNorm pieces against autograd ------------------------------------------------------------------------------------
def bn_records(y, Wrr, Wri, Wii, Br, Bi, eps=1e-5):
    """forward records [Cr, 16] from the definitions (sehip_cbn_finalize; csrc/cbn.hip cbn_fwd_record): biased batch moments,
    U = (V + eps I)^(-1/2) in closed form, Z = W U"""
    cr = Wrr.numel()
    yr, yi = y[:, :cr], y[:, cr:]
    mr, mi = yr.mean(0), yi.mean(0)
    vrr, vri, vii = ((yr - mr) ** 2).mean(0) + eps, ((yr - mr) * (yi - mi)).mean(0), ((yi - mi) ** 2).mean(0) + eps
    s = (vrr * vii - vri * vri).sqrt()
    t = (vrr + vii + 2 * s).sqrt()
    rst = 1.0 / (s * t)
    urr, uii, uri = (s + vii) * rst, (s + vrr) * rst, -vri * rst
    rec = torch.zeros(cr, 16, dtype=F64)
    for k, v in enumerate([Wrr * urr + Wri * uri, Wrr * uri + Wri * uii, Wri * urr + Wii * uri, Wri * uri + Wii * uii, mr, mi, Br, Bi, urr,
                           uri, uii, vrr, vri, vii]):
        rec[:, k] = v
    return rec


def bn_bwd_records(sums, rec, Wrr, Wri, Wii, n):
    """backward records [Cr, 16] and (gWrr, gWri, gWii, gBr, gBi) from the six sums (sehip_cbn_bwd_finalize; cbn_bwd_record)"""
    sdr, sdi, qrr, qri, qir, qii = sums
    urr, uri, uii, vrr, vri, vii = (rec[:, k] for k in range(8, 14))
    prr, pri, pir, pii = qrr * urr + qri * uri, qrr * uri + qri * uii, qir * urr + qii * uri, qir * uri + qii * uii
    hrr, hri = Wrr * qrr + Wri * qir, Wrr * qri + Wri * qii
    hir, hii = Wri * qrr + Wii * qir, Wri * qri + Wii * qii
    dUrr, dUri, dUii = hrr, hri + hir, hii
    s = (vrr * vii - vri * vri).sqrt()
    t = (vrr + vii + 2 * s).sqrt()
    rst = 1.0 / (s * t)
    d_rst = dUrr * (s + vii) - dUri * vri + dUii * (s + vrr)
    d_s = (dUrr + dUii) * rst + d_rst * (-rst / s)
    d_vii, d_vrr, d_vri = dUrr * rst, dUii * rst, -dUri * rst
    d_t = d_rst * (-rst / t)
    d_tau = d_t / (2 * t)
    d_s = d_s + d_t / t
    d_delta = d_s / (2 * s)
    d_vrr, d_vii, d_vri = d_vrr + d_delta * vii + d_tau, d_vii + d_delta * vrr + d_tau, d_vri + d_delta * (-2 * vri)
    arr, ari, air, aii = urr * Wrr + uri * Wri, urr * Wri + uri * Wii, uri * Wrr + uii * Wri, uri * Wri + uii * Wii
    b = torch.zeros(rec.shape[0], 16, dtype=F64)
    for k, v in enumerate([arr, ari, air, aii, 2 * d_vrr / n, d_vri / n, 2 * d_vii / n, -(arr * sdr + ari * sdi) / n,
                           -(air * sdr + aii * sdi) / n]):
        b[:, k] = v
    return b, (prr, pri + pir, pii, sdr, sdi)


def test_fused_batchnorm_pieces_against_autograd(ctx):
    """the 6 Cr + 1 sums of the reduce pass and the value the apply pass would store, against autograd through the oracle's
    ComplexBatchNorm + PReLU in float64: the parameter gradients the sums define, the slope's gradient, and the input gradient"""
    cr, Bq, Fq, Tq = 8, 2, 6, 5
    g = ctx["g"]
    x = torch.randn(Bq, 2 * cr, Fq, Tq, generator=g, dtype=F64) * 0.7 + 0.2
    x = x.requires_grad_(True)
    p = {k: v.double().requires_grad_(True) for k, v in (("Wrr", 1 + 0.3 * torch.randn(cr, generator=g)), ("Wri", torch.rand(cr, generator=g) - 0.5),
                                                          ("Wii", 1 + 0.3 * torch.randn(cr, generator=g)), ("Br", 0.2 * torch.randn(cr, generator=g)),
                                                          ("Bi", 0.2 * torch.randn(cr, generator=g)))}
    slope = torch.tensor([0.25], dtype=F64, requires_grad=True)
    z = F.prelu(O.complex_batchnorm(x, p, "", True), slope)
    dz = torch.randn(z.shape, generator=g, dtype=F64)
    ref = torch.autograd.grad((z * dz).sum(), [x, p["Wrr"], p["Wri"], p["Wii"], p["Br"], p["Bi"], slope])
    rows = lambda t: cl(t).reshape(-1, 2 * cr)
    y2, dz2 = rows(x), rows(dz)
    W = [p[k].detach() for k in ("Wrr", "Wri", "Wii")]
    rec = bn_records(y2, *W, p["Br"].detach(), p["Bi"].detach())
    sums, sl, mags, sl_mag, slack, sl_slack = D.bn_reduce_sums(dz2, y2, rec, slope.detach())
    assert float(slack.max()) == 0.0 and float(sl_slack) == 0.0 and float(mags.min()) > 0.0
    brec, g5 = bn_bwd_records(sums, rec, *W, y2.shape[0])
    for got, want, nm in zip(g5, ref[1:6], ("gWrr", "gWri", "gWii", "gBr", "gBi")):
        assert rel(got, want) < TOL, nm
    assert abs(float(sl) - float(ref[6])) < TOL * abs(float(ref[6]))
    dy, mag, amb = D.bn_apply(dz2, y2, rec, brec, slope.detach())
    assert not bool(amb.any()) and bool((mag >= dy.abs() * (1 - 1e-12)).all())
    assert rel(dy, rows(ref[0])) < TOL
    # the same value as float32 arithmetic would evaluate it (what the bn_dz weight gradient rounds to bf16): every fusing order
    # within a few float32 roundings of the float64 value, measured against the size of its terms
    rec32, brec32 = rec.float(), brec.float()
    y16, dz16 = D.round_bf16(y2), D.round_bf16(dz2)
    dy64, mag64, _ = D.bn_apply(dz16, y16, rec32, brec32, slope.detach())
    for order in ("none", "lhs", "rhs"):
        dy32 = D.bn_apply_f32(dz16, y16, rec32, brec32, slope.detach(), order)
        assert torch.equal(dy32, dy32.float().double())
        assert float(((dy32 - dy64).abs() / mag64).max()) < 8 * D.EPS24, order


def test_ambiguous_prelu_branches_are_reported(ctx):
    """an element whose pre-activation is (numerically) zero: float32 and float64 may take different PReLU branches; the reference
    reports by how much its sums could move instead of pretending to know"""
    cr = 2
    rec = torch.zeros(cr, 16, dtype=F64)
    rec[:, 0] = rec[:, 3] = 1.0                              # Z = I, M = 0: v = y + B
    rec[1, 7] = -1.0                                         # Bi of channel 1: v_i = y_i - 1 cancels
    y = torch.tensor([[1.0, -1.0, 0.5, 1.0 + 1e-12], [2.0, 3.0, -1.0, 3.0]], dtype=F64)
    dz = torch.ones_like(y)
    sums, sl, mags, sl_mag, slack, sl_slack = D.bn_reduce_sums(dz, y, rec, 0.25)
    assert float(slack[1, 1]) == pytest.approx(0.75) and float(slack[0].sum()) == 0.0 and float(slack[1, 0]) == 0.0
    assert float(sums[0, 1]) == pytest.approx(0.25 + 1.0) and float(sums[1, 0]) == pytest.approx(1.0 + 0.25)
    assert float(sums[1, 1]) == pytest.approx(2.0) and float(sums[0, 0]) == pytest.approx(2.0)


# ---- w_tiled ------------------------------------------------------------------------------------------------------------------------
def test_untile_round_trips_the_plan_order(ctx):
    """desc_ref.untile_w (worded after include/sehip.h) against GemmSpec.tile_weights, the table builder: the tiled pack entries,
    un-tiled, are the [Npad][K] entries -- for a 128-column-tile product, a 64-column one and a two-source one"""
    from sehip.plan import enc_entry
    st = ctx["st"]
    seen = 0
    for name in ("enc3.fwd", "enc2.dg0", "dec0.fwd1", "dec2.fwd0", "enc5.fwd"):
        sp = st.specs[name]
        if not sp.w_tiled:
            continue
        seen += 1
        cs = sp.v3_channels()
        nat = torch.from_numpy(enc_entry(sp.widx, sp.wneg).astype(np.int64))
        tiled = torch.from_numpy(enc_entry(sp.widx_packed, sp.wneg_packed).astype(np.int64)).reshape(-1)
        assert torch.equal(D.untile_w(tiled, sp.Npad, sp.K, sp.conv[0], cs[0] + cs[1]), nat), name
        assert torch.equal(D.tile_w(nat, sp.Npad, sp.K, sp.conv[0], cs[0] + cs[1]), tiled), name
        assert not torch.equal(tiled.reshape(sp.Npad, sp.K), nat)
        # the packing table holds exactly these entries at w_off
        assert np.array_equal(st.wtab[sp.w_off:sp.w_off + sp.Npad * sp.K], tiled.numpy().astype(np.int32))
    assert seen >= 3


# ---- sensitivity of the GPU test's gates, on the reference side -----------------------------------------------------------------------
def passes_bf16(got, want):
    return W.gate_bf16(got, want)[0]


def passes_f32(got, want):
    return W.gate_f32(got, want)[0]


def passes_dw(got, want, g, src_c):
    return W.gate_dw(got, want, g["ktab"], src_c)[0]


def drop_last_frame(A, g):
    """zero what the rows read from the LAST valid frame of source 0"""
    kt = g["ktab"]
    T_s, tlo, thi = g["srcs"][0][:3]
    toff = (kt[:, 1] >> 16).repeat_interleave(8)
    m = torch.arange(g["M"])
    t = (m // g["J"]) % g["TT"]
    hit = ((t[:, None] + toff[None, :]) == thi - 1) & (kt[:, 0].repeat_interleave(8) == 0)[None, :]
    assert bool(hit.any())
    return torch.where(hit, torch.zeros((), dtype=F64), A)


def shift_one_tap(kt, g):
    """the chunks of ONE (frame, row) tap of source 0 read one row further down"""
    C_s = g["srcs"][0][4]
    first = int((kt[:, 0] == 0).nonzero()[0])
    same = (kt[:, 0] == 0) & (kt[:, 1] == kt[first, 1])
    roff = ((kt[:, 1] & 0xffff) ^ 0x8000) - 0x8000
    kt[same, 1] = ((kt[same, 1] >> 16) << 16) | ((roff[same] + 1) & 0xffff)
    kt[same, 2] += C_s
    return kt


CASES = [("enc3.fwd", "bf16"), ("dec5.fwd0", "f32"), ("dec1.fwd1", "bf16")]


def _inputs(ctx, name):
    st, kn = ctx["st"], ctx["st"].cfg.kernel_num
    spec = st.specs[name]
    bufs = {}
    for nm, _ in spec.srcs:
        # (bf16-representable inputs, as every operand on the device is)
        bufs[nm] = D.round_bf16(rnd(ctx, B, *ctx["geom"][nm]))
    return bufs


@pytest.mark.parametrize("name,kind", CASES)
def test_gates_reject_subtly_wrong_products(ctx, name, kind):
    """got = the correctly rounded result; want perturbed three ways; each must FAIL the gate the GPU test applies to that
    destination -- and the unperturbed want must pass it"""
    bufs = _inputs(ctx, name)
    g, A, out = product(ctx, name, bufs)
    N = g["N"]
    got = D.round_bf16(out[:, :N]) if kind == "bf16" else out[:, :N].float().double()
    passes = passes_bf16 if kind == "bf16" else passes_f32
    assert passes(got, out[:, :N])
    _, _, dropped = product(ctx, name, bufs, a_edit=drop_last_frame)
    _, _, shifted = product(ctx, name, bufs, ktab_edit=shift_one_tap)
    for what, bad in (("last frame dropped", dropped), ("tap shifted", shifted), ("scaled by 1 + 1e-3", out * (1 + 1e-3))):
        assert not torch.equal(bad, out)
        assert not passes(got, bad[:, :N]), what


def test_two_rounding_gate_for_residual_launches(ctx):
    """a launch that rounds the product to bf16, adds `res` to that and rounds again (conv_gemm_v3, convt_stream, ...): its CORRECT
    result is outside the one-rounding gate wherever product and residual cancel, and inside desc_ref.out_err2 with the same
    constants; a dropped last frame and a shifted tap are outside that one too"""
    name = "enc2.dg0"
    bufs = _inputs(ctx, name)
    g, A, out = product(ctx, name, bufs)
    res = D.round_bf16(rnd(ctx, g["M"], g["N"]) * out.abs().mean())
    got = D.round_bf16(D.round_bf16(out) + res)
    assert W.gate_bf16(got, out + res, out)[0]
    assert not W.gate_bf16(got, out + res)[0]
    _, _, dropped = product(ctx, name, bufs, a_edit=drop_last_frame)
    _, _, shifted = product(ctx, name, bufs, ktab_edit=shift_one_tap)
    for what, bad in (("last frame dropped", dropped), ("tap shifted", shifted)):
        assert not W.gate_bf16(got, bad + res, bad)[0], what


def test_gates_reject_subtly_wrong_weight_gradients(ctx):
    name = "enc3.fwd"
    bufs = _inputs(ctx, name)
    g, A, _ = product(ctx, name, bufs)
    src_c = [s[4] for s in g["srcs"]]
    dO = D.round_bf16(rnd(ctx, g["M"], g["N"]))
    want = dO.t() @ A
    got = want.float().double()
    assert passes_dw(got, want, g, src_c)
    _, A1, _ = product(ctx, name, bufs, a_edit=drop_last_frame)
    _, A2, _ = product(ctx, name, bufs, ktab_edit=shift_one_tap)
    for what, bad in (("last frame dropped", dO.t() @ A1), ("tap shifted", dO.t() @ A2), ("scaled", want * (1 + 1e-3))):
        assert not passes_dw(got, bad, g, src_c), what
    # a tap shifted by one row moves ONE (frame, row) slice of K: the whole-matrix norm alone is the weaker gate
    errs = dict(D.slice_errors(got, dO.t() @ A2, g["ktab"], src_c))
    assert sum(e > F32_TOL for e in errs.values()) == 1 and len(errs) == 10


def test_sum_gate_rejects_one_missing_row(ctx):
    """the fused statistics (and the reduce sums): float32 sums of n addends against float64, bound 4 * 2^-24 * sqrt(n) * sum |addend|.
    One row of one frame missing must fail it -- here, and by arithmetic at the largest n of the GPU test's shapes"""
    name = "enc3.fwd"
    g, A, out = product(ctx, name, _inputs(ctx, name))
    y = D.round_bf16(out)                                     # the values the launch stores
    cr = g["N"] // 2
    re, im = y[:, :cr], y[:, cr:]                             # (columns in tile order: a permutation of the channels, same for both sets)
    adds = [re, im, re * re, re * im, im * im]
    n = y.shape[0]
    got = torch.stack([a.float().sum(0).double() for a in adds])
    want = torch.stack([a.sum(0) for a in adds])
    mag = torch.stack([a.abs().sum(0) for a in adds])
    assert W.gate_sum(got, want, n, mag)[0]
    bad = torch.stack([a[1:].sum(0) for a in adds])
    for k in range(5):                                        # every kind of sum notices
        assert not W.gate_sum(got[k], bad[k], n, mag[k])[0], k
    # a sanity bound, not evidence (the evidence is the data-based check above): at the n of the GPU test's shapes the allowance is
    # below 1 / n of sum |addend|, the size of an average row
    for n in (16 * 128, 3 * 44 * 64, 3 * 43 * 128):
        assert W.SUM_FACTOR * D.EPS24 * n ** 0.5 < 1.0 / n
    assert float(D.sum_bound(4, torch.tensor(1.0), 1e9)) == 5 * D.EPS24      # never above the ceiling

