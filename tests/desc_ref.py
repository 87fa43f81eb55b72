"""The arithmetic a sehip_gemm_desc (include/sehip.h) asks for, restated in plain float64 torch -- none of libsehip.  Device-agnostic:
tests/test_desc_ref_host.py feeds it CPU tensors built from a GemmSpec and proves it against the oracle's convolutions and autograd;
tests/test_gpu_dccrn_products.py feeds it the device tensors a bound CGemmDesc points at and judges every DCCRN product launch with it.

  gather_A          row m = (b*TT + t)*J + j of the implicit matrix, 8-element chunks through the bound chunk table (sehip_kchunk)
  dst_index         element index of (row m, column n) in each destination, through the column table (sehip_nchunk)
  expected_weights  bf16(+-params[...]) through the plan's own pack entries ([Npad][K] order), expected_bias likewise
  untile_w          undoes the w_tiled order as sehip.h words it
  bn_reduce_sums    the 6 Cr + 1 sums of sehip_cbn_bwd_reduce, from the record definitions (csrc/cbn.hip)
  bn_apply          the value sehip_cbn_bwd_apply would store; bn_apply_f32: the same as float32 arithmetic evaluates it
  Resolver          descriptor pointer -> (flat tensor, element offset) by address range
  out_err2 / sum_bound / tap_slices: the gates' own arithmetic, shared by the host sensitivity test and the GPU test
"""
import numpy as np
import torch

F64 = torch.float64
EPS24 = 2.0 ** -24


# ---- pointers -----------------------------------------------------------------------------------------------------------------------
class Resolver:
    """Maps a raw address to the registered tensor whose storage range holds it (descriptors of a chunked launch point into the
    middle of a buffer, plan.DCCRNWorkspace._chunk_desc).  The largest tensor that holds the address wins (`h1` over `h1_0`)."""

    def __init__(self):
        self.items = []

    def add(self, name, t):
        if t is not None and t.numel():
            self.items.append((t.data_ptr(), t.data_ptr() + t.numel() * t.element_size(), name, t))
            self.items.sort(key=lambda e: e[0] - e[1])

    def find(self, ptr):
        """(name, flat tensor, element offset)"""
        for lo, hi, name, t in self.items:
            if lo <= ptr < hi:
                assert (ptr - lo) % t.element_size() == 0, (name, ptr - lo)
                return name, t.reshape(-1), (ptr - lo) // t.element_size()
        raise KeyError(f"pointer {ptr:#x} lies in no registered buffer")

    def by_name(self, name):
        return next(t for _, _, n, t in self.items if n == name).reshape(-1)

    def view(self, ptr):
        """flat tensor that starts at ptr (runs to the end of its buffer)"""
        _, t, off = self.find(ptr)
        return t[off:]


# ---- the implicit matrix ------------------------------------------------------------------------------------------------------------
def _rows(M, TT, J, dev):
    m = torch.arange(M, device=dev)
    j, bt = m % J, m // J
    return bt // TT, bt % TT, j


def gather_A(srcs, ktab, M, K, TT, J, fmul, tmul=1):
    """[M, K] float64.  srcs: [(flat tensor, T, tlo, thi, F, C)] (index = sehip_kchunk.src); ktab: integer tensor [K/8, 4] of BOUND
    chunks (src, (frame offset << 16) | (row offset & 0xffff), element delta, valid rows of a narrow chunk).  Element (m, 8 c + e) is
    src[((b*T_s + t*tmul)*F_s + j*fmul)*C_s + delta + e], zero unless frame t*tmul + frame offset lies in [tlo, thi) and row
    j*fmul + row offset in [0, F_s); src = -1: a zero chunk.  C_s == 2 (narrow): 4 consecutive rows x 2 channels, e = 2 q + channel,
    row q valid for q < coff and inside [0, F_s)."""
    dev = ktab.device
    kt = ktab.to(torch.int64)
    assert kt.shape == (K // 8, 4)
    b, t, j = _rows(M, TT, J, dev)
    tm = max(int(tmul), 1)
    toff = kt[:, 1] >> 16                                     # arithmetic shift of the sign-extended int32
    roff = ((kt[:, 1] & 0xffff) ^ 0x8000) - 0x8000
    A = torch.zeros(M, K // 8, 8, dtype=F64, device=dev)
    e8 = torch.arange(8, device=dev)
    for s, (x, T_s, tlo, thi, F_s, C_s) in enumerate(srcs):
        sel = (kt[:, 0] == s).nonzero().flatten()
        if sel.numel() == 0:
            continue
        frame = (t * tm)[:, None] + toff[sel][None, :]
        row = (j * fmul)[:, None] + roff[sel][None, :]
        ok = (frame >= tlo) & (frame < thi)
        base = (((b * T_s + t * tm) * F_s + j * fmul) * C_s)[:, None] + kt[sel, 2][None, :]
        idx = base[:, :, None] + e8
        if C_s == 2:
            q = e8 // 2
            rq = row[:, :, None] + q
            ok = ok[:, :, None] & (rq >= 0) & (rq < F_s) & (q[None, None, :] < kt[sel, 3][None, :, None])
        else:
            ok = (ok & (row >= 0) & (row < F_s))[:, :, None].expand(-1, -1, 8)
        v = x[idx.clamp(0, x.numel() - 1)].to(F64)
        A[:, sel] = torch.where(ok, v, torch.zeros((), dtype=F64, device=dev))
    return A.reshape(M, K)


def dst_index(dsts, ntab, M, N, Npad, TT, J):
    """{destination q: (columns n [k], destination column of each [k], element index [M, k])}.  dsts: [(T, F, C, toff, fmul, fadd, tmul)] (sehip_dst without pointer
    and type); ntab: integer tensor [Npad/4, 4] (dst, coff, nvalid, -).  Column n = 4 g + q (q < nvalid[g], n < N) of row (b, t, j)
    lives at ((b*T + t*tmul + toff)*F + j*fmul + fadd)*C + coff[g] + q of destination dst[g]."""
    dev = ntab.device
    nt = ntab.to(torch.int64)
    assert nt.shape[0] == Npad // 4
    n = torch.arange(Npad, device=dev)
    g, q = n // 4, n % 4
    valid = (q < nt[g, 2]) & (n < N)
    col = nt[g, 1] + q
    b, t, j = _rows(M, TT, J, dev)
    out = {}
    for k, (T, F, C, toff, fmul, fadd, tmul) in enumerate(dsts):
        sel = (valid & (nt[g, 0] == k)).nonzero().flatten()
        if sel.numel() == 0:
            continue
        row = ((b * T + t * max(int(tmul), 1) + toff) * F + j * fmul + fadd) * C
        out[k] = (sel, col[sel], row[:, None] + col[sel][None, :])
    return out


# ---- weights ------------------------------------------------------------------------------------------------------------------------
def _term(params, e):
    e = torch.as_tensor(np.asarray(e, dtype=np.int64), device=params.device)
    v = torch.where(e >= 0, params[e.clamp(min=0) >> 1], torch.zeros((), dtype=params.dtype, device=params.device))
    return torch.where((e >= 0) & ((e & 1) == 1), -v, v)      # (an absent entry packs as +0, whatever its low bit)


def expected_weights(spec, params):
    """bf16 [Npad, K] in the descriptor's K order: bf16(+-params[e]) through the plan's pack entries (tests/test_host_plan.py
    plan_entry), never read from the packed buffer."""
    from sehip.plan import enc_entry
    return _term(params.float(), enc_entry(spec.widx, spec.wneg)).to(torch.bfloat16)


def expected_bias(spec, params):
    """float64 [Npad]: +-params[e0] +- params[e1] (sehip_pack_f32), or None"""
    if spec.bias_pairs is None:
        return None
    p = params.to(F64)
    return _term(p, spec.bias_pairs[:, 0]) + _term(p, spec.bias_pairs[:, 1])


def untile_w(flat, Npad, K, cv_nf, ctot):
    """[Npad, K] from the w_tiled order of include/sehip.h: for output tile nt (128 columns; 64 when Npad is not a multiple of 128),
    16-channel chunk ch of the concatenated sources and tap pair j (taps 2 j, 2 j + 1 of the K order (kt, tap, source, channel)), one
    contiguous block [2 taps][128 (64) n][16 channels] at element ((nt * (Ctot / 16) + ch) * cv_nf + j) * 4096 (2048)."""
    bn = 64 if Npad % 128 else 128
    ntn, nch = Npad // bn, ctot // 16
    assert K == 2 * cv_nf * ctot and flat.numel() == Npad * K
    a = flat.reshape(ntn, nch, cv_nf, 2, bn, 16)              # [nt][ch][j][u][n][c]
    return a.permute(0, 4, 2, 3, 1, 5).reshape(Npad, K)       # [nt][n][(j, u) = tap 2 j + u][ch][c]


def tile_w(w, Npad, K, cv_nf, ctot):
    """the inverse of untile_w (what a table builder has to produce)"""
    bn = 64 if Npad % 128 else 128
    ntn, nch = Npad // bn, ctot // 16
    a = w.reshape(ntn, bn, cv_nf, 2, nch, 16)
    return a.permute(0, 4, 2, 3, 1, 5).reshape(-1)


# ---- ComplexBatchNorm + PReLU backward, from the records ----------------------------------------------------------------------------
# forward record (sehip_cbn_finalize, [Cr][16]): 0 Zrr 1 Zri 2 Zir 3 Zii 4 Mr 5 Mi 6 Br 7 Bi (8 .. 13 whitening matrix and covariance)
# backward record (sehip_cbn_bwd_finalize, [Cr][16]): 0 Arr 1 Ari 2 Air 3 Aii 4 Err 5 Eri 6 Eii 7 kr 8 ki
AMBIGUOUS = 2.0 ** -18      # |v| below this fraction of its terms: fp32 and float64 may disagree about the PReLU branch


def _bn_common(dz, y, coef, slope):
    cr_ = coef.shape[0]
    k = coef.to(F64)
    dz, y = dz.to(F64), y.to(F64)
    c_r, c_i = y[:, :cr_] - k[:, 4], y[:, cr_:] - k[:, 5]
    t_r = (k[:, 0] * c_r, k[:, 1] * c_i)
    t_i = (k[:, 2] * c_r, k[:, 3] * c_i)
    v_r, v_i = t_r[0] + t_r[1] + k[:, 6], t_i[0] + t_i[1] + k[:, 7]
    a = float(slope)
    g_r, g_i = dz[:, :cr_], dz[:, cr_:]
    neg_r, neg_i = ~(v_r > 0), ~(v_i > 0)
    d_r = torch.where(neg_r, a * g_r, g_r)
    d_i = torch.where(neg_i, a * g_i, g_i)
    amb_r = v_r.abs() <= AMBIGUOUS * (t_r[0].abs() + t_r[1].abs() + k[:, 6].abs())
    amb_i = v_i.abs() <= AMBIGUOUS * (t_i[0].abs() + t_i[1].abs() + k[:, 7].abs())
    return dict(c_r=c_r, c_i=c_i, v_r=v_r, v_i=v_i, g_r=g_r, g_i=g_i, d_r=d_r, d_i=d_i, neg_r=neg_r, neg_i=neg_i, amb_r=amb_r,
                amb_i=amb_i, a=a)


def bn_reduce_sums(dz, y, coef, slope):
    """dz, y [rows, 2 Cr] (real half | imaginary half), coef [Cr, 16] forward records, slope the PReLU weight.  With c = y - M,
    v = Z c + B, d = dz * (v > 0 ? 1 : slope):  sums [6, Cr] = sum d_r, sum d_i, sum d_r c_r, sum d_r c_i, sum d_i c_r, sum d_i c_i
    and the slope's sum of dz * v over v <= 0 (csrc/cbn.hip cbn_bwd_reduce_kernel).  Returns (sums, slope sum, sum |addend| [6, Cr],
    slope's sum |addend|, slack [6, Cr], slope slack): slack = by how much a sum moves if every element whose branch float32 and
    float64 may decide differently (|v| within AMBIGUOUS of zero) took the other branch -- the reference's own uncertainty."""
    q = _bn_common(dz, y, coef, slope)
    add = [q["d_r"], q["d_i"], q["d_r"] * q["c_r"], q["d_r"] * q["c_i"], q["d_i"] * q["c_r"], q["d_i"] * q["c_i"]]
    sums = torch.stack([x.sum(0) for x in add])
    mags = torch.stack([x.abs().sum(0) for x in add])
    sl = torch.where(q["neg_r"], q["g_r"] * q["v_r"], 0 * q["v_r"]) + torch.where(q["neg_i"], q["g_i"] * q["v_i"], 0 * q["v_i"])
    sl_mag = (torch.where(q["neg_r"], (q["g_r"] * q["v_r"]).abs(), 0 * q["v_r"]) + torch.where(q["neg_i"], (q["g_i"] * q["v_i"]).abs(), 0 * q["v_i"])).sum()
    one_a = abs(1.0 - q["a"])
    fr = torch.where(q["amb_r"], one_a * q["g_r"].abs(), 0 * q["g_r"])
    fi = torch.where(q["amb_i"], one_a * q["g_i"].abs(), 0 * q["g_i"])
    slack = torch.stack([fr.sum(0), fi.sum(0), (fr * q["c_r"].abs()).sum(0), (fr * q["c_i"].abs()).sum(0), (fi * q["c_r"].abs()).sum(0),
                         (fi * q["c_i"].abs()).sum(0)])
    sl_slack = (torch.where(q["amb_r"], (q["g_r"] * q["v_r"]).abs(), 0 * q["v_r"]) + torch.where(q["amb_i"], (q["g_i"] * q["v_i"]).abs(), 0 * q["v_i"])).sum()
    return sums, sl.sum(), mags, sl_mag, slack, sl_slack


def bn_apply(dz, y, coef, bcoef, slope):
    """what sehip_cbn_bwd_apply would store, before its rounding to bf16: dy_r = Arr d_r + Ari d_i + Err c_r + Eri c_i + kr,
    dy_i = Air d_r + Aii d_i + Eri c_r + Eii c_i + ki  [rows, 2 Cr] float64.  Also returns sum |term| per element (the scale of the
    float32 evaluation's error) and the mask of elements whose PReLU branch is ambiguous (see bn_reduce_sums)."""
    q = _bn_common(dz, y, coef, slope)
    k = bcoef.to(F64)
    tr = [k[:, 0] * q["d_r"], k[:, 1] * q["d_i"], k[:, 4] * q["c_r"], k[:, 5] * q["c_i"], k[:, 7].expand_as(q["c_r"])]
    ti = [k[:, 2] * q["d_r"], k[:, 3] * q["d_i"], k[:, 5] * q["c_r"], k[:, 6] * q["c_i"], k[:, 8].expand_as(q["c_r"])]
    dy = torch.cat([sum(tr), sum(ti)], 1)
    mag = torch.cat([sum(x.abs() for x in tr), sum(x.abs() for x in ti)], 1)
    amb = q["amb_r"] | q["amb_i"]
    return dy, mag, torch.cat([amb, amb], 1)


def bn_apply_f32(dz, y, coef, bcoef, slope, order="lhs"):
    """bn_apply evaluated as float32 arithmetic would: every operation rounded to float32 (carried in float64: a product of two
    float32 is exact there), `order` = how the multiply-adds of v = Zrr c_r + Zri c_i + B and of dy = p0 d_r + p1 d_i + p2 c_r + p3 c_i
    + p4 are fused: "none" (every product rounded), "lhs" (a * b + c * d -> fma(a, b, round(c * d)), later terms fma'd onto the sum:
    what the compiler's contraction makes of the source expression), "rhs" (round(a * b) first, every later term fma'd onto it)."""
    r32 = lambda x: x.to(torch.float32).to(F64)
    cr_ = coef.shape[0]
    k, b = coef.to(torch.float32).to(F64), bcoef.to(torch.float32).to(F64)
    a = float(torch.tensor(float(slope), dtype=torch.float32))
    dz, y = dz.to(F64), y.to(F64)

    def chain(terms, last):
        (p0, x0), (p1, x1) = terms[0], terms[1]
        if order == "none":
            t = r32(r32(p0 * x0) + r32(p1 * x1))
        elif order == "lhs":
            t = r32(p0 * x0 + r32(p1 * x1))
        else:
            t = r32(r32(p0 * x0) + p1 * x1)
        for p, x in terms[2:]:
            t = r32(t + (r32(p * x) if order == "none" else p * x))
        return r32(t + last)
    c_r, c_i = r32(y[:, :cr_] - k[:, 4]), r32(y[:, cr_:] - k[:, 5])
    v_r = chain([(k[:, 0], c_r), (k[:, 1], c_i)], k[:, 6])
    v_i = chain([(k[:, 2], c_r), (k[:, 3], c_i)], k[:, 7])
    d_r = torch.where(v_r > 0, dz[:, :cr_], r32(dz[:, :cr_] * a))
    d_i = torch.where(v_i > 0, dz[:, cr_:], r32(dz[:, cr_:] * a))
    dy_r = chain([(b[:, 0], d_r), (b[:, 1], d_i), (b[:, 4], c_r), (b[:, 5], c_i)], b[:, 7])
    dy_i = chain([(b[:, 2], d_r), (b[:, 3], d_i), (b[:, 5], c_r), (b[:, 6], c_i)], b[:, 8])
    return torch.cat([dy_r, dy_i], 1)


# ---- the gates' arithmetic ----------------------------------------------------------------------------------------------------------
def round_bf16(x):
    return x.to(torch.float32).to(torch.bfloat16).to(F64)


def out_err2(got, want, prod):
    """(rms, max) of |got - want| / (|want| + |prod| + floor) for a destination the kernel rounds TWICE: the product (+ bias) is
    rounded to bf16 where the tile is staged, the residual is added to that and the sum rounded again.  Each rounding is half a bf16
    ulp of its own value, so against |want| + |prod| the two together stay inside the constants of ONE rounding against |want|
    (tests/test_gpu_demucs_fullwidth.py out_err, whose floor this keeps)."""
    got, want, prod = got.double(), want.double(), prod.double()
    floor = 1e-3 * float(want.pow(2).mean().sqrt())
    r = (got - want).abs() / (want.abs() + prod.abs() + floor)
    return float(r.pow(2).mean().sqrt()), float(r.max())


def sum_bound(n, mag, factor=4.0):
    """|got - want| allowed for a float32 sum of n addends with sum |addend| = mag: factor * 2^-24 * sqrt(n) * mag (the random-order
    model), never above the ceiling that holds for ANY order, (n + 1) * 2^-24 * mag."""
    return torch.minimum(factor * EPS24 * (n ** 0.5) * mag, (n + 1) * EPS24 * mag)


def tap_slices(ktab, src_channels):
    """[((frame offset, row offset), columns of K)] from a bound chunk table: the (frame tap, row tap) every column of the implicit
    matrix reads.  A narrow chunk (source with 2 channels) spans 4 row taps, 2 columns each; zero chunks / rows are left out."""
    kt = ktab.to(torch.int64).cpu()
    toff = (kt[:, 1] >> 16).repeat_interleave(8)
    roff = (((kt[:, 1] & 0xffff) ^ 0x8000) - 0x8000).repeat_interleave(8)
    src = kt[:, 0].repeat_interleave(8)
    e = torch.arange(8).repeat(kt.shape[0])
    valid = src >= 0
    for s, c in enumerate(src_channels):
        if c == 2:
            nar = src == s
            roff = torch.where(nar, roff + e // 2, roff)
            valid = valid & (~nar | (e // 2 < kt[:, 3].repeat_interleave(8)))
    keys = torch.stack([toff, roff], 1)[valid]
    cols = valid.nonzero().flatten()
    out = []
    for key in torch.unique(keys, dim=0):
        out.append(((int(key[0]), int(key[1])), cols[(keys == key).all(1)]))
    return out


def slice_errors(got, want, ktab, src_channels):
    """[(tap, relative error)] of a weight gradient [N, K] per (frame tap, row tap) slice of K: |got - want| over the slice against
    |want| over the slice + 1e-3 x the rms of the whole matrix x sqrt(elements of the slice) -- a wrong tap cannot hide in the norm"""
    rms = float(want.pow(2).mean().sqrt())
    out = []
    for key, cols in tap_slices(ktab, src_channels):
        cols = cols.to(got.device)
        g, w = got[:, cols], want[:, cols]
        out.append((key, float((g - w).norm() / (w.norm() + 1e-3 * rms * w.numel() ** 0.5 + 1e-300))))
    return out


# ---- a GemmSpec as plain tables (host side) -----------------------------------------------------------------------------------------
def plan_weights(spec, params):
    """[Npad, K] +-params[e] through the plan's pack entries, in params' own precision"""
    from sehip.plan import enc_entry
    return _term(params, enc_entry(spec.widx, spec.wneg))


def from_spec(st, spec, geom, B, T):
    """The plain arguments of gather_A / dst_index for one GemmSpec bound to buffers of geometry geom[name] = (Tst, F, C), as
    plan.DCCRNWorkspace._bind binds it (chunk table through plan.bind_chunk_table)."""
    from sehip.plan import bind_chunk_table
    kt = st.ktab.copy()
    bind_chunk_table(st.ktab, kt, spec.kt_off, spec.K // 8, [geom[b][1:] for b, _ in spec.srcs])
    tt = T if spec.tt == "T" else T + 1
    srcs = []
    for name, mode in spec.srcs:
        tst, f, c = geom[name]
        srcs.append((tst,) + ((1, T + 1) if mode == "drop1" else (0, tst)) + (f, c))
    dsts = []
    for name, toff, fmul, fadd in spec.dsts:
        tst, f, c = geom[name]
        dsts.append((tst, 1, f * c, toff, fmul, fadd, 1) if spec.J == 1 else (tst, f, c, toff, fmul, fadd, 1))
    return dict(M=B * tt * spec.J, N=spec.N, Npad=spec.Npad, K=spec.K, TT=tt, J=spec.J, fmul=spec.fmul, tmul=1,
                ktab=torch.from_numpy(kt[spec.kt_off:spec.kt_off + spec.K // 8].astype(np.int64)),
                ntab=torch.from_numpy(np.asarray(spec.ntab).reshape(-1, 4).astype(np.int64)), srcs=srcs, dsts=dsts)
