"""The engine of tests/test_gpu_dccrn_products.py, and its child process for the run with forced tile switches.

One DCCRN train step at the headline widths with EVERY product launch (sehip_gemm, sehip_gemm_pair, sehip_wgrad, sehip_wgrad_pair,
sehip_wgrad_group, sehip_wgrad_dense_group) intercepted at the call and compared, at that moment, with tests/desc_ref.py evaluated
in float64 on the operands the descriptor passed to the call points at -- later launches reuse workspace memory.  Order per launch:
synchronise, snapshot every output (destinations, dW / dbias, stats, bnr_part), let the call run, synchronise, read sehip_last_kernel,
compare.  Failures are collected, not raised (the calls sit inside autograd's backward); the caller asserts on the report.

As a program: `python dccrn_products_worker.py B LENGTH` runs one such step and prints ONE JSON object (the report) as its last line.
The switches that are read once per process (SEHIP_C3_TM, SEHIP_C3_PAIR_TM, SEHIP_CT_CHUNKS, SEHIP_BNR_CHUNKS) come in through the
environment: that is why this run needs a process of its own."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "speech-enhancement-pytorch_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

import desc_ref as D  # noqa: E402
from test_gpu_demucs_fullwidth import OUT_TOL, ULP_TOL, F32_TOL, out_err, rel  # noqa: E402  (imported, not copied)

KW = dict(kernel_num=[16, 32, 64, 128, 256, 256], rnn_units=128)
PRODUCT_CALLS = ("sehip_gemm", "sehip_gemm_pair", "sehip_wgrad", "sehip_wgrad_pair", "sehip_wgrad_group", "sehip_wgrad_dense_group")
# fp32 sums against float64: |got - want| <= SUM_FACTOR * 2^-24 * sqrt(n) * sum |addend| (tests/test_desc_ref_host.py shows that one
# missing row fails this at these shapes), never above the any-order ceiling (n + 1) * 2^-24 * sum |addend|
SUM_FACTOR = 4.0
# Kernels that stage the product tile (+ bias) in LDS as bf16 and add the residual `res` to THAT, rounding a second time (csrc/conv3.hip
# pair epilogue, csrc/convt.hip store phase): the two kernels that carry `res` in the four runs, and no other.  Their launches with `res`
# are held to desc_ref.out_err2 -- one bf16 ulp of |product| + |sum| -- with the same constants.  Every other kernel that meets `res` is
# held to the plain gate (gemm_pair_kernel adds `res` to the fp32 accumulator: dx1_r + dx1_i), and so is a launch with `res` AND `stats`:
# conv_gemm_v3's dense path with both adds `res` in fp32 before it stages the tile, which is one rounding.
RES_AFTER_BF16 = {"conv_gemm_v3_pair_kernel", "convt_stream_kernel"}


# ---- the gates (tests/test_desc_ref_host.py shows on the reference side that each rejects a subtly wrong result) ---------------------
def gate_bf16(got, want, prod=None):
    """(ok, rms, max) of a bf16 destination; prod: the product (+ bias) of a launch that rounds it before adding `res` (RES_AFTER_BF16)"""
    e, u = out_err(got, want) if prod is None else D.out_err2(got, want, prod)
    return e < OUT_TOL and u < ULP_TOL, e, u


def gate_f32(got, want):
    e = rel(got, want)
    return e < F32_TOL, e


def gate_dw(got, want, ktab, src_channels):
    """(ok, whole-matrix error, (tap, error) of the worst slice, slices): F32_TOL over the whole matrix AND over every (frame tap, row
    tap) slice of K"""
    e = rel(got, want)
    sl = D.slice_errors(got, want, ktab, src_channels)
    worst = max(sl, key=lambda t: t[1])
    return e < F32_TOL and worst[1] < F32_TOL, e, worst, len(sl)


def gate_sum(got, want, n, mag, slack=0.0):
    """(ok, worst |got - want| in units of 2^-24 sqrt(n) sum |addend|: SUM_FACTOR is the gate) of fp32 sums of n addends"""
    err = (got - want).abs() - slack
    ratio = float((err / (D.EPS24 * n ** 0.5 * mag + 1e-300)).max())
    return bool((err <= D.sum_bound(n, mag, SUM_FACTOR)).all()), ratio


def base_name(kernel):
    return kernel.split("<")[0].split("(")[0].replace("void ", "").strip()


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


class Checker:
    def __init__(self, model, ws):
        from sehip import _lib
        self.model, self.ws, self.st, self.lib = model, ws, ws.st, _lib.lib()
        self.params = model.flat_params.detach()
        r = self.res = D.Resolver()
        for name, b in ws.bufs.items():
            r.add(name, b.t)
        for name, t in (("gpack", ws.gpack), ("bn_stats_all", ws.bn_stats_all), ("bn_acc", ws.bn_acc), ("bn_bcoef", ws.bn_bcoef),
                        ("wpack", ws.tb.wpack), ("bpack", ws.tb.bpack), ("ktab", ws.ktab_dev), ("ntab", ws.tb.ntab), ("params", self.params)):
            r.add(name, t)
        for pre, t in ws.bn_coef.items():
            r.add("bn_coef." + pre, t)
        self.launches, self.failures = [], []
        self.intercepted = self.compared = 0
        self.bias_got, self.bias_want, self.bias_names = {}, {}, {}
        self.bnr_expected, self.bnr_compared = [], []
        self.bn_dz_bias = None
        self._wexp = {}

    # ---- bookkeeping ---------------------------------------------------------------------------------------------------------------
    def fail(self, label, what, *figs):
        self.failures.append([label, what] + [float(f) if isinstance(f, (int, float)) else str(f) for f in figs])

    def name_of(self, d):
        addr = C.addressof(d)
        for name, x in self.ws.desc.items():
            if C.addressof(x) == addr:
                return name
        for (name, t0, t1), x in self.ws._chunk_cache.items():
            if C.addressof(x) == addr:
                return name
        raise KeyError("a product launch with a descriptor the workspace does not know")

    def group_names(self, buf_ptr):
        for names, (buf, n, total, dense) in self.ws._wg_groups.items():
            if buf.data_ptr() == buf_ptr or (dense is not None and dense[0].data_ptr() == buf_ptr):
                return list(names)
        raise KeyError("a grouped weight-gradient launch the workspace does not know")

    def table(self, ptr, n):
        _, t, off = self.res.find(ptr)
        return t[off:off + 4 * n].view(n, 4).to(torch.int64)

    def hook(self, orig):
        def call(fn, *args):
            if fn not in PRODUCT_CALLS:
                return orig(fn, *args)
            self.intercepted += 1
            if fn in ("sehip_gemm", "sehip_wgrad"):
                descs = [args[0]._obj]
            elif fn in ("sehip_gemm_pair", "sehip_wgrad_pair"):
                descs = [args[0]._obj, args[1]._obj]
            else:
                descs = [self.ws.desc[nm + ".wg"] for nm in self.group_names(args[0])]
            named = [(self.name_of(d), d) for d in descs]
            label = "+".join(n for n, _ in named) if len(named) <= 2 else f"lstm.wg[{len(named)}]"
            torch.cuda.synchronize()
            snap = self.snapshot(fn, descs)
            orig(fn, *args)
            torch.cuda.synchronize()
            kernel = self.lib.sehip_last_kernel().decode()
            figs = {}
            try:
                if fn.startswith("sehip_gemm"):
                    self.check_gemm(label, named, snap, kernel, figs)
                else:
                    self.check_wgrad(label, named, snap, kernel, figs)
                self.compared += 1
            except Exception as e:      # a reference-side error is a failure of this launch, not of the step
                self.fail(label, "exception", repr(e))
            self.launches.append(dict(label=label, fn=fn, kernel=kernel, figs=figs))
        return call

    def snapshot(self, fn, descs):
        snap = {}

        def keep(ptr):
            if ptr:
                name, t, _ = self.res.find(ptr)
                if name not in snap:
                    snap[name] = t.clone()
        for d in descs:
            if fn.startswith("sehip_gemm"):
                for q in range(2):
                    keep(d.dst[q].ptr)
                keep(d.stats)
                keep(d.bnr_part)
            else:
                keep(d.dW)
                keep(d.dbias)
        return snap

    # ---- operands ------------------------------------------------------------------------------------------------------------------
    def operands(self, d):
        srcs = []
        for q in range(4):
            s = d.src[q]
            if not s.ptr:
                break
            srcs.append((self.res.view(s.ptr), s.T, s.tlo, s.thi, s.F, s.C))
        ktab = self.table(d.ktab, d.K // 8)
        ntab = self.table(d.ntab, d.Npad // 4)
        A = D.gather_A(srcs, ktab, d.M, d.K, d.TT, d.J, d.fmul, d.tmul)
        geo = lambda x: (x.T, x.F, x.C, x.toff, x.fmul, x.fadd, x.tmul)
        dsts = [geo(d.dst[0])] + ([geo(d.dst[1])] if d.dst[1].ptr else [])
        idx = D.dst_index(dsts, ntab, d.M, d.N, d.Npad, d.TT, d.J)
        return srcs, ktab, A, idx

    def weights(self, label, name, d):
        """float64 [N, K] and bias [N]: the EXPECTED bf16 weights through the plan's pack entries; the packed buffer (un-tiled as sehip.h
        words the order when w_tiled is set) must hold exactly those bits -- a wrong tile order fails here, not as a product error"""
        spec = self.st.specs[name]
        if name not in self._wexp:
            self._wexp[name] = (D.expected_weights(spec, self.params), D.expected_bias(spec, self.params))
        wexp, bexp = self._wexp[name]
        packed = self.res.view(d.W)[:d.Npad * d.K]
        if d.w_tiled:
            cs = spec.v3_channels()
            packed = D.untile_w(packed, d.Npad, d.K, d.cv_nf, cs[0] + cs[1])
        if not torch.equal(_bits(packed.reshape(d.Npad, d.K).contiguous()), _bits(wexp.contiguous())):
            self.fail(label, "packed weights differ from bf16(+-params) through the pack entries" + (" (w_tiled)" if d.w_tiled else ""), name)
        bias = None
        if d.bias:
            bias = bexp[:d.N]
            e = rel(self.res.view(d.bias)[:d.N], bias)
            if not e < 1e-6:
                self.fail(label, "packed bias", e)
        return wexp[:d.N].double(), bias

    def by_channel(self, ptr, cols, idx, width):
        """[M, width] float64: the tensor at ptr (laid out like the destination) gathered at idx, columns put at their destination
        channel"""
        v = self.res.view(ptr)[idx].double()
        out = torch.zeros(idx.shape[0], width, dtype=torch.float64, device=v.device)
        out[:, cols] = v
        return out

    # ---- forward / input-gradient products -----------------------------------------------------------------------------------------
    def check_gemm(self, label, named, snap, kernel, figs):
        kb = base_name(kernel)
        addressed = {}
        stats_parts, bnr = [], None
        for name, d in named:
            srcs, ktab, A, idx = self.operands(d)
            W, bias = self.weights(label, name, d)
            prod = A @ W.t()
            if bias is not None:
                prod = prod + bias[None, :]
            for q, (cols, dcol, ix) in idx.items():
                tname, flat, off = self.res.find(d.dst[q].ptr)
                got = flat[off + ix]
                addressed.setdefault(tname, torch.zeros(flat.numel(), dtype=torch.bool, device=flat.device))[(off + ix).reshape(-1)] = True
                want = prod[:, cols]
                if d.dst[q].is_f32:
                    ok, e = gate_f32(got, want)
                    figs[f"{name}.f32"] = e
                    if not ok:
                        self.fail(label, "fp32 destination", name, e)
                    continue
                if d.res and q == 0:
                    r = self.res.view(d.res)[ix].double()
                    twice = kb in RES_AFTER_BF16 and not d.stats
                    ok, e, u = gate_bf16(got, want + r, want if twice else None)
                    figs[f"{name}.res2"] = float(twice)
                else:
                    ok, e, u = gate_bf16(got, want)
                figs[f"{name}.rms"], figs[f"{name}.ulp"] = e, u / 2 ** -8
                if not ok:
                    self.fail(label, "bf16 destination", name, e, u / 2 ** -8)
            if d.stats:
                cols, dcol, ix = idx[0]
                stats_parts.append((d, self.by_channel(d.dst[0].ptr, dcol, ix, d.dst[0].C)))
            if d.bnr_part and d.bnr_y and d.bnr_coef and d.bnr_slope and self.lib.sehip_bnr_rows(C.byref(d), None) > 0:
                self.bnr_expected.append(name)       # the descriptor carries the operands and the library says the launch honours them
                bnr = (name, d, idx[0])
        # stray writes: what no descriptor of this launch addresses keeps its bits
        for tname, mask in addressed.items():
            flat = self.res.by_name(tname)
            same = _bits(flat) == _bits(snap[tname])
            n_bad = int((~same & ~mask).sum())
            figs[f"stray.{tname}"] = n_bad
            if n_bad:
                self.fail(label, "stray writes", tname, n_bad)
        if stats_parts:
            self.check_stats(label, stats_parts, snap, figs)
        if bnr is not None:
            self.check_bnr(label, *bnr, figs)

    def sum_gate(self, label, what, got, want, n, mag, slack, figs):
        """the ratio reported is |got - want| / (2^-24 sqrt(n) sum |addend|): the gate is SUM_FACTOR"""
        ok, ratio = gate_sum(got, want, n, mag, slack)
        figs[what] = max(ratio, figs.get(what, 0.0))
        if not ok:
            self.fail(label, what, ratio, n)

    def check_stats(self, label, parts, snap, figs):
        d = parts[0][0]
        cr = d.stats_cr
        name, flat, off = self.res.find(d.stats)
        after = flat[off:off + 40 * cr].double().view(8, 5, cr)
        before = snap[name][off:off + 40 * cr].double().view(8, 5, cr)
        got = (after - before).sum(0)
        y = torch.cat([p[1] for p in parts])                 # the bf16 values the launch stored, [rows, 2 cr]
        re, im = y[:, :cr], y[:, cr:]
        adds = [re, im, re * re, re * im, im * im]
        want = torch.stack([a.sum(0) for a in adds])
        mag = torch.stack([a.abs().sum(0) for a in adds])
        self.sum_gate(label, "stats", got, want, y.shape[0], mag, 0.0, figs)

    def check_bnr(self, label, name, d, idx0, figs):
        cols, dcol, ix = idx0
        cr = d.dst[0].C // 2
        rows = int(self.lib.sehip_bnr_rows(C.byref(d), None))
        dz = self.by_channel(d.dst[0].ptr, dcol, ix, 2 * cr)          # the values the launch stored
        y = self.by_channel(d.bnr_y, dcol, ix, 2 * cr)
        coef = self.res.view(d.bnr_coef)[:16 * cr].view(cr, 16)
        slope = float(self.res.view(d.bnr_slope)[0])
        part = self.res.view(d.bnr_part)[:rows * (6 * cr + 1)].double().view(rows, 6 * cr + 1).sum(0)
        sums, sl, mags, sl_mag, slack, sl_slack = D.bn_reduce_sums(dz, y, coef, slope)
        self.sum_gate(label, "bnr_part", part[:6 * cr].view(6, cr), sums, dz.shape[0], mags, slack, figs)
        self.sum_gate(label, "bnr_part", part[6 * cr:], sl.reshape(1), 2 * cr * dz.shape[0], sl_mag.reshape(1), sl_slack.reshape(1), figs)
        self.bnr_compared.append(name)
        figs["bnr_rows"] = rows

    # ---- weight gradients ----------------------------------------------------------------------------------------------------------
    def check_wgrad(self, label, named, snap, kernel, figs):
        gname, gflat, _ = self.res.find(named[0][1].dW)
        before = snap[gname]
        written = torch.zeros(gflat.numel(), dtype=torch.bool, device=gflat.device)
        for name, d in named:
            srcs, ktab, A, idx = self.operands(d)
            assert list(idx) == [0], "dOut is addressed through destination 0"
            cols, dcol, ix = idx[0]
            dO = torch.zeros(d.M, d.Npad, dtype=torch.float64, device=A.device)
            if d.bn_dz:
                # narrow_wgrad_mfma_kernel<5, 2, true> computes dOut = the BatchNorm + PReLU backward value from bn_dz / bn_y and the
                # records IN FLOAT32, ROUNDS IT TO bf16 (pack_bf2, as sehip_cbn_bwd_apply would store it) and multiplies that.  The
                # reference does the same: the value evaluated as float32 arithmetic in the order of the kernel's source expression
                # (desc_ref.bn_apply_f32, "lhs"; within float32 rounding of the float64 value, tests/test_desc_ref_host.py), then
                # rounded to bf16.  Rounding the float64 value instead puts a few elements of 264 192 on the other side of a bf16 tie,
                # and ONE such element of a large row is 3e-5 of its tap slice (measured: 2e-6 ... 2e-5 that way, 2e-7 this way).
                cr = d.dst[0].C // 2
                coef = self.res.view(d.bn_coef)[:16 * cr].view(cr, 16)
                bcoef = self.res.view(d.bn_bcoef)[:16 * cr].view(cr, 16)
                dy = D.bn_apply_f32(self.by_channel(d.bn_dz, dcol, ix, 2 * cr), self.by_channel(d.bn_y, dcol, ix, 2 * cr), coef, bcoef,
                                    float(self.res.view(d.bn_slope)[0]), "lhs")
                dO[:, cols] = D.round_bf16(dy)[:, dcol]
                figs[f"{name}.bn_dz"] = 1.0
            else:
                _, flat, off = self.res.find(d.dst[0].ptr)
                dO[:, cols] = flat[off + ix].double()
            want = dO.t() @ A                                              # [Npad, K], zero rows beyond N
            _, _, woff = self.res.find(d.dW)
            written[woff:woff + d.Npad * d.K] = True
            got = (gflat[woff:woff + d.Npad * d.K].double() - before[woff:woff + d.Npad * d.K].double()).view(d.Npad, d.K)
            ok, e, worst, nsl = gate_dw(got, want, ktab, [s[5] for s in srcs])
            figs[f"{name}.dW"], figs[f"{name}.dW_slice"], figs[f"{name}.slices"] = e, worst[1], nsl
            if d.bn_dz:
                figs[f"{name}.bn_dz_dW"] = max(e, worst[1])
            if not ok:
                self.fail(label, "dW", name, e, str(worst[0]), worst[1])
            if d.dbias:
                _, _, boff = self.res.find(d.dbias)
                written[boff:boff + d.Npad] = True
                g = gflat[boff:boff + d.N].double() - before[boff:boff + d.N].double()
                self.bias_got[boff] = self.bias_got.get(boff, 0) + g
                self.bias_want[boff] = self.bias_want.get(boff, 0) + dO[:, :d.N].sum(0)
                self.bias_names.setdefault(boff, []).append(name)
                if d.bn_dz:
                    self.bn_dz_bias = boff
        n_bad = int(((_bits(gflat) != _bits(before)) & ~written).sum())
        figs["stray.gpack"] = n_bad
        if n_bad:
            self.fail(label, "stray writes", "gpack", n_bad)

    def finish(self):
        """dbias within 5 * F32_TOL, summed over the launches that share one bias"""
        out = []
        for boff, want in self.bias_want.items():
            e = rel(self.bias_got[boff], want)
            out.append(("+".join(self.bias_names[boff]), e))
            if boff == self.bn_dz_bias:
                self.bn_dz_dbias = e
            if not e < 5 * F32_TOL:
                self.fail("bias of " + "+".join(self.bias_names[boff]), "dbias", e)
        return out


def run_step(B, length, deterministic=False, fuse_enc0=False, patch=None):
    """One intercepted train step; returns the report (a JSON-able dict).  patch(obj, name, value): how attributes are replaced
    (pytest's monkeypatch.setattr in the test process; the child process sets and restores them itself).  `call` is wrapped where the
    plan looks it up: sehip.plan.call, and sehip.workspace.call for the launches GemmWorkspace issues (gemm())."""
    from sehip import plan, workspace
    from sehip.model import DCCRN
    from sehip.utils import set_deterministic
    undo = []
    if patch is None:
        def patch(obj, name, value):
            undo.append((obj, name, getattr(obj, name)))
            setattr(obj, name, value)
    old = os.environ.get("SEHIP_NO_SIDE_STREAM")
    os.environ["SEHIP_NO_SIDE_STREAM"] = "1"        # (read when the workspace is built: arithmetic, not the two-queue schedule)
    try:
        if deterministic:
            set_deterministic(True)
        if fuse_enc0:
            patch(plan, "FUSE_ENC0_BN_WGRAD", True)
        torch.manual_seed(5)
        model = DCCRN(length=length, **KW).to(torch.device("cuda:0")).train()
        g = torch.Generator().manual_seed(6)
        with torch.no_grad():        # the terms the constructors leave at zero: every bias path carries a value
            L = model.static.layout
            for name in L.param_names:
                if name.endswith(("conv.bias", "1.Br", "1.Bi")):
                    off, shape = L.param_off[name]
                    n = 1
                    for s in shape:
                        n *= s
                    model.flat_params[off:off + n] = (0.1 * torch.randn(n, generator=g)).to(model.flat_params.device)
        if deterministic:
            model.set_deterministic(True)
        ws = model.workspace(B, length)
        assert ws.side is None
        chk = Checker(model, ws)
        patch(plan, "call", chk.hook(plan.call))
        patch(workspace, "call", chk.hook(workspace.call))
        x = (0.1 * torch.randn(B, 1, length, generator=g)).cuda()
        out = model(x)
        G = torch.randn(out.shape, generator=g) / out.numel() ** 0.5
        out.backward(G.cuda())
        torch.cuda.synchronize()
        assert model.workspace(B, length) is ws
        bias = chk.finish()
    finally:
        for obj, name, value in reversed(undo):
            setattr(obj, name, value)
        if deterministic:
            set_deterministic(False)
        if old is None:
            os.environ.pop("SEHIP_NO_SIDE_STREAM", None)
        else:
            os.environ["SEHIP_NO_SIDE_STREAM"] = old
    return dict(T=int(ws.T), intercepted=chk.intercepted, compared=chk.compared, launches=chk.launches, failures=chk.failures, bias=bias,
                enc0_bn_in_wgrad=bool(ws.enc0_bn_in_wgrad), bnr=sorted(name for _, name in ws.bnr_rows.values()),
                bnr_expected=sorted(chk.bnr_expected), bnr_compared=sorted(chk.bnr_compared), bn_dz_dbias=getattr(chk, "bn_dz_dbias", None))


def worst(report):
    """the figures the test prints: worst of each kind with its launch"""
    w = {}
    for la in report["launches"]:
        for k, v in la["figs"].items():
            kind = k.split(".")[-1] if "." in k else k
            if kind in ("rms", "ulp", "f32", "dW", "dW_slice", "stats", "bnr_part", "bn_dz_dW"):
                if v >= w.get(kind, (-1.0, ""))[0]:
                    w[kind] = (v, la["label"] if kind in ("stats", "bnr_part") else k.rsplit(".", 1)[0])
    if report["bias"]:
        n, e = max(report["bias"], key=lambda t: t[1])
        w["dbias"] = (e, n)
    return w


def summary(tag, report):
    w = worst(report)
    f = lambda k: f"{w[k][0]:.2e} ({w[k][1]})" if k in w else "none"
    return (f"DCCRN products [{tag}] T = {report['T']}: {report['compared']} of {report['intercepted']} launches compared, "
            f"{len(set(la['kernel'] for la in report['launches']))} kernel instantiations; worst bf16 rms {f('rms')}, ulp {f('ulp')}; fp32 {f('f32')}; "
            f"dW {f('dW')}, dW slice {f('dW_slice')}; dbias {f('dbias')}; stats {f('stats')} and bnr_part {f('bnr_part')} of the "
            f"{SUM_FACTOR:g} allowed (units of 2^-24 sqrt(n) sum|addend|)"
            + (f"; bn_dz weight gradient: dW / worst slice {f('bn_dz_dW')}, its dbias {report['bn_dz_dbias']:.2e}"
               if "bn_dz_dW" in w else ""))


if __name__ == "__main__":
    rep = run_step(int(sys.argv[1]), int(sys.argv[2]))
    print(summary("child", rep), file=sys.stderr)
    print(json.dumps(rep))
