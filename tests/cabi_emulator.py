"""A host emulation of the C-ABI calls that the plans on sehip/prodgraph.py issue -- TEST INFRASTRUCTURE ONLY.

What the Wave-U-Net and the U-Net plan share, restated in float64 numpy on the RAW POINTERS the plans pass (CPU tensors have host
addresses), from the documented semantics of include/sehip.h: the packing / un-packing tables, the implicit-GEMM descriptor in its 2-D
form (chunk table with frame and row offsets, source strides tmul / fmul, column table, two sources, two destinations with the scatter
toff / tmul / fmul / fadd, bias, `res`, weight and bias gradient; the 1-D products are its J = 1, F = 1, stride 1 case) and the
BatchNorm statistics, records and backward records of csrc/clbn.h / csrc/wavunet.hip.  tests/wavunet_cabi_emulator.py and
tests/unet_cabi_emulator.py add their model's own entry points.

Two modes:
  * write (default): every call stores its result, bf16 stores round to nearest even as the kernels do.  With it a plan's own
    forward() / backward() run on the CPU, so its wiring is tested against the reference's vectors without a GPU;
  * check (Emulator(check=True)): the memory already holds what the device computed (a workspace copied back from the GPU).  Every call
    recomputes its result in float64 FROM THE OPERANDS THE KERNEL ITSELF READ and compares it with what is there instead of storing it;
    the findings are collected in .findings (stored bf16 tensors, fp32 sums against the sum of the absolute addends, exact values).
    Accumulated regions (weight / bias / BatchNorm gradients in the packed-gradient buffer) are summed into a shadow buffer and
    compared once, by finish().
"""
import ctypes as C

import numpy as np
import torch

from sehip.plan import CGemmDesc


def f32(ptr, n):
    return np.ctypeslib.as_array((C.c_float * int(n)).from_address(ptr))


def i32(ptr, n):
    return np.ctypeslib.as_array((C.c_int32 * int(n)).from_address(ptr))


def u16(ptr, n):
    return np.ctypeslib.as_array((C.c_uint16 * int(n)).from_address(ptr))


def bf_get(ptr, n):
    return (u16(ptr, n).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def bf_round(a):
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).bfloat16()
    return t.view(torch.int16).numpy().view(np.uint16)


def _rows(d):
    """A [M][K] of a descriptor, gathered through its bound chunk table"""
    TT, J = d.TT, d.J
    B = d.M // (TT * J)
    tmul, fmul = d.tmul or 1, d.fmul or 1
    kt = i32(d.ktab, d.K // 8 * 4).reshape(-1, 4)
    A = np.zeros((d.M, d.K))
    m = np.arange(d.M)
    j, bt = m % J, m // J
    t, b = bt % TT, bt // TT
    data = {}
    for c, (s, packed, delta, _) in enumerate(kt):
        if s < 0:
            continue
        src = d.src[s]
        if s not in data:
            data[s] = bf_get(src.ptr, B * src.T * src.F * src.C)
        toff = int(packed) >> 16
        foff = ((int(packed) & 0xFFFF) ^ 0x8000) - 0x8000
        tt, ff = t * tmul + toff, j * fmul + foff
        ok = (tt >= src.tlo) & (tt < src.thi) & (ff >= 0) & (ff < src.F)
        base = ((b * src.T + t * tmul) * src.F + j * fmul) * src.C + int(delta)
        for e in range(8):
            A[ok, 8 * c + e] = data[s][base[ok] + e]
    return A


def _columns(d):
    """(destination, flat element index per row m) for every output column n < Npad, None where the column is padding"""
    TT, J = d.TT, d.J
    nt = i32(d.ntab, d.Npad // 4 * 4).reshape(-1, 4)
    m = np.arange(d.M)
    j, bt = m % J, m // J
    t, b = bt % TT, bt // TT
    cols = []
    for n in range(d.Npad):
        q, coff, nvalid, _ = nt[n // 4]
        if n % 4 >= nvalid:
            cols.append(None)
            continue
        dst = d.dst[q]
        tm, fm = dst.tmul or 1, dst.fmul or 1
        tt, ff = t * tm + dst.toff, j * fm + dst.fadd
        assert (tt >= 0).all() and (tt < dst.T).all() and (ff >= 0).all() and (ff < dst.F).all(), "a destination row outside its tensor"
        cols.append((q, ((b * dst.T + tt) * dst.F + ff) * dst.C + coff + n % 4))
    return cols


class Emulator:
    ONE_ROUNDING_RMS = 1.65e-3
    SLOPE = None                # LeakyReLU's, the model's

    def __init__(self, check=False, gpack=None):
        """check mode: gpack = (pointer, floats) of the packed-gradient buffer the device filled"""
        self.calls, self.check, self.findings = [], check, []
        if check:
            self.gp_ptr, self.gp_n = gpack
            self.shadow, self.shadow_abs = np.zeros(self.gp_n), np.zeros(self.gp_n)

    def __call__(self, name, *a):
        self.calls.append(name)
        self._what = f"#{len(self.calls)} {name}"
        getattr(self, name)(*a)

    def lrelu(self, o):
        return np.where(o > 0, o, self.SLOPE * o)

    # ---- stores -------------------------------------------------------------------------------------------------------
    def _bf(self, ptr, want, idx=None, what=""):
        """store (write mode) or compare (check mode) a bf16 result; idx: flat element indices, else dense from ptr"""
        want = np.asarray(want, dtype=np.float64).reshape(-1)
        if not self.check:
            if idx is None:
                u16(ptr, want.size)[:] = bf_round(want)
            else:
                u16(ptr, int(idx.max()) + 1)[idx.reshape(-1)] = bf_round(want)
            return
        got = bf_get(ptr, want.size) if idx is None else bf_get(ptr, int(idx.max()) + 1)[idx.reshape(-1)]
        floor = 1e-3 * np.sqrt(np.mean(want ** 2))
        den = np.sqrt(np.sum(want ** 2))
        rms = float(np.sqrt(np.sum((got - want) ** 2)) / den) if den > 0 else float(np.abs(got).max())
        ideal_t = torch.from_numpy(want).float().bfloat16().double().numpy()
        ideal = float(np.sqrt(np.sum((ideal_t - want) ** 2)) / den) if den > 0 else 0.0
        ulp = float((np.abs(got - want) / (np.abs(want) + floor + 1e-300)).max())
        self.findings.append(dict(kind="stored", what=f"{self._what} {what}", rms=rms, ideal=ideal, ulp=ulp, n=want.size))

    def _sum(self, ptr, want, addends, what=""):
        """fp32 sums written once: store / compare against the sum of the absolute addends"""
        want = np.asarray(want, dtype=np.float64).reshape(-1)
        if not self.check:
            f32(ptr, want.size)[:] = want
            return
        got = f32(ptr, want.size).astype(np.float64)
        err = float((np.abs(got - want) / (np.asarray(addends, dtype=np.float64).reshape(-1) + 1e-30)).max())
        self.findings.append(dict(kind="sum", what=f"{self._what} {what}", err=err, n=want.size))

    def _acc(self, ptr, want, addends):
        """fp32 sums accumulated into the packed-gradient buffer"""
        want = np.asarray(want, dtype=np.float64).reshape(-1)
        if not self.check:
            f32(ptr, want.size)[:] += want.astype(np.float32)
            return
        off = (ptr - self.gp_ptr) // 4
        assert 0 <= off and off + want.size <= self.gp_n
        self.shadow[off:off + want.size] += want
        self.shadow_abs[off:off + want.size] += np.asarray(addends, dtype=np.float64).reshape(-1)

    def finish(self):
        """check mode: the packed-gradient buffer against the shadow sums, relative to the sum of the absolute addends"""
        got = f32(self.gp_ptr, self.gp_n).astype(np.float64)
        live = self.shadow_abs > 0
        err = float((np.abs(got - self.shadow)[live] / self.shadow_abs[live]).max())
        dead = float(np.abs(got[~live]).max()) if (~live).any() else 0.0
        self.findings.append(dict(kind="sum", what="packed gradients (dW, db, dgamma, dbeta)", err=err, n=int(live.sum())))
        self.findings.append(dict(kind="exact", what="packed-gradient entries nobody writes stay zero", bad=int(dead != 0.0)))

    # ---- tables ----------------------------------------------------------------------------------------------------
    def sehip_zero_regions(self, p0, b0, p1, b1, p2, b2, p3, b3, st):
        if self.check:
            return
        for p, n in ((p0, b0), (p1, b1), (p2, b2), (p3, b3)):
            if p and n:
                f32(p, n // 4)[:] = 0

    def sehip_pack_bf16(self, params, table, n, out, st):
        t = i32(table, n)
        v = np.where(t >= 0, f32(params, int(t.max() >> 1) + 1)[np.maximum(t, 0) >> 1], 0.0)
        self._bf(out, v, what="packed weights")

    def sehip_pack_f32(self, params, table2, n, out, st):
        t = i32(table2, 2 * n).reshape(-1, 2)
        if t.max() < 0:
            return
        p = f32(params, int(t.max() >> 1) + 1)
        v = sum(np.where(t[:, j] >= 0, p[np.maximum(t[:, j], 0) >> 1], 0.0) for j in range(2))
        self._sum(out, v, np.abs(v) + 1e-30, what="packed biases")

    def sehip_unpack_grad1(self, packed, table1, n, grads, st):
        t = i32(table1, n)
        g = f32(packed, int(t.max() >> 1) + 1)
        v = np.where(t >= 0, g[np.maximum(t, 0) >> 1], 0.0)
        self._sum(grads, v, np.abs(v) + 1e-30, what="flat gradients")

    def sehip_stream_depend(self, *a):
        pass

    # ---- products --------------------------------------------------------------------------------------------------
    def sehip_gemm(self, dref, st):
        d = C.cast(dref, C.POINTER(CGemmDesc)).contents
        out = _rows(d) @ bf_get(d.W, d.Npad * d.K).reshape(d.Npad, d.K).T
        if d.bias:
            out = out + f32(d.bias, d.Npad)
        cols = _columns(d)
        if d.res:
            dst = d.dst[0]
            res = bf_get(d.res, (d.M // (d.TT * d.J)) * dst.T * dst.F * dst.C)
        for q in range(2):
            sel = [(n, c[1]) for n, c in enumerate(cols) if c is not None and c[0] == q]
            if not sel:
                continue
            idx = np.stack([c for _, c in sel], 1)
            val = out[:, [n for n, _ in sel]]
            if d.res and q == 0:
                val = val + res[idx]
            self._bf(d.dst[q].ptr, val, idx=idx, what=f"destination {q}")

    def sehip_wgrad(self, dref, st):
        d = C.cast(dref, C.POINTER(CGemmDesc)).contents
        dout = np.zeros((d.M, d.Npad))
        for n, col in enumerate(_columns(d)):
            if col is not None:
                dst = d.dst[col[0]]
                dout[:, n] = bf_get(dst.ptr, int(col[1].max()) + 1)[col[1]]
        A = _rows(d)
        self._acc(d.dW, dout.T @ A, np.abs(dout).T @ np.abs(A))
        if d.dbias:
            self._acc(d.dbias, dout.sum(0), np.abs(dout).sum(0))

    # ---- BatchNorm statistics and records (csrc/clbn.h, csrc/wavunet.hip), from the math ---------------------------------
    def sehip_wun_bn_stats(self, y, rows, Cc, part, st):
        v = bf_get(y, rows * Cc).reshape(rows, Cc)
        self._y_moments = (y, v)
        nblk = self._nblk(rows, Cc)
        if not self.check:      # (all of it in the first workgroup's row)
            p = f32(part, nblk * 2 * Cc).reshape(nblk, 2, Cc)
            p[:] = 0
            p[0, 0], p[0, 1] = (v - v[0]).sum(0), ((v - v[0]) ** 2).sum(0)
        else:                   # the workgroups' partial rows, added: sums of deviations from the channel's first value
            p = f32(part, nblk * 2 * Cc).astype(np.float64).reshape(nblk, 2, Cc)
            dv = v - v[0]
            for a, (want, addends) in enumerate(((dv.sum(0), np.abs(dv).sum(0)), ((dv * dv).sum(0), (dv * dv).sum(0)))):
                err = float((np.abs(p[:, a].sum(0) - want) / (addends + 1e-30)).max())
                self.findings.append(dict(kind="sum", what=f"{self._what} moment {a + 1}", err=err, n=Cc))

    @staticmethod
    def _nblk(rows, Cc):
        from sehip import _lib
        return int(_lib.lib().sehip_wun_bn_scratch_floats(rows, Cc)) // (2 * Cc)

    def _bn_finalize(self, part, y, gamma, beta, rm, rv, nbt, rows, Cc, Cr, eps, momentum, training, coef):
        """the records of the first Cr channels; the padding channels' are exact zeros"""
        if training:
            assert self._y_moments[0] == y                                     # the statistics pass ran on this tensor
            v = self._y_moments[1][:, :Cr]
            mean, var = v.mean(0), v.var(0)
            if not self.check:
                f32(rm, Cr)[:] = (1 - momentum) * f32(rm, Cr) + momentum * mean
                f32(rv, Cr)[:] = (1 - momentum) * f32(rv, Cr) + momentum * var * rows / (rows - 1)
                np.ctypeslib.as_array((C.c_int64 * 1).from_address(nbt))[0] += 1
            dev = np.abs(v - v[0]).mean(0)
        else:
            mean, var = f32(rm, Cr).astype(np.float64), f32(rv, Cr).astype(np.float64)
            dev = np.abs(mean)
        rstd = 1 / np.sqrt(var + eps)
        sc = f32(gamma, Cr) * rstd
        want = np.zeros((Cc, 4))
        want[:Cr] = np.stack([sc, f32(beta, Cr) - mean * sc, mean, rstd], 1)
        if not self.check:
            f32(coef, 4 * Cc)[:] = want.reshape(-1)
            return
        got = f32(coef, 4 * Cc).astype(np.float64).reshape(Cc, 4)
        tol = np.zeros((Cc, 4))
        tol[:Cr] = 1e-5 * np.abs(want[:Cr]) + 1e-5 * np.stack([np.abs(sc), np.abs(mean * sc) + np.abs(f32(beta, Cr)), dev, rstd], 1)
        bad = int((np.abs(got - want) > tol).sum())
        self.findings.append(dict(kind="exact", what=f"{self._what} coefficient records within 1e-5 (padding records exact zeros)", bad=bad))

    def sehip_wun_bn_bwd_finalize(self, part, coef, rows, Cc, dgamma, dbeta, bcoef, st):
        """after the model's bwd_reduce, which leaves _bwd_sums = (sum g, sum g xh, sum |g|, sum |g xh|) per channel"""
        s0, s1, a0, a1 = self._bwd_sums
        self._acc(dbeta, s0, a0)
        self._acc(dgamma, s1, a1)
        k = f32(coef, 4 * Cc).reshape(Cc, 4)
        want = np.stack([k[:, 0], s0 / rows, s1 / rows, np.zeros(Cc)], 1)
        self._sum(bcoef, want, np.stack([np.abs(k[:, 0]), a0 / rows, a1 / rows, np.ones(Cc)], 1) + 1e-30, what="backward records")
