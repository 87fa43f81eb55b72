"""A host emulation of the C-ABI calls that sehip/plan_wavunet.py issues -- TEST INFRASTRUCTURE ONLY.

Every entry point the Wave-U-Net plan calls, restated in numpy on the RAW POINTERS the plan passes (CPU tensors have host addresses), from
the documented semantics of include/sehip.h: the packing / un-packing tables, the implicit-GEMM descriptor (chunk table, column table, two
sources, two destinations, bias, weight and bias gradient) and the csrc/wavunet.hip entry points written from their math.  With it the
plan's own forward() / backward() run on the CPU, so its wiring -- buffer names and levels, pointer offsets, bound tables, launch order --
is tested against the reference's vectors without a GPU (tests/test_wavunet_host.py).  bf16 stores round to nearest even as the kernels do.
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


def bf_put(ptr, a):
    u16(ptr, a.size)[:] = bf_round(a).reshape(-1)


def lrelu(o):
    return np.where(o > 0, o, 0.1 * o)


def _rows(d):
    """A [M][K] of a descriptor, gathered through its bound chunk table (J = 1, F = 1, frame stride 1)"""
    B, TT = d.M // d.TT, d.TT
    kt = i32(d.ktab, d.K // 8 * 4).reshape(-1, 4)
    A = np.zeros((d.M, d.K))
    b, t = np.divmod(np.arange(d.M), TT)
    for c, (s, packed, delta, _) in enumerate(kt):
        if s < 0:
            continue
        src = d.src[s]
        data = bf_get(src.ptr, B * src.T * src.C)
        toff = int(packed) >> 16
        ok = (t + toff >= src.tlo) & (t + toff < src.thi)
        base = (b * src.T + t) * src.C + int(delta)
        for e in range(8):
            A[ok, 8 * c + e] = data[base[ok] + e]
    return A


def _columns(d):
    """(destination, flat element index per row m) for every output column n < Npad, -1 where the column is padding"""
    nt = i32(d.ntab, d.Npad // 4 * 4).reshape(-1, 4)
    b, t = np.divmod(np.arange(d.M), d.TT)
    cols = []
    for n in range(d.Npad):
        q, coff, nvalid, _ = nt[n // 4]
        if n % 4 >= nvalid:
            cols.append(None)
            continue
        dst = d.dst[q]
        cols.append((q, (b * dst.T + t + dst.toff) * dst.C + coff + n % 4))
    return cols


class Emulator:
    def __init__(self):
        self.calls = []

    def __call__(self, name, *a):
        self.calls.append(name)
        getattr(self, name)(*a)

    # ---- tables ----------------------------------------------------------------------------------------------------
    def sehip_zero_regions(self, p0, b0, p1, b1, p2, b2, p3, b3, st):
        for p, n in ((p0, b0), (p1, b1), (p2, b2), (p3, b3)):
            if p and n:
                f32(p, n // 4)[:] = 0

    def sehip_pack_bf16(self, params, table, n, out, st):
        t = i32(table, n)
        v = np.where(t >= 0, f32(params, int(t.max() >> 1) + 1)[np.maximum(t, 0) >> 1], 0.0)
        bf_put(out, v)

    def sehip_pack_f32(self, params, table2, n, out, st):
        t = i32(table2, 2 * n).reshape(-1, 2)
        p = f32(params, int(t.max() >> 1) + 1)
        f32(out, n)[:] = sum(np.where(t[:, j] >= 0, p[np.maximum(t[:, j], 0) >> 1], 0.0) for j in range(2))

    def sehip_unpack_grad1(self, packed, table1, n, grads, st):
        t = i32(table1, n)
        g = f32(packed, int(t.max() >> 1) + 1)
        f32(grads, n)[:] = np.where(t >= 0, g[np.maximum(t, 0) >> 1], 0.0)

    # ---- products --------------------------------------------------------------------------------------------------
    def sehip_gemm(self, dref, st):
        d = C.cast(dref, C.POINTER(CGemmDesc)).contents
        out = _rows(d) @ bf_get(d.W, d.Npad * d.K).reshape(d.Npad, d.K).T
        if d.bias:
            out = out + f32(d.bias, d.Npad)
        B = d.M // d.TT
        for n, col in enumerate(_columns(d)):
            if col is not None:
                dst = d.dst[col[0]]
                u16(dst.ptr, B * dst.T * dst.C)[col[1]] = bf_round(out[:, n])

    def sehip_wgrad(self, dref, st):
        d = C.cast(dref, C.POINTER(CGemmDesc)).contents
        B = d.M // d.TT
        dout = np.zeros((d.M, d.Npad))
        for n, col in enumerate(_columns(d)):
            if col is not None:
                dst = d.dst[col[0]]
                dout[:, n] = bf_get(dst.ptr, B * dst.T * dst.C)[col[1]]
        f32(d.dW, d.Npad * d.K)[:] += (dout.T @ _rows(d)).reshape(-1).astype(np.float32)
        if d.dbias:
            f32(d.dbias, d.Npad)[:] += dout.sum(0).astype(np.float32)

    def sehip_stream_depend(self, *a):
        pass

    # ---- csrc/wavunet.hip, from the math ---------------------------------------------------------------------------
    def sehip_wun_enc0_fwd(self, x, W, bias, B, T, C0, y0, st):
        xp = np.pad(f32(x, B * T).astype(np.float64).reshape(B, T), ((0, 0), (7, 7)))
        w = f32(W, C0 * 15).astype(np.float64).reshape(C0, 15)
        win = np.stack([xp[:, k:k + T] for k in range(15)], -1)                # [B][T][15]
        bf_put(y0, win @ w.T + f32(bias, C0))

    def sehip_wun_enc0_wgrad(self, dy0, x, B, T, C0, dW, db, scratch, st):
        xp = np.pad(f32(x, B * T).astype(np.float64).reshape(B, T), ((0, 0), (7, 7)))
        win = np.stack([xp[:, k:k + T] for k in range(15)], -1).reshape(B * T, 15)
        g = bf_get(dy0, B * T * C0).reshape(B * T, C0)
        f32(dW, C0 * 15)[:] = (g.T @ win).reshape(-1)
        f32(db, C0)[:] = g.sum(0)

    def sehip_wun_bn_stats(self, y, rows, Cc, part, st):
        self._y_moments = (y, bf_get(y, rows * Cc).reshape(rows, Cc))

    def sehip_wun_bn_finalize(self, part, y, gamma, beta, rm, rv, nbt, rows, Cc, eps, momentum, training, coef, st):
        if training:
            assert self._y_moments[0] == y                                     # the statistics pass ran on this tensor
            v = self._y_moments[1]
            mean, var = v.mean(0), v.var(0)
            f32(rm, Cc)[:] = (1 - momentum) * f32(rm, Cc) + momentum * mean
            f32(rv, Cc)[:] = (1 - momentum) * f32(rv, Cc) + momentum * var * rows / (rows - 1)
            np.ctypeslib.as_array((C.c_int64 * 1).from_address(nbt))[0] += 1
        else:
            mean, var = f32(rm, Cc).astype(np.float64), f32(rv, Cc).astype(np.float64)
        rstd = 1 / np.sqrt(var + eps)
        sc = f32(gamma, Cc) * rstd
        f32(coef, 4 * Cc)[:] = np.stack([sc, f32(beta, Cc) - mean * sc, mean, rstd], 1).reshape(-1)

    def _z(self, y, coef, rows, Cc):
        k = f32(coef, 4 * Cc).astype(np.float64).reshape(Cc, 4)
        v = bf_get(y, rows * Cc).reshape(rows, Cc)
        return lrelu(k[:, 0] * v + k[:, 1]), v, k

    def sehip_wun_bn_apply(self, y, coef, rows, Cc, z, st):
        bf_put(z, self._z(y, coef, rows, Cc)[0])

    def sehip_wun_bn_apply_up2(self, y, coef, B, Tin, Cc, up, st):
        from sehip.plan_wavunet import up2_table
        z = self._z(y, coef, B * Tin, Cc)[0].reshape(B, Tin, Cc)
        i0, i1, w = up2_table(Tin)
        bf_put(up, z[:, i0] * (1 - w)[None, :, None] + z[:, i1] * w[None, :, None])

    def sehip_wun_up2_bwd(self, dup, B, Tin, Cc, dz, st):
        from sehip.plan_wavunet import up2_table
        g = bf_get(dup, B * 2 * Tin * Cc).reshape(B, 2 * Tin, Cc)
        i0, i1, w = up2_table(Tin)
        out = np.zeros((B, Tin, Cc))
        np.add.at(out, (slice(None), i0), g * (1 - w)[None, :, None])
        np.add.at(out, (slice(None), i1), g * w[None, :, None])
        bf_put(dz, out)

    def _g(self, dzf, dze, y, coef, rows, Cc):
        z, v, k = self._z(y, coef, rows, Cc)
        d = bf_get(dzf, rows * Cc).reshape(rows, Cc).copy()
        if dze:
            d[::2] += bf_get(dze, rows // 2 * Cc).reshape(rows // 2, Cc)
        return np.where(k[:, 0] * v + k[:, 1] > 0, d, 0.1 * d), (v - k[:, 2]) * k[:, 3], k

    def sehip_wun_bn_bwd_reduce(self, dzf, dze, y, coef, rows, Cc, part, st):
        g, xh, _ = self._g(dzf, dze, y, coef, rows, Cc)
        self._bwd_sums = (g.sum(0), (g * xh).sum(0))

    def sehip_wun_bn_bwd_finalize(self, part, coef, rows, Cc, dgamma, dbeta, bcoef, st):
        s0, s1 = self._bwd_sums
        f32(dbeta, Cc)[:] = s0
        f32(dgamma, Cc)[:] = s1
        k = f32(coef, 4 * Cc).reshape(Cc, 4)
        f32(bcoef, 4 * Cc)[:] = np.stack([k[:, 0], s0 / rows, s1 / rows, np.zeros(Cc)], 1).reshape(-1)

    def sehip_wun_bn_bwd_apply(self, dzf, dze, y, coef, bcoef, rows, Cc, dy, st):
        g, xh, _ = self._g(dzf, dze, y, coef, rows, Cc)
        kb = f32(bcoef, 4 * Cc).astype(np.float64).reshape(Cc, 4)
        bf_put(dy, kb[:, 0] * (g - kb[:, 1] - xh * kb[:, 2]))

    def sehip_wun_out_fwd(self, z, x, W, bias, rows, C0, out, st):
        w = f32(W, C0 + 1).astype(np.float64)
        f32(out, rows)[:] = np.tanh(bf_get(z, rows * C0).reshape(rows, C0) @ w[:C0] + w[C0] * f32(x, rows) + f32(bias, 1)[0])

    def sehip_wun_out_bwd(self, dout, out, z, x, W, rows, C0, dz, dW, db, scratch, st):
        o = f32(out, rows).astype(np.float64)
        dp = f32(dout, rows) * (1 - o * o)
        w = f32(W, C0 + 1).astype(np.float64)
        bf_put(dz, dp[:, None] * w[None, :C0])
        f32(dW, C0 + 1)[:] = np.concatenate([dp @ bf_get(z, rows * C0).reshape(rows, C0), [dp @ f32(x, rows)]])
        f32(db, 1)[0] = dp.sum()
