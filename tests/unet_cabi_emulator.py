"""A host emulation of the C-ABI calls that sehip/plan_unet.py issues -- TEST INFRASTRUCTURE ONLY.

tests/cabi_emulator.py (the tables, the products in their 2-D form, the BatchNorm statistics and records, the write and the check mode)
plus the csrc/unet.hip entry points written from their math in float64: LeakyReLU(0.01), the two dropout sites, the fused MaxPool2d(2)
with its argmax codes.  Write mode runs the plan's own forward() / backward() on the CPU (tests/test_unet_host.py); check mode
recomputes every launch from the operands the kernel itself read, over a workspace copied back from the GPU (tests/test_gpu_unet.py).
"""
import ctypes as C

import numpy as np

import cabi_emulator
from cabi_emulator import bf_get, f32, u16
from unet_ref import drop_keep_mask


class Emulator(cabi_emulator.Emulator):
    SLOPE = 0.01

    def sehip_rsm_counter_next(self, counter, used, st):
        if self.check:
            return
        c = np.ctypeslib.as_array((C.c_uint64 * 1).from_address(counter))
        np.ctypeslib.as_array((C.c_uint32 * 1).from_address(used))[0] = int(c[0]) & 0xFFFFFFFF
        c[0] += 1

    # ---- csrc/unet.hip, from the math -------------------------------------------------------------------------------------
    def _spec(self, ptr, R, uc, F, T):
        return f32(ptr, R * uc * F * T * 2).astype(np.float64).reshape(R, uc, F, T, 2)

    def _padded_cl(self, v, Cp):
        """[R, uc, F, T] -> channels-last [R][T][F][Cp] with zero padding channels"""
        R, uc, F, T = v.shape
        out = np.zeros((R, T, F, Cp))
        out[..., :uc] = v.transpose(0, 3, 2, 1)
        return out

    def sehip_unet_features(self, spec, R, uc, F, T, Cp, amp, st):
        z = self._spec(spec, R, uc, F, T)
        self._bf(amp, self._padded_cl(z[..., 0] ** 2 + z[..., 1] ** 2, Cp), what="amp")

    def sehip_unet_mask_bwd(self, dout, spec, R, uc, F, T, Cp, dm, st):
        z, g = self._spec(spec, R, uc, F, T), self._spec(dout, R, uc, F, T)
        self._bf(dm, self._padded_cl(g[..., 0] * z[..., 0] + g[..., 1] * z[..., 1], Cp), what="dm")

    def sehip_unet_mask_fwd(self, y, coef, spec, R, uc, F, T, Cp, out, st):
        k = f32(coef, 4 * Cp).astype(np.float64).reshape(Cp, 4)
        v = bf_get(y, R * T * F * Cp).reshape(R, T, F, Cp)
        pre = k[:, 0] * v + k[:, 1]
        m = self.lrelu(pre)[..., :uc].transpose(0, 3, 2, 1)                               # [R, uc, F, T]
        mabs = (np.where(pre > 0, 1.0, self.SLOPE) * (np.abs(k[:, 0] * v) + np.abs(k[:, 1])))[..., :uc].transpose(0, 3, 2, 1)
        z = self._spec(spec, R, uc, F, T)
        self._sum(out, z * m[..., None], np.abs(z) * mabs[..., None] + 1e-30, what="out")

    def sehip_unet_bn_finalize(self, part, y, gamma, beta, rm, rv, nbt, rows, Cc, Cr, eps, momentum, training, coef, st):
        self._bn_finalize(part, y, gamma, beta, rm, rv, nbt, rows, Cc, Cr, eps, momentum, training, coef)

    def _keep(self, n, seed_lo, seed_hi, ctr, layer, thresh):
        if not thresh:
            return np.ones(n)
        counter = int(np.ctypeslib.as_array((C.c_uint32 * 1).from_address(ctr))[0])
        return drop_keep_mask((int(seed_hi) << 32) | int(seed_lo), counter, layer, n, thresh / float(1 << 24)).astype(np.float64)

    def _z(self, y, coef, rows, Cc, drop):
        """(z after dropout, keep x scale, pre-activation, y, coef) of a full-resolution tensor"""
        seed_lo, seed_hi, ctr, layer, thresh, scale = drop
        k = f32(coef, 4 * Cc).astype(np.float64).reshape(Cc, 4)
        v = bf_get(y, rows * Cc).reshape(rows, Cc)
        pre = k[:, 0] * v + k[:, 1]
        ks = np.ones((rows, Cc))
        if thresh:
            ks = self._keep(rows * Cc, seed_lo, seed_hi, ctr, layer, thresh).reshape(rows, Cc) * float(np.float32(scale))
        return self.lrelu(pre) * ks, ks, pre, v, k

    def sehip_unet_bn_act(self, y, coef, rows, Cc, seed_lo, seed_hi, ctr, layer, thresh, scale, z, st):
        self._bf(z, self._z(y, coef, rows, Cc, (seed_lo, seed_hi, ctr, layer, thresh, scale))[0], what="z")

    @staticmethod
    def _windows(a, R, T, F, Cc):
        """[R T F][C] -> candidates [4][R][T/2][F/2][C] in the order code = 2 (F offset) + (T offset)"""
        a = a.reshape(R, T, F, Cc)[:, :T // 2 * 2, :F // 2 * 2]
        return np.stack([a[:, dt::2, df::2] for df in (0, 1) for dt in (0, 1)], 0)

    def sehip_unet_bn_act_pool(self, y, coef, R, T, F, Cc, seed_lo, seed_hi, ctr, layer, thresh, scale, zp, code, st):
        z = self._z(y, coef, R * T * F, Cc, (seed_lo, seed_hi, ctr, layer, thresh, scale))[0]
        cand = self._windows(z, R, T, F, Cc)
        best, cd = cand[0].copy(), np.zeros(cand[0].shape, dtype=np.int64)
        for k in (1, 2, 3):
            m = cand[k] > best
            best[m], cd[m] = cand[k][m], k
        self._bf(zp, best, what="pooled z")
        words = (cd.reshape(-1, Cc // 8, 8) << (2 * np.arange(8))).sum(-1).astype(np.uint16).reshape(-1)
        if not self.check:
            u16(code, words.size)[:] = words
        else:
            self.findings.append(dict(kind="exact", what=f"{self._what} argmax codes", bad=int((u16(code, words.size) != words).sum())))

    def _g(self, dz, code, y, coef, R, T, F, Cc, drop):
        rows = R * T * F
        _, ks, pre, v, k = self._z(y, coef, rows, Cc, drop)
        if not code:
            d = bf_get(dz, rows * Cc).reshape(rows, Cc)
        else:
            T2, F2 = T // 2, F // 2
            gp = bf_get(dz, R * T2 * F2 * Cc).reshape(R, T2, F2, Cc)
            words = u16(code, R * T2 * F2 * (Cc // 8)).astype(np.int64).reshape(R, T2, F2, Cc // 8, 1)
            cd = ((words >> (2 * np.arange(8))) & 3).reshape(R, T2, F2, Cc)
            d = np.zeros((R, T, F, Cc))
            for kk in range(4):
                df, dt = kk >> 1, kk & 1
                d[:, dt:2 * T2:2, df:2 * F2:2] = np.where(cd == kk, gp, 0.0)
            d = d.reshape(rows, Cc)
        g = d * ks * np.where(pre > 0, 1.0, self.SLOPE)
        return g, (v - k[:, 2]) * k[:, 3], k

    def sehip_unet_bn_bwd_reduce(self, dz, code, y, coef, R, T, F, Cc, seed_lo, seed_hi, ctr, layer, thresh, scale, part, st):
        g, xh, _ = self._g(dz, code, y, coef, R, T, F, Cc, (seed_lo, seed_hi, ctr, layer, thresh, scale))
        self._bwd_sums = (g.sum(0), (g * xh).sum(0), np.abs(g).sum(0), np.abs(g * xh).sum(0))

    def sehip_unet_bn_bwd_apply(self, dz, code, y, coef, bcoef, R, T, F, Cc, seed_lo, seed_hi, ctr, layer, thresh, scale, dy, st):
        g, xh, _ = self._g(dz, code, y, coef, R, T, F, Cc, (seed_lo, seed_hi, ctr, layer, thresh, scale))
        kb = f32(bcoef, 4 * Cc).astype(np.float64).reshape(Cc, 4)
        self._bf(dy, kb[:, 0] * (g - kb[:, 1] - xh * kb[:, 2]), what="dy")
