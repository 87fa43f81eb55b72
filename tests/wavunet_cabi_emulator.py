"""A host emulation of the C-ABI calls that sehip/plan_wavunet.py issues -- TEST INFRASTRUCTURE ONLY.

tests/cabi_emulator.py (the tables, the products, the BatchNorm statistics and records) in its write mode, plus the csrc/wavunet.hip
entry points written from their math in float64: the first layer from the fp32 waveform, LeakyReLU(0.1), the `[::2]` adjoint in the
BatchNorm backward, the x2 upsampling and the head.  With it the plan's own forward() / backward() run on the CPU, so its wiring -- buffer
names and levels, pointer offsets, bound tables, launch order -- is tested against the reference's vectors without a GPU
(tests/test_wavunet_host.py).  bf16 stores round to nearest even as the kernels do.
"""
import numpy as np

import cabi_emulator
from cabi_emulator import bf_get, f32


class Emulator(cabi_emulator.Emulator):
    SLOPE = 0.1

    def __init__(self):
        super().__init__()          # write mode only: the fp32 results of this file's entry points are stored, never compared

    # ---- csrc/wavunet.hip, from the math ---------------------------------------------------------------------------
    def sehip_wun_enc0_fwd(self, x, W, bias, B, T, C0, y0, st):
        xp = np.pad(f32(x, B * T).astype(np.float64).reshape(B, T), ((0, 0), (7, 7)))
        w = f32(W, C0 * 15).astype(np.float64).reshape(C0, 15)
        win = np.stack([xp[:, k:k + T] for k in range(15)], -1)                # [B][T][15]
        self._bf(y0, win @ w.T + f32(bias, C0))

    def sehip_wun_enc0_wgrad(self, dy0, x, B, T, C0, dW, db, scratch, st):
        xp = np.pad(f32(x, B * T).astype(np.float64).reshape(B, T), ((0, 0), (7, 7)))
        win = np.stack([xp[:, k:k + T] for k in range(15)], -1).reshape(B * T, 15)
        g = bf_get(dy0, B * T * C0).reshape(B * T, C0)
        f32(dW, C0 * 15)[:] = (g.T @ win).reshape(-1)
        f32(db, C0)[:] = g.sum(0)

    def sehip_wun_bn_finalize(self, part, y, gamma, beta, rm, rv, nbt, rows, Cc, eps, momentum, training, coef, st):
        self._bn_finalize(part, y, gamma, beta, rm, rv, nbt, rows, Cc, Cc, eps, momentum, training, coef)

    def _z(self, y, coef, rows, Cc):
        k = f32(coef, 4 * Cc).astype(np.float64).reshape(Cc, 4)
        v = bf_get(y, rows * Cc).reshape(rows, Cc)
        return self.lrelu(k[:, 0] * v + k[:, 1]), v, k

    def sehip_wun_bn_apply(self, y, coef, rows, Cc, z, st):
        self._bf(z, self._z(y, coef, rows, Cc)[0])

    def sehip_wun_bn_apply_up2(self, y, coef, B, Tin, Cc, up, st):
        from sehip.plan_wavunet import up2_table
        z = self._z(y, coef, B * Tin, Cc)[0].reshape(B, Tin, Cc)
        i0, i1, w = up2_table(Tin)
        self._bf(up, z[:, i0] * (1 - w)[None, :, None] + z[:, i1] * w[None, :, None])

    def sehip_wun_up2_bwd(self, dup, B, Tin, Cc, dz, st):
        from sehip.plan_wavunet import up2_table
        g = bf_get(dup, B * 2 * Tin * Cc).reshape(B, 2 * Tin, Cc)
        i0, i1, w = up2_table(Tin)
        out = np.zeros((B, Tin, Cc))
        np.add.at(out, (slice(None), i0), g * (1 - w)[None, :, None])
        np.add.at(out, (slice(None), i1), g * w[None, :, None])
        self._bf(dz, out)

    def _g(self, dzf, dze, y, coef, rows, Cc):
        z, v, k = self._z(y, coef, rows, Cc)
        d = bf_get(dzf, rows * Cc).reshape(rows, Cc).copy()
        if dze:
            d[::2] += bf_get(dze, rows // 2 * Cc).reshape(rows // 2, Cc)
        return np.where(k[:, 0] * v + k[:, 1] > 0, d, self.SLOPE * d), (v - k[:, 2]) * k[:, 3], k

    def sehip_wun_bn_bwd_reduce(self, dzf, dze, y, coef, rows, Cc, part, st):
        g, xh, _ = self._g(dzf, dze, y, coef, rows, Cc)
        self._bwd_sums = (g.sum(0), (g * xh).sum(0), np.abs(g).sum(0), np.abs(g * xh).sum(0))

    def sehip_wun_bn_bwd_apply(self, dzf, dze, y, coef, bcoef, rows, Cc, dy, st):
        g, xh, _ = self._g(dzf, dze, y, coef, rows, Cc)
        kb = f32(bcoef, 4 * Cc).astype(np.float64).reshape(Cc, 4)
        self._bf(dy, kb[:, 0] * (g - kb[:, 1] - xh * kb[:, 2]))

    def sehip_wun_out_fwd(self, z, x, W, bias, rows, C0, out, st):
        w = f32(W, C0 + 1).astype(np.float64)
        f32(out, rows)[:] = np.tanh(bf_get(z, rows * C0).reshape(rows, C0) @ w[:C0] + w[C0] * f32(x, rows) + f32(bias, 1)[0])

    def sehip_wun_out_bwd(self, dout, out, z, x, W, rows, C0, dz, dW, db, scratch, st):
        o = f32(out, rows).astype(np.float64)
        dp = f32(dout, rows) * (1 - o * o)
        w = f32(W, C0 + 1).astype(np.float64)
        self._bf(dz, dp[:, None] * w[None, :C0])
        f32(dW, C0 + 1)[:] = np.concatenate([dp @ bf_get(z, rows * C0).reshape(rows, C0), [dp @ f32(x, rows)]])
        f32(db, 1)[0] = dp.sum()
