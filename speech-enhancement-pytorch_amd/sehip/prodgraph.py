"""The product graph that the plans of `wav-unet` (plan_wavunet.py) and `unet` (plan_unet.py) share: every convolution a product of the
implicit-GEMM engine's generic kernels (csrc/gemm.hip), declared once per model and independent of the input shape, and bound to the
buffers of one shape by a workspace.

  Prod               one product: chunk rows of K, the packing table of its weights, its sources and destinations
  ProdStatic         the registrars (buf / prod / norm), the arenas of the packed weights, biases, tables and gradients, and the
                     one-column un-pack table with its proof that every parameter element has exactly one packed-gradient entry
  ProdDeviceTables   the tables and the packed weights on the device
  ProdWorkspace      buffers (with canary bands for the tests), BatchNorm records and partials, the bound descriptors, and the three
                     launch groups every step has: prologue (zero, pack), start of a backward pass, join + un-pack

The 1-D Wave-U-Net is the J = 1, F = 1, stride 1 case of the 2-D form.  A plan keeps what is its own: configuration, shape refusals,
forward() / backward() and the launches around the products.  The descriptor binder, the un-pack table builder and its coverage proof
are gemmdesc.py's, shared with the other three plans of the engine.  plan_demucs.py is deliberately not built on this module: its
packed-weight segments, compact un-pack forms, framed rows and dense weight-gradient binding are their own design.
"""
import sys

import numpy as np
import torch

from . import _lib
from ._lib import ptr, SehipError
from .gemmdesc import (Arena, ParamLayout, UnpackTable, check_unpack_coverage, dense_ntab, enc_entry, fill_desc, npad_of, pad_ktab, row_ptr,
                       upload_chunk_table, wgrad_twin, BF16)
from .workspace import Buf, GemmWorkspace


class Prod:
    """One product of the engine (independent of the input shape).  rows: [(source, frame offset, row offset, channel offset)] per
    8-channel chunk of K; widx [N][8 len(rows)]: parameter index of every weight, -1 = zero; srcs: the sources as the plan's workspace
    names them (ProdWorkspace._src_view); dsts: [(buffer, columns)]; level: the row space is T_level x F_level per item; stride: (tmul,
    fmul) of the sources; scatter: (toff, fadd) with tmul = fmul = 2 in the destination (a parity class of a transposed convolution) or
    None; res: buffer added to what goes to dsts[0]; dout: the buffer a forward product's weight-gradient twin reads as dOut; bias_key:
    products that share one bias-gradient region (default: the product's own)."""

    def __init__(self, name, rows, widx, srcs, dsts, level, bias=None, kind="fwd", dout=None, stride=(1, 1), scatter=None, res=None,
                 bias_key=None):
        self.name, self.srcs, self.dsts, self.level, self.kind, self.dout = name, srcs, dsts, level, kind, dout
        self.stride, self.scatter, self.res, self.bias_key = stride, scatter, res, bias_key or name
        self.ktab, self.K = pad_ktab(list(rows))
        n, k0 = widx.shape
        assert k0 == 8 * len(rows)
        self.N, self.Npad = n, npad_of(n)
        w = np.full((self.Npad, self.K), -1, dtype=np.int32)
        w[:n, :k0] = enc_entry(widx, 0)
        self.wtab = w.reshape(-1)
        self.bias = None
        if bias is not None:
            b = np.full((self.Npad, 2), -1, dtype=np.int32)
            b[:n, 0] = enc_entry(np.asarray(bias), 0)
            self.bias = b
        assert sum(c for _, c in dsts) == n
        nt = np.concatenate([dense_ntab(c, c, q, 0) for q, (_, c) in enumerate(dsts)])
        self.ntab = np.concatenate([nt, np.zeros((self.Npad // 4 - nt.shape[0], 4), dtype=np.int32)])
        self.w_off = self.b_off = self.dw_off = self.db_off = self.kt_off = self.nt_off = None


class ProdStatic:
    """Products, packed-weight layout and gradient un-packing table of one configuration.  A subclass registers its buffers, products and
    norms (and reserves what else it keeps in the packed-gradient buffer from self.ga), then calls _assemble()."""
    plan_name = None

    def __init__(self, cfg):
        self.cfg = cfg
        self.layout = ParamLayout(cfg)
        self.prods = {}
        self.buffers = {}       # name -> (level, stored channels)
        self.norms = {}         # key -> dict(pre = prefix of weight / bias / running_*, C stored, Cr real, level, y, goff)
        self.ga = Arena(16)     # the packed-gradient buffer

    def buf(self, name, level, c):
        assert name not in self.buffers
        self.buffers[name] = (level, c)

    def prod(self, *a, **k):
        p = Prod(*a, **k)
        assert p.name not in self.prods
        self.prods[p.name] = p

    def norm(self, key, pre, c, level, y, cr=None):
        self.norms[key] = dict(pre=pre, C=c, Cr=c if cr is None else cr, level=level, y=y, goff=self.ga.reserve(2 * c))

    def _assemble(self, extra=()):
        """the arenas; extra: the un-pack entries of what the plan computes outside the products and norms"""
        wa, ba, kta, nta, ga = Arena(64), Arena(4), Arena(1), Arena(1), self.ga
        shared_db = {}
        for p in self.prods.values():
            p.kt_off = kta.add(p.ktab)
            p.nt_off = nta.add(p.ntab)
            p.w_off = wa.add(p.wtab)
            if p.bias is not None:
                p.b_off = ba.add(p.bias)
            if p.kind == "fwd":
                p.dw_off = ga.reserve(p.Npad * p.K)
                if p.bias is not None:
                    if p.bias_key not in shared_db:
                        shared_db[p.bias_key] = ga.reserve(p.Npad)
                    p.db_off = shared_db[p.bias_key]
        self.n_wpack, self.n_bpack, self.n_gpack = wa.size, max(ba.size, 4), ga.size
        if max(self.n_wpack, self.n_gpack, self.layout.n_params) >= 2 ** 30:
            raise SehipError(f"sehip {self.plan_name}: the 32-bit packing tables hold fewer than 2^30 entries")
        self.wtab = wa.build(np.int32)
        self.btab = ba.build(np.int32, 2) if ba.size else np.full((4, 2), -1, dtype=np.int32)
        self.ktab = kta.build(np.int32, 4)
        self.ntab = nta.build(np.int32, 4, fill=0)
        for p in self.prods.values():
            p.wtab = None            # the arena's table holds the only copy from here on
        wa.pieces = []
        self.utab1 = self._build_unpack_table(extra)

    def _build_unpack_table(self, extra=()):
        """int32 [n_params]: (index in the packed-gradient buffer) << 1 of every parameter element, -1 for the layout's padding.
        extra: [(parameter indices, packed indices)]."""
        Lay = self.layout
        ia = Lay.index_array
        ut = UnpackTable(Lay.n_params, limit=1)
        put = ut.put
        done_bias = set()
        for p in self.prods.values():
            if p.dw_off is None:
                continue
            w = self.wtab[p.w_off:p.w_off + p.Npad * p.K]
            m = np.flatnonzero(w >= 0)
            put(w[m] >> 1, p.dw_off + m)
            if p.db_off is not None and p.db_off not in done_bias:      # the four parity classes of one transposed convolution share it
                done_bias.add(p.db_off)
                b = p.bias[:, 0]
                m = np.flatnonzero(b >= 0)
                put(b[m] >> 1, p.db_off + m)
        for nm in self.norms.values():
            put(ia(nm["pre"] + "weight"), nm["goff"] + np.arange(nm["Cr"]))
            put(ia(nm["pre"] + "bias"), nm["goff"] + nm["C"] + np.arange(nm["Cr"]))
        for pidx, gidx in extra:
            put(pidx, gidx)
        check_unpack_coverage(Lay, ut.count, exact=True, what=self.plan_name)
        return np.ascontiguousarray(ut.tab[:, 0])


class ProdDeviceTables:
    def __init__(self, st: ProdStatic, device):
        f = lambda a: torch.from_numpy(a).to(device)
        self.wtab, self.btab, self.ntab, self.utab1 = f(st.wtab), f(st.btab), f(st.ntab), f(st.utab1)
        self.tensor_offsets = f(st.layout.tensor_offsets)
        self.wpack = torch.zeros(st.n_wpack, dtype=BF16, device=device)
        self.bpack = torch.zeros(st.n_bpack, dtype=torch.float32, device=device)


class ProdWorkspace(GemmWorkspace):
    """Buffers and bound descriptors for `items` tensors of Tl[level] frames x Fl[level] rows.  `guard` > 0 (tests): every activation
    buffer sits between two bands of that many canary elements inside its allocation."""
    GUARD_BF16 = -1234.0

    def __init__(self, st: ProdStatic, tables: ProdDeviceTables, items, Tl, Fl, device, guard=0):
        super().__init__()
        self.st, self.tb, self.items, self.Tl, self.Fl, self.device = st, tables, items, Tl, Fl, device
        self.guard, self._alloc = int(guard), {}
        self.bufs = {}
        for name, (level, c) in st.buffers.items():
            self.bufs[name] = Buf(self._make(name, (items, Tl[level], Fl[level], c), BF16), Tl[level], Fl[level], c)
        lib = _lib.lib()
        self.coef, self.bcoef, self.part, self.bpart = {}, {}, {}, {}
        for k, nm in st.norms.items():
            self.coef[k] = torch.zeros(nm["C"], 4, dtype=torch.float32, device=device)
            self.bcoef[k] = torch.zeros(nm["C"], 4, dtype=torch.float32, device=device)
            # one row of partial sums per workgroup; every layer its own (the op-local tests read them back)
            self.part[k] = torch.zeros(max(int(lib.sehip_wun_bn_scratch_floats(self._norm_rows(k), nm["C"])), 1), dtype=torch.float32,
                                       device=device)
            self.bpart[k] = torch.zeros_like(self.part[k])
        self.gpack = torch.zeros(st.n_gpack, dtype=torch.float32, device=device)
        self._bwd_clean = False
        self.side = self._new_side_stream(device) if device.type == "cuda" else None
        self._bind()

    def _make(self, name, shape, dtype):
        n = int(np.prod(shape))
        g = self.guard
        if not g:
            t = torch.zeros(shape, dtype=dtype, device=self.device)
        else:
            whole = torch.full((n + 2 * g,), self.GUARD_BF16 if dtype == BF16 else -21846, dtype=dtype, device=self.device)
            self._alloc[name] = whole
            t = whole[g:g + n].view(shape)
            t.zero_()
        return t

    def guards_intact(self):
        """names of the buffers whose canary bands were written (tests)"""
        g, bad = self.guard, []
        for name, whole in self._alloc.items():
            want = self.GUARD_BF16 if whole.dtype == BF16 else -21846
            if not (bool((whole[:g] == want).all()) and bool((whole[-g:] == want).all())):
                bad.append(name)
        return bad

    def _norm_rows(self, key):
        lv = self.st.norms[key]["level"]
        return self.items * self.Tl[lv] * self.Fl[lv]

    def _src_view(self, s):
        """(pointer, T, F, C) of an entry of Prod.srcs as the products read it"""
        b = self.bufs[s]
        return b.ptr, b.Tst, b.F, b.C

    def _bind(self):
        st, tb = self.st, self.tb
        self.desc = {}
        self.ktab_dev = upload_chunk_table(st.ktab, st.prods.values(), lambda p: [self._src_view(s)[2:] for s in p.srcs], self.device)
        for name, p in st.prods.items():
            tt, jj = self.Tl[p.level], self.Fl[p.level]
            srcs, dsts = [], []
            for s in p.srcs:
                sp, sT, sF, sC = self._src_view(s)
                if p.stride == (1, 1):
                    assert (sT, sF) == (tt, jj), (name, s)
                else:
                    assert sT >= 2 * tt and sF >= 2 * jj, (name, s)
                srcs.append((sp, sT, sF, sC, 0, sT))
            for bname, cols in p.dsts:
                ob = self.bufs[bname]
                assert ob.C == cols, (name, bname)
                if p.scatter is None:
                    assert (ob.Tst, ob.F) == (tt, jj), (name, bname)
                    dsts.append((ob.ptr, ob.Tst, ob.F, ob.C, 0, 1, 0, 1, 0))
                else:
                    assert ob.Tst >= 2 * tt and ob.F >= 2 * jj, (name, bname)
                    dsts.append((ob.ptr, ob.Tst, ob.F, ob.C, p.scatter[0], 2, p.scatter[1], 2, 0))
            ob = self.bufs[p.dsts[0][0]]
            res = None
            if p.res is not None:
                rb = self.bufs[p.res]
                assert (rb.Tst, rb.F, rb.C) == (ob.Tst, ob.F, ob.C), (name, p.res)
                res = rb.ptr
            d = self.desc[name] = fill_desc(srcs, dsts, row_ptr(self.ktab_dev, p.kt_off), row_ptr(tb.ntab, p.nt_off),
                                            row_ptr(tb.wpack, p.w_off), row_ptr(tb.bpack, p.b_off), self.items * tt * jj, p.N, p.Npad,
                                            p.K, tt, jj, p.stride[1], p.stride[0], res)
            if p.dw_off is not None:
                gb = self.bufs[p.dout]
                assert (gb.Tst, gb.F, gb.C) == (ob.Tst, ob.F, ob.C), (name, p.dout)
                self.desc[name + ".wg"] = wgrad_twin(d, row_ptr(self.gpack, p.dw_off), row_ptr(self.gpack, p.db_off), gb.ptr)

    # ---- launches (gemm, wgrad: GemmWorkspace) ------------------------------------------------------------------------
    def _launch(self, name, *a):
        """On the current stream, through the `call` and `stream` of the module that defines the plan's workspace, as the plan's own
        launches go: whoever intercepts a plan's launches there (the tests' emulator and their "refused before any launch" recorders)
        sees the prologue and the un-pack too.  This module has no `call` of its own to forget."""
        m = sys.modules[type(self).__module__]
        m.call(name, *a, m.stream())

    def _prologue(self, params):
        """what every forward pass starts with: the packed gradients cleared, weights and biases packed"""
        st, tb = self.st, self.tb
        self._launch("sehip_zero_regions", ptr(self.gpack), self.gpack.numel() * 4, None, 0, None, 0, None, 0)
        self._bwd_clean = True
        self._launch("sehip_pack_bf16", ptr(params), ptr(tb.wtab), st.n_wpack, ptr(tb.wpack))
        self._launch("sehip_pack_f32", ptr(params), ptr(tb.btab), st.n_bpack, ptr(tb.bpack))

    def _begin_backward(self):
        if not self._bwd_clean:            # a second backward pass over the same forward
            self.gpack.zero_()
        self._bwd_clean = False
        self._chain_dirty = True

    def _unpack(self, grads, tail):
        """the two streams joined, then the packed gradients through the one-column table into the flat gradients (overwritten)"""
        self.join_side()
        np_ = self.st.layout.n_params
        if tail is not None:      # FlatOptimizer's accumulators: the un-pack also takes the clipping norm / metric sums
            self._launch("sehip_unpack_grad1_sums", ptr(self.gpack), ptr(self.tb.utab1), np_, ptr(grads), tail[2], tail[3], tail[0], tail[1],
                         tail[4], None)
        else:
            self._launch("sehip_unpack_grad1", ptr(self.gpack), ptr(self.tb.utab1), np_, ptr(grads))
        return grads
