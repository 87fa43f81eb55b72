"""Host types of the implicit-GEMM engine (csrc/gemm.hip), shared by every plan; a leaf module: nothing of the package but _lib.

  CSrc / CDst / CGemmDesc   ctypes mirrors of include/sehip.h
  ParamLayout, Arena        the flat parameter buffer of a configuration; the pieces of one flat table
  enc_entry ... pad_ktab    packing-table and chunk-table helpers
  bind_chunk_table, upload_chunk_table   the chunk table of one workspace's source geometry
  fill_desc, wgrad_twin     the binder: a descriptor from plain values, and its weight-gradient twin
  UnpackTable, check_unpack_coverage     (parameter, packed-gradient entry, sign) -> the four-column un-pack table, and the proof that
                            every parameter element has an entry and the layout's padding has none
Nothing here launches anything or reads an environment variable.
"""
import ctypes as C

import numpy as np
import torch

from ._lib import SehipError

BF16 = torch.bfloat16


# --------------------------------------------------------------------------------------------------
# ctypes mirrors of include/sehip.h
# --------------------------------------------------------------------------------------------------
class CSrc(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("T", C.c_int32), ("tlo", C.c_int32), ("thi", C.c_int32), ("F", C.c_int32),
                ("C", C.c_int32), ("pad_", C.c_int32)]


class CDst(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("T", C.c_int32), ("F", C.c_int32), ("C", C.c_int32), ("toff", C.c_int32),
                ("fmul", C.c_int32), ("fadd", C.c_int32), ("is_f32", C.c_int32), ("tmul", C.c_int32)]


class CGemmDesc(C.Structure):
    _fields_ = [("src", CSrc * 4), ("dst", CDst * 2), ("ktab", C.c_void_p), ("ntab", C.c_void_p), ("W", C.c_void_p),
                ("bias", C.c_void_p), ("dW", C.c_void_p), ("dbias", C.c_void_p), ("M", C.c_int32), ("N", C.c_int32),
                ("Npad", C.c_int32), ("K", C.c_int32), ("TT", C.c_int32), ("J", C.c_int32), ("fmul", C.c_int32),
                ("tmul", C.c_int32), ("cv_nf", C.c_int32), ("cv_fadd", C.c_int32), ("cv_toff", (C.c_int32 * 2) * 2),
                ("res", C.c_void_p), ("stats", C.c_void_p), ("stats_cr", C.c_int32), ("cv2_nkt", C.c_int32), ("cv2_nf", C.c_int32),
                ("cv2_fadd", C.c_int32), ("cv2_t0", C.c_int32), ("w_tiled", C.c_int32), ("wg_hint", C.c_int32), ("dense_rows", C.c_int32),
                ("dw_split_stride", C.c_int64),
                ("bn_dz", C.c_void_p), ("bn_y", C.c_void_p), ("bn_coef", C.c_void_p), ("bn_bcoef", C.c_void_p),
                ("bn_slope", C.c_void_p),
                ("bnr_y", C.c_void_p), ("bnr_coef", C.c_void_p), ("bnr_slope", C.c_void_p), ("bnr_part", C.c_void_p),
                ("gln_stats", C.c_void_p), ("gln_slope", C.c_void_p)]


def npad_of(n):
    if n <= 16:
        return 16
    if n <= 32:
        return 32
    if n <= 64:
        return 64
    return (n + 127) // 128 * 128


def round_up(x, m):
    return (x + m - 1) // m * m


class ParamLayout:
    def __init__(self, cfg):
        self.cfg = cfg
        self.specs = cfg.param_specs()
        self.param_off, self.buffer_off, self.nbt_idx = {}, {}, {}
        po = bo = 0
        self.param_names, self.buffer_names, self.nbt_names = [], [], []
        for name, shape, kind in self.specs:
            n = int(np.prod(shape)) if len(shape) else 1
            if kind == "param":
                self.param_off[name] = (po, shape)
                self.param_names.append(name)
                po += round_up(n, 4)
            elif kind == "buffer":
                self.buffer_off[name] = (bo, shape)
                self.buffer_names.append(name)
                bo += round_up(n, 4)
            else:
                self.nbt_idx[name] = len(self.nbt_names)
                self.nbt_names.append(name)
        self.n_params = po
        self.n_buffers = bo
        # tensor boundaries for the reference's per-tensor grad_norm metric (src/solver.py:494-498)
        offs = [self.param_off[n][0] for n in self.param_names] + [po]
        self.tensor_offsets = np.asarray(offs, dtype=np.int64)

    # ComplexBatchNorm field -> (tensor, element offset inside it); None = the field does not exist (real BatchNorm2d: no cross terms)
    _REAL_BN = {"1.Wrr": ("1.weight", 0), "1.Wii": ("1.weight", 1), "1.Br": ("1.bias", 0), "1.Bi": ("1.bias", 1), "1.Wri": None,
                "1.RMr": ("1.running_mean", 0), "1.RMi": ("1.running_mean", 1), "1.RVrr": ("1.running_var", 0),
                "1.RVii": ("1.running_var", 1), "1.RVri": None}

    def bn_field(self, pre, k, cr):
        """(name, element offset) of ComplexBatchNorm field k ("1.Wrr", "1.RMr", ...) of layer `pre`, or None.  With use_cbn=False the
        layer is an nn.BatchNorm2d over 2 cr channels: its weight / bias / running statistics are the real and imaginary halves."""
        if getattr(self.cfg, "use_cbn", True) or k not in self._REAL_BN:
            return pre + k, 0
        m = self._REAL_BN[k]
        return None if m is None else (pre + m[0], m[1] * cr)

    def index_array(self, name):
        off, shape = self.param_off[name]
        n = int(np.prod(shape))
        return (off + np.arange(n, dtype=np.int64)).reshape(shape)


# --------------------------------------------------------------------------------------------------
# table helpers
# --------------------------------------------------------------------------------------------------
def enc_entry(idx, neg):
    """(index<<1)|neg, -1 where idx < 0."""
    idx = np.asarray(idx, dtype=np.int64)
    neg = np.broadcast_to(np.asarray(neg, dtype=np.int64), idx.shape)
    e = (idx << 1) | neg
    return np.where(idx < 0, -1, e).astype(np.int32)


class Arena:
    """Grows a list of numpy pieces that end up as one flat device buffer; returns element offsets."""

    def __init__(self, align):
        self.pieces, self.size, self.align = [], 0, align

    def add(self, arr):
        off = self.size
        self.pieces.append((off, arr))
        self.size += round_up(arr.shape[0], self.align)
        return off

    def reserve(self, n):
        off = self.size
        self.size += round_up(n, self.align)
        return off

    def build(self, dtype, width=None, fill=-1):
        shape = (self.size,) if width is None else (self.size, width)
        out = np.full(shape, fill, dtype=dtype)
        for off, arr in self.pieces:
            out[off:off + arr.shape[0]] = arr
        return out


def dense_ntab(n, npad, dst=0, base=0):
    t = np.zeros((npad // 4, 4), dtype=np.int32)
    for q in range(npad // 4):
        t[q] = (dst, base + 4 * q, max(0, min(4, n - 4 * q)), 0)
    return t


def wide_chunks(src, toff, fadd, c0, cn):
    """chunks covering channels [c0, c0+cn) of one source row."""
    assert cn % 8 == 0 and c0 % 8 == 0
    return [(src, toff, fadd, c0 + 8 * q) for q in range(cn // 8)]


def pad_ktab(rows):
    k = len(rows) * 8
    kp = round_up(k, 64)
    rows = rows + [(-1, 0, 0, 0)] * ((kp - k) // 8)
    return np.asarray(rows, dtype=np.int32).reshape(-1, 4), kp


def bind_chunk_table(src_tab, out_tab, kt_off, nchunks, geometry):
    """Binds the chunk rows [kt_off, kt_off + nchunks) of a (src, frame offset, row offset, channel offset) table to the
    geometry [(F, C)] of the product's sources: [src, (toff << 16) | (fadd & 0xffff), element delta, rows of a narrow chunk]
    (sehip_kchunk in include/sehip.h)."""
    rows = src_tab[kt_off:kt_off + nchunks]
    out = out_tab[kt_off:kt_off + nchunks]
    for q, (F, Cc) in enumerate(geometry):
        m = rows[:, 0] == q
        if not m.any():
            continue
        toff, fadd, coff = rows[m, 1].astype(np.int64), rows[m, 2].astype(np.int64), rows[m, 3].astype(np.int64)
        narrow = Cc == 2
        delta = (toff * F + fadd) * Cc + (0 if narrow else coff)
        assert np.abs(delta).max() < 2 ** 31 and np.abs(toff).max() < 2 ** 15 and np.abs(fadd).max() < 2 ** 15
        out[m, 1] = (((toff << 16) | (fadd & 0xffff)) & 0xffffffff).astype(np.uint32).view(np.int32)
        out[m, 2] = delta.astype(np.int32)
        out[m, 3] = coff.astype(np.int32) if narrow else 0


def upload_chunk_table(ktab, products, geometry_of, device):
    """The static chunk table bound to one workspace's source geometry, on the device.  products: the plan's product records (kt_off, K);
    geometry_of(product): [(F, C)] of its sources as the product reads them."""
    kt = ktab.copy()
    for p in products:
        bind_chunk_table(ktab, kt, p.kt_off, p.K // 8, geometry_of(p))
    return torch.from_numpy(kt).to(device)


# --------------------------------------------------------------------------------------------------
# the binder
# --------------------------------------------------------------------------------------------------
def row_ptr(t, i):
    """address of row i of a tensor (element i of a flat one); None for i = None"""
    return None if i is None else t.data_ptr() + i * t.stride(0) * t.element_size()


def fill_desc(srcs, dsts, ktab, ntab, W, bias, M, N, Npad, K, TT, J, fmul, tmul, res=None):
    """A CGemmDesc from plain values.  srcs: [(ptr, T, F, C, tlo, thi)]; dsts: [(ptr, T, F, C, toff, fmul, fadd, tmul, is_f32)]; ktab,
    ntab, W, bias, res: addresses (None = NULL).  Every other field stays zero: a plan sets what is its own."""
    d = CGemmDesc()
    for s, v in zip(d.src, srcs):
        s.ptr, s.T, s.F, s.C, s.tlo, s.thi = v
    for o, v in zip(d.dst, dsts):
        o.ptr, o.T, o.F, o.C, o.toff, o.fmul, o.fadd, o.tmul, o.is_f32 = v
    d.ktab, d.ntab, d.W, d.bias, d.res = ktab, ntab, W, bias, res
    d.M, d.N, d.Npad, d.K, d.TT, d.J, d.fmul, d.tmul = M, N, Npad, K, TT, J, fmul, tmul
    return d


def wgrad_twin(d, dW, dbias=None, dout=None):
    """The weight-gradient twin of a descriptor (sehip_wgrad reads dst[0] as the second operand): a copy with dW, dbias and -- unless dout is
    None -- dst[0] pointed at the bf16 dOut buffer.  Nothing else changes here.  In particular `res`, which several dispatch predicates of
    csrc/ test: the twins of DCCRN, DCUnet and the product graph (wav-unet, unet) keep their parent's; ConvTasNet and Demucs clear it on
    the twin themselves."""
    w = CGemmDesc.from_buffer_copy(d)
    w.dW, w.dbias = dW, dbias
    if dout is not None:
        w.dst[0].ptr, w.dst[0].is_f32 = dout, 0
    return w


# --------------------------------------------------------------------------------------------------
# the un-pack table
# --------------------------------------------------------------------------------------------------
class UnpackTable:
    """int32 [n_params][4]: the packed-gradient entries (index << 1) | sign that fold into every parameter element, -1 = none.  An entry
    goes to the next free column of its parameter, in registration order (across put() calls and within one).  count: int8 [n_params]
    entries per element.  limit: the most entries one element may have (4 columns; 1 for the plans whose un-pack reads one column)."""

    def __init__(self, n_params, limit=4):
        assert 1 <= limit <= 4
        self.limit = limit
        self.tab = np.full((n_params, 4), -1, dtype=np.int32)
        self.count = np.zeros(n_params, dtype=np.int8)
        self._mark = np.zeros(n_params, dtype=np.int32)

    def put(self, pidx, gidx, neg=0):
        p = np.asarray(pidx, dtype=np.int64).reshape(-1)
        g = np.asarray(gidx, dtype=np.int64).reshape(-1)
        if p.size == 0:
            return
        assert g.size == p.size and p.min() >= 0 and g.min() >= 0
        if g.max() >= 2 ** 30:
            raise SehipError("un-pack table: a packed-gradient index of 2^30 or more does not fit the 32-bit entry")
        e = ((g << 1) | np.broadcast_to(np.asarray(neg, dtype=np.int64).reshape(-1), p.shape)).astype(np.int32)
        seq = np.arange(p.size, dtype=np.int32)
        self._mark[p] = seq
        if (self._mark[p] != seq).any():               # a parameter several times in one call: they take consecutive columns
            order = np.argsort(p, kind="stable")
            p, e = p[order], e[order]
            first = np.flatnonzero(np.r_[True, p[1:] != p[:-1]])
            seq -= np.repeat(first, np.diff(np.r_[first, p.size])).astype(np.int32)
        else:
            seq[:] = 0
        slot = self.count[p] + seq
        if slot.max() >= self.limit:
            raise SehipError(f"un-pack table: a parameter feeds more than {self.limit} packed-gradient entries")
        self.tab[p, slot] = e
        self.count[p] = slot + 1                       # (repeated p: ascending slots, the last assignment stays)


def check_unpack_coverage(layout, count, exact=False, exempt=(), what="model"):
    """Every parameter element of the layout has at least one (exact: exactly one) entry in the un-pack table, no element of the layout's
    padding has any.  exempt: names of parameters whose gradients do not come through the table (they must then have no entry)."""
    used = np.zeros(layout.n_params, dtype=bool)
    for name in layout.param_names:
        if name not in exempt:
            off, shape = layout.param_off[name]
            used[off:off + (int(np.prod(shape)) if len(shape) else 1)] = True
    missing = int((count[used] < 1).sum())
    doubled = int((count[used] > 1).sum()) if exact else 0
    stray = int((count[~used] != 0).sum())
    if missing or doubled or stray:
        raise SehipError(f"sehip {what}: the un-pack table must give every parameter element {'exactly' if exact else 'at least'} one "
                         f"packed-gradient entry and the padding none: {missing} missing, {doubled} doubled, {stray} on padding or exempt")
