"""What every plan's workspace shares: the life cycle the models' workspace cache relies on (generation / pinned / closed), and for the
plans built on the implicit-GEMM engine the event pool, the product launches, the weight gradients on the side stream and the un-pack of
the packed gradients.  What a plan allocates, binds and launches in forward() / backward() stays in its own module; the descriptor type, its binder and the
un-pack table builder are gemmdesc.py's.  GemmDeviceTables: the device copies of the tables of the plans with a four-column un-pack.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib
from ._lib import call, ptr, stream, SehipError
from .gemmdesc import BF16


class Buf:
    """One activation tensor [items][Tst][F][C] of a workspace (t0: first frame held, plan.DCCRNWorkspace only)."""

    def __init__(self, t, tst, f, c, t0=0):
        self.t, self.Tst, self.F, self.C, self.t0 = t, tst, f, c, t0

    @property
    def ptr(self):
        return self.t.data_ptr()


def gather_ordered_unpack_table(tab, tensor_offsets):
    """The un-pack table [n_params][4] with the rows of every tensor sorted by the address of their first packed entry, and the
    parameter each row un-packs (int32 [n_params]): the form sehip_unpack_grad_sums_perm takes.  A convolution weight
    [co][ci][kf][kt] reads dW[n][(kt, kf, ci)]: in parameter order neighbouring lanes gather floats 5 C apart (one 64-byte sector per
    4-byte read), in gather order they read a run of `ci`.  Rows never leave their tensor: the per-tensor sums are taken by position."""
    tab = np.asarray(tab)
    n = tab.shape[0]
    first = tab[:, 0].astype(np.int64) >> 1
    first[tab[:, 0] < 0] = np.iinfo(np.int64).max >> 2          # parameters without a packed entry stay where they are, at the end
    offs = np.asarray(tensor_offsets, dtype=np.int64)
    tensor_of = np.searchsorted(offs, np.arange(n, dtype=np.int64), side="right") - 1
    perm = np.lexsort((np.arange(n), first, tensor_of)).astype(np.int32)     # by tensor, then by gather address, stable
    assert np.array_equal(tensor_of[perm], tensor_of)
    return np.ascontiguousarray(tab[perm]), perm


def gather_ordered_device_tables(utab, tensor_offsets, to_device):
    """(utab_g, uperm) of a *DeviceTables: the fused tail's un-pack in gather order; (None, None) under SEHIP_NO_UNPACK_PERM
    (parameter order)."""
    if os.environ.get("SEHIP_NO_UNPACK_PERM"):
        return None, None
    tg, pm = gather_ordered_unpack_table(utab, tensor_offsets)
    return to_device(tg), to_device(pm)


class GemmDeviceTables:
    """Device copies of the static tables of a plan with the four-column un-pack table (shared by every workspace of a model on one
    device) and its packed weights; bias=True: the bias table and the packed biases too.  A subclass adds what else its plan reads."""

    def __init__(self, st, layout, device, bias=True):
        f = self.to_device = lambda a: torch.from_numpy(a).to(device)
        self.wtab, self.utab, self.ntab = f(st.wtab), f(st.utab), f(st.ntab)
        self.tensor_offsets = f(layout.tensor_offsets)
        self.utab_g, self.uperm = gather_ordered_device_tables(st.utab, layout.tensor_offsets, f)
        self.wpack = torch.zeros(st.n_wpack, dtype=BF16, device=device)
        if bias:
            self.btab = f(st.btab)
            self.bpack = torch.zeros(max(st.n_bpack, 4), dtype=torch.float32, device=device)


class Workspace:
    """Life cycle of the buffers of one input shape.  generation: bumped by every forward (a backward checks that its activations are
    still the live ones); pinned: a captured hipGraph holds raw pointers into this workspace, never evict; closed: evicted, or the model
    moved."""
    event_attrs = ()        # names of the lists of HIP events close() destroys

    def __init__(self):
        self.generation, self.pinned, self.closed = 0, False, False
        for a in self.event_attrs:
            setattr(self, a, [])

    def close(self):
        """Destroys the HIP events of this workspace (the tensors go with the Python object)."""
        if self.closed:
            return
        self.closed = True
        for a in self.event_attrs:
            for e in getattr(self, a):
                _lib.lib().sehip_event_destroy(e)
            setattr(self, a, [])

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def _layout(self):
        return self.st.layout

    def _pp(self, params, name):
        return params.data_ptr() + 4 * self._layout.param_off[name][0]


class GemmWorkspace(Workspace):
    """Workspace of a plan on the implicit-GEMM engine.  A subclass provides desc (name -> CGemmDesc, the weight-gradient twin under
    name + ".wg"), gpack, tb (its *DeviceTables) and side (the weight-gradient stream, or None)."""
    event_attrs = ("_events",)
    event_pool = 16

    def __init__(self):
        super().__init__()
        self._event_i, self._chain_dirty = 0, True

    @staticmethod
    def _new_side_stream(device):
        return None if os.environ.get("SEHIP_NO_SIDE_STREAM") else torch.cuda.Stream(device=device)

    @staticmethod
    def _new_event():
        e = _lib.lib().sehip_event_create()
        if not e:
            raise SehipError("sehip_event_create: " + _lib.lib().sehip_last_error().decode())
        return e

    def _event(self):
        """Round-robin pool of fence-free events (sehip_stream_depend)."""
        if not self._events:
            self._events = [self._new_event() for _ in range(self.event_pool)]
        self._event_i = (self._event_i + 1) % len(self._events)
        return self._events[self._event_i]

    def gemm(self, name):
        self._chain_dirty = True
        call("sehip_gemm", C.byref(self.desc[name]), stream())

    def _side_in_use(self):
        """a graph capture keeps everything on the chain's own stream"""
        return self.side is not None and not torch.cuda.is_current_stream_capturing()

    def _issue_wgrad(self, name, handle):
        call("sehip_wgrad", C.byref(self.desc[name + ".wg"]), handle)

    def wgrad(self, name):
        """Weight gradients are side work (nothing in the backward chain consumes them): they go to the second stream, which waits for
        everything enqueued so far on the main one (the producer of dOut included) -- once per run of weight gradients: every event
        record costs the chain a bubble, and nothing new is on the chain until the next gemm() / _chain_dirty = True.  join_side() brings
        the two streams together before the gradients are un-packed."""
        if not self._side_in_use():
            self._issue_wgrad(name, stream())
            return
        if self._chain_dirty:
            call("sehip_stream_depend", self.side.cuda_stream, stream(), self._event())
            self._chain_dirty = False
        self._issue_wgrad(name, self.side.cuda_stream)

    def join_side(self):
        if self._side_in_use():
            call("sehip_stream_depend", stream(), self.side.cuda_stream, self._event())

    def unpack(self, grads, tail, guard=None):
        """The packed gradients through the four-column table into the flat parameter gradients (overwritten).  tail = (sumsq,
        tensor_sums, offsets, ntensors, step counter) of the fused optimizer: the un-pack also takes its clipping norm / metric sums and
        advances its device step counter, unless the word at `guard` is set (FlatOptimizer._arm_fused_tail)."""
        tb, n = self.tb, self._layout.n_params
        if tail is None:
            call("sehip_unpack_grad", ptr(self.gpack), ptr(tb.utab), n, ptr(grads), stream())
        elif tb.uperm is not None:
            call("sehip_unpack_grad_sums_perm", ptr(self.gpack), ptr(tb.utab_g), ptr(tb.uperm), n, ptr(grads), tail[2], tail[3], tail[0],
                 tail[1], tail[4], guard, stream())
        else:
            call("sehip_unpack_grad_sums", ptr(self.gpack), ptr(tb.utab), n, ptr(grads), tail[2], tail[3], tail[0], tail[1], tail[4],
                 guard, stream())
