"""Host logic of the workspace base (sehip/workspace.py), without a GPU: every library call goes to a recorder, the side stream is a
stand-in with a `cuda_stream` handle.  Asserted: one stream dependency per run of weight gradients, the event pool's size and order,
close() destroying every event once, and the un-pack entry point chosen by `tail` / `uperm` with the tail's fields in the C ABI's
argument order."""
import types

import pytest
import torch

MAIN, SIDE = 1001, 2002


class Recorder:
    def __init__(self):
        self.calls, self.created, self.destroyed = [], [], []

    def __call__(self, name, *args):
        self.calls.append((name,) + args)

    def names(self):
        return [c[0] for c in self.calls]

    # the part of the library the base reaches through _lib.lib()
    def lib(self):
        return self

    def sehip_event_create(self):
        self.created.append(5000 + len(self.created))
        return self.created[-1]

    def sehip_event_destroy(self, e):
        self.destroyed.append(e)


@pytest.fixture
def rec(monkeypatch):
    from sehip import workspace as W
    r = Recorder()
    monkeypatch.setattr(W, "call", r)
    monkeypatch.setattr(W, "stream", lambda: MAIN)
    monkeypatch.setattr(W, "ptr", lambda t: t)              # "pointers" are the objects themselves
    monkeypatch.setattr(W, "_lib", r)
    monkeypatch.setattr(W.C, "byref", lambda d: d)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    return r


def make(side=True, pool=None, uperm=None, extra_events=False):
    from sehip.workspace import GemmWorkspace

    class Ws(GemmWorkspace):
        event_attrs = ("_events", "_mine") if extra_events else ("_events",)
        if pool is not None:
            event_pool = pool

        def __init__(self):
            super().__init__()
            self.desc = {"a": "desc a", "a.wg": "wg a", "b.wg": "wg b", "c.wg": "wg c"}
            self.side = types.SimpleNamespace(cuda_stream=SIDE) if side else None
            self.st = types.SimpleNamespace(layout=types.SimpleNamespace(n_params=77))
            self.tb = types.SimpleNamespace(utab="utab", utab_g="utab_g", uperm=uperm)
            self.gpack = "gpack"

    return Ws()


def test_one_dependency_per_run_of_weight_gradients(rec):
    ws = make()
    ws.wgrad("a"); ws.wgrad("b")
    assert rec.names() == ["sehip_stream_depend", "sehip_wgrad", "sehip_wgrad"]
    dep = rec.calls[0]
    assert dep[1:3] == (SIDE, MAIN) and dep[3] in rec.created                  # the side stream waits for the chain
    assert rec.calls[1] == ("sehip_wgrad", "wg a", SIDE) and rec.calls[2] == ("sehip_wgrad", "wg b", SIDE)
    ws.gemm("a")                                                                 # the chain moved on: the next run waits again
    assert rec.calls[3] == ("sehip_gemm", "desc a", MAIN)
    ws.wgrad("c"); ws.wgrad("a")
    assert rec.names()[4:] == ["sehip_stream_depend", "sehip_wgrad", "sehip_wgrad"]
    assert rec.calls[4][1:3] == (SIDE, MAIN) and rec.calls[4][3] != dep[3]       # (the pool's next event)
    ws.join_side()
    assert rec.calls[-1][:3] == ("sehip_stream_depend", MAIN, SIDE) and rec.names().count("sehip_stream_depend") == 3


def test_without_a_side_stream_everything_stays_on_the_chain(rec):
    ws = make(side=False)
    ws.wgrad("a"); ws.gemm("a"); ws.wgrad("b"); ws.join_side()
    assert rec.calls == [("sehip_wgrad", "wg a", MAIN), ("sehip_gemm", "desc a", MAIN), ("sehip_wgrad", "wg b", MAIN)]
    assert rec.created == []


def test_a_capturing_stream_keeps_the_weight_gradients_on_the_chain(rec, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    ws = make()
    ws.wgrad("a"); ws.join_side()
    assert rec.calls == [("sehip_wgrad", "wg a", MAIN)]


@pytest.mark.parametrize("pool", [16, 32])
def test_event_pool_round_robin(rec, pool):
    from sehip.workspace import GemmWorkspace
    from sehip.plan import DCCRNWorkspace
    assert GemmWorkspace.event_pool == 16 and DCCRNWorkspace.event_pool == 32
    ws = make(pool=None if pool == 16 else pool)
    got = [ws._event() for _ in range(2 * pool + 3)]
    assert len(rec.created) == pool and len(set(rec.created)) == pool            # created once, on first use
    assert sorted(got[:pool]) == sorted(rec.created)                             # every event once per round ...
    assert got[pool:2 * pool] == got[:pool] and got[2 * pool:] == got[:3]        # ... in the same order every round
    assert all(got[i + 1] == rec.created[(rec.created.index(got[i]) + 1) % pool] for i in range(len(got) - 1))


def test_close_destroys_every_event_exactly_once(rec):
    ws = make(extra_events=True)
    assert ws._mine == [] and not ws.closed and ws.generation == 0 and not ws.pinned
    ws._event()
    ws._mine = [ws._new_event(), ws._new_event()]                                # a subclass's own list (Demucs, DCCRN)
    assert len(rec.created) == 18
    ws.close()
    assert ws.closed and sorted(rec.destroyed) == sorted(rec.created) and ws._events == [] and ws._mine == []
    ws.close()
    ws.__del__()
    assert len(rec.destroyed) == 18


def test_event_creation_failure_is_an_error(rec, monkeypatch):
    from sehip import SehipError
    monkeypatch.setattr(rec, "sehip_event_create", lambda: None)
    monkeypatch.setattr(rec, "sehip_last_error", lambda: b"out of events", raising=False)
    with pytest.raises(SehipError, match="sehip_event_create: out of events"):
        make()._event()


TAIL = ("sumsq", "tensor_sums", "offsets", "ntensors", "step")                  # FlatOptimizer's order


def test_unpack_picks_the_entry_point_and_orders_the_tail(rec):
    # C ABI: (gpack, table[, perm], n, grads, offsets, ntensors, sumsq, tensor_sums, step counter, guard, stream)
    make(uperm="uperm").unpack("grads", TAIL, guard="guard")
    make(uperm=None).unpack("grads", TAIL)
    make(uperm="uperm").unpack("grads", None)
    make(uperm=None).unpack("grads", None, guard="guard")
    assert rec.calls == [
        ("sehip_unpack_grad_sums_perm", "gpack", "utab_g", "uperm", 77, "grads", "offsets", "ntensors", "sumsq", "tensor_sums", "step", "guard", MAIN),
        ("sehip_unpack_grad_sums", "gpack", "utab", 77, "grads", "offsets", "ntensors", "sumsq", "tensor_sums", "step", None, MAIN),
        ("sehip_unpack_grad", "gpack", "utab", 77, "grads", MAIN),
        ("sehip_unpack_grad", "gpack", "utab", 77, "grads", MAIN)]


def test_unpack_argument_counts_match_the_prototypes():
    from sehip import _lib
    assert len(_lib._PROTOS["sehip_unpack_grad_sums_perm"]) == 12 and len(_lib._PROTOS["sehip_unpack_grad_sums"]) == 11
    assert len(_lib._PROTOS["sehip_unpack_grad"]) == 5


def test_the_plans_share_the_base_and_bench_sees_what_it_saw():
    """bench.py branches on hasattr(ws, "launch_units") / hasattr(ws, "_launch_wgrad"): neither may appear on the base."""
    from sehip import plan, plan_dcunet, plan_demucs, plan_rnnmask, plan_tasnet, plan_wavunet, workspace as W
    gemm = [plan.DCCRNWorkspace, plan_dcunet.DCUNetWorkspace, plan_demucs.DemucsWorkspace, plan_tasnet.TasNetWorkspace,
            plan_wavunet.WavUnetWorkspace]
    assert all(issubclass(c, W.GemmWorkspace) for c in gemm)
    assert issubclass(plan_rnnmask.RnnMaskWorkspace, W.Workspace) and not issubclass(plan_rnnmask.RnnMaskWorkspace, W.GemmWorkspace)
    assert plan.Buf is W.Buf and plan_dcunet.Buf is W.Buf
    for base in (W.Workspace, W.GemmWorkspace):
        assert not hasattr(base, "_launch_wgrad") and not hasattr(base, "launch_units") and not hasattr(base, "pl") and not hasattr(base, "st")
    assert [c for c in gemm if hasattr(c, "_launch_wgrad")] == [plan_demucs.DemucsWorkspace]
    assert [c for c in gemm if hasattr(c, "launch_units")] == [plan.DCCRNWorkspace]
    assert plan_demucs.DemucsWorkspace.event_attrs == ("_events", "_held_events")
    assert plan.DCCRNWorkspace.event_attrs == ("_events", "_fs_events")
    b = W.Buf("t", 3, 4, 5)
    assert (b.Tst, b.F, b.C, b.t0) == (3, 4, 5, 0) and W.Buf("t", 3, 4, 5, 2).t0 == 2
