"""Host bookkeeping every plan of the implicit-GEMM engine shares (sehip/gemmdesc.py), without a GPU: the un-pack table builder and its
coverage proof on a toy layout with padding, the descriptor binder on CPU tensors and what a weight-gradient twin changes."""
import ctypes as C

import numpy as np
import pytest
import torch


class ToyConfig:
    """three tensors of 3, 5 and 1 elements: the layout pads them to 4, 8 and 4 (elements 3, 9-11, 13-15 are padding)"""

    def param_specs(self):
        return [("a", (3,), "param"), ("b", (5,), "param"), ("c", (), "param")]


@pytest.fixture(scope="module")
def G():
    from sehip import gemmdesc
    return gemmdesc


@pytest.fixture(scope="module")
def layout(G):
    L = G.ParamLayout(ToyConfig())
    assert L.n_params == 16 and [L.param_off[n][0] for n in "abc"] == [0, 4, 12]
    return L


REAL = [0, 1, 2, 4, 5, 6, 7, 8, 12]


def test_the_leaf_module_is_what_the_plans_use(G):
    from sehip import plan, plan_demucs, plan_dcunet, plan_tasnet, prodgraph
    for name in ("CSrc", "CDst", "CGemmDesc", "ParamLayout", "Arena", "enc_entry", "npad_of", "round_up", "dense_ntab", "wide_chunks",
                 "pad_ktab", "bind_chunk_table", "BF16"):
        assert getattr(plan, name) is getattr(G, name), name
    assert not hasattr(plan, "Gemm")
    for m in (plan_demucs, plan_dcunet, plan_tasnet, prodgraph):
        assert m.ParamLayout is G.ParamLayout and m.UnpackTable is G.UnpackTable and m.fill_desc is G.fill_desc


def test_unpack_slots_follow_registration_order_and_carry_the_sign(G):
    ut = G.UnpackTable(16)
    ut.put([0, 1, 2], [100, 101, 102])
    ut.put([2, 4, 2, 5, 2], [200, 201, 202, 203, 204], [1, 0, 0, 1, 1])      # parameter 2 three times in one call: the next three columns
    ut.put([4], 300, 1)                                                      # ... and across calls
    e = lambda g, neg=0: (g << 1) | neg
    assert ut.tab.dtype == np.int32 and ut.tab.shape == (16, 4)
    assert ut.tab[0].tolist() == [e(100), -1, -1, -1] and ut.tab[1].tolist() == [e(101), -1, -1, -1]
    assert ut.tab[2].tolist() == [e(102), e(200, 1), e(202), e(204, 1)]
    assert ut.tab[4].tolist() == [e(201), e(300, 1), -1, -1] and ut.tab[5].tolist() == [e(203, 1), -1, -1, -1]
    assert ut.count.tolist() == [1, 1, 4, 0, 2, 1] + [0] * 10
    assert (ut.tab[[3, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15]] == -1).all()
    ut.put(np.zeros(0, np.int64), np.zeros(0, np.int64))                     # nothing to register
    assert ut.count.sum() == 9


def test_unpack_refuses_a_fifth_entry_a_second_under_limit_one_and_wide_indices(G):
    from sehip import SehipError
    ut = G.UnpackTable(16)
    ut.put([7, 7, 7], [1, 2, 3])
    ut.put([7], [4])
    with pytest.raises(SehipError, match="more than 4"):
        ut.put([7], [5])
    with pytest.raises(SehipError, match="more than 4"):
        G.UnpackTable(16).put([1] * 5, np.arange(5))
    one = G.UnpackTable(16, limit=1)
    one.put([0, 1], [10, 11])
    with pytest.raises(SehipError, match="more than 1"):
        one.put([5, 1], [12, 13])
    with pytest.raises(SehipError, match="more than 1"):
        G.UnpackTable(16, limit=1).put([3, 3], [1, 2])
    with pytest.raises(SehipError, match="2\\^30"):
        G.UnpackTable(16).put([0], [2 ** 30])
    ok = G.UnpackTable(16)
    ok.put([0], [2 ** 30 - 1])
    assert ok.tab[0, 0] == 2 ** 31 - 2


def test_coverage_check(G, layout):
    from sehip import SehipError

    def counts(idx):
        ut = G.UnpackTable(16)
        ut.put(idx, np.arange(len(idx)))
        return ut.count

    G.check_unpack_coverage(layout, counts(REAL))
    G.check_unpack_coverage(layout, counts(REAL), exact=True)
    G.check_unpack_coverage(layout, counts(REAL + [5]))                      # at-least-one mode: a doubled element is fine
    with pytest.raises(SehipError, match="1 missing, 0 doubled, 0 on padding"):
        G.check_unpack_coverage(layout, counts([i for i in REAL if i != 8]))
    with pytest.raises(SehipError, match="0 missing, 0 doubled, 1 on padding"):
        G.check_unpack_coverage(layout, counts(REAL + [9]))
    with pytest.raises(SehipError, match="0 missing, 1 doubled, 0 on padding"):
        G.check_unpack_coverage(layout, counts(REAL + [5]), exact=True)
    # an exempt parameter has no entry, and may have none
    G.check_unpack_coverage(layout, counts(REAL[:-1]), exact=True, exempt=("c",))
    with pytest.raises(SehipError, match="0 missing, 0 doubled, 1 on padding or exempt"):
        G.check_unpack_coverage(layout, counts(REAL), exempt=("c",))


def _bound(G):
    t = {k: torch.zeros(n, dtype=dt) for k, n, dt in (("x", 64, G.BF16), ("s", 64, G.BF16), ("y", 64, G.BF16), ("m", 64, torch.float32),
                                                        ("r", 64, G.BF16), ("w", 256, G.BF16), ("b", 16, torch.float32), ("g", 512, torch.float32),
                                                        ("dy", 64, G.BF16))}
    kt, nt = torch.zeros(8, 4, dtype=torch.int32), torch.zeros(8, 4, dtype=torch.int32)
    p = lambda k: t[k].data_ptr()
    d = G.fill_desc([(p("x"), 7, 4, 8, 1, 8), (p("s"), 6, 4, 16, 0, 6)],
                    [(p("y"), 7, 8, 4, 1, 2, 1, 2, 0), (p("m"), 9, 2, 2, 3, 1, 0, 1, 1)],
                    G.row_ptr(kt, 3), G.row_ptr(nt, 2), G.row_ptr(t["w"], 64), G.row_ptr(t["b"], 4), 56, 12, 16, 64, 7, 4, 2, 3, p("r"))
    return t, kt, nt, d


def test_fill_desc_reads_back_field_by_field(G):
    t, kt, nt, d = _bound(G)
    p = lambda k: t[k].data_ptr()
    src = [(s.ptr, s.T, s.F, s.C, s.tlo, s.thi, s.pad_) for s in d.src]
    assert src == [(p("x"), 7, 4, 8, 1, 8, 0), (p("s"), 6, 4, 16, 0, 6, 0), (None, 0, 0, 0, 0, 0, 0), (None, 0, 0, 0, 0, 0, 0)]
    dst = [(o.ptr, o.T, o.F, o.C, o.toff, o.fmul, o.fadd, o.tmul, o.is_f32) for o in d.dst]
    assert dst == [(p("y"), 7, 8, 4, 1, 2, 1, 2, 0), (p("m"), 9, 2, 2, 3, 1, 0, 1, 1)]
    assert (d.ktab, d.ntab) == (kt.data_ptr() + 3 * 16, nt.data_ptr() + 2 * 16)
    assert (d.W, d.bias, d.res) == (p("w") + 2 * 64, p("b") + 4 * 4, p("r"))
    assert (d.M, d.N, d.Npad, d.K, d.TT, d.J, d.fmul, d.tmul) == (56, 12, 16, 64, 7, 4, 2, 3)
    own = {"src", "dst", "ktab", "ntab", "W", "bias", "res", "M", "N", "Npad", "K", "TT", "J", "fmul", "tmul", "cv_toff"}
    assert all(not getattr(d, name) for name, _ in G.CGemmDesc._fields_ if name not in own)      # everything else: zero / NULL
    assert [list(r) for r in d.cv_toff] == [[0, 0], [0, 0]]
    assert G.row_ptr(t["w"], None) is None
    e = G.fill_desc([(p("x"), 7, 4, 8, 0, 7)], [(p("y"), 7, 8, 4, 0, 1, 0, 1, 0)], G.row_ptr(kt, 0), G.row_ptr(nt, 0), None, None,
                    1, 2, 16, 64, 7, 4, 1, 1)
    assert (e.W, e.bias, e.res, e.src[1].ptr, e.dst[1].ptr) == (None,) * 5


def test_a_twin_differs_in_dw_dbias_and_the_first_destination_only(G):
    t, kt, nt, d = _bound(G)
    d.dst[0].is_f32 = 1                            # (so that the twin's bf16 dOut shows)
    d.w_tiled, d.dense_rows, d.stats = 1, 1, t["g"].data_ptr()
    before = bytes(d)
    w = G.wgrad_twin(d, G.row_ptr(t["g"], 128), G.row_ptr(t["g"], 384), t["dy"].data_ptr())
    assert bytes(d) == before and w is not d       # the parent is left alone
    assert (w.dW, w.dbias, w.dst[0].ptr, w.dst[0].is_f32) == (t["g"].data_ptr() + 512, t["g"].data_ptr() + 1536, t["dy"].data_ptr(), 0)
    assert w.res == d.res                          # not normalised: a plan that wants it cleared clears it
    # put the four fields back: every other byte is the parent's
    w.dW, w.dbias, w.dst[0].ptr, w.dst[0].is_f32 = d.dW, d.dbias, d.dst[0].ptr, d.dst[0].is_f32
    assert bytes(w) == before
    # no dOut (a weight-gradient-only product keeps its destination), no bias gradient
    k = G.wgrad_twin(d, G.row_ptr(t["g"], 0))
    assert (k.dW, k.dbias, k.dst[0].ptr, k.dst[0].is_f32) == (t["g"].data_ptr(), None, d.dst[0].ptr, 1)
    k.dW = None
    assert bytes(k) == before
    assert C.sizeof(G.CGemmDesc) == len(before)
