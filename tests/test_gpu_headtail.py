"""GPU: every entry point of csrc/pack.hip and csrc/optim.hip on synthetic tables against tests/headtail_ref.py, a plain numpy
restatement that shares no code with the kernels (tests/test_headtail_host.py proves it on the CPU).  The gathers and the roundings to
bf16 are compared BIT FOR BIT; the sums are taken over integer gradients whose fp32 partial sums are exact in any order, so they are
compared for EQUALITY; the optimizer update is compared element by element with float64 inside bounds derived from the roundings of
opt_step_kernel, which torch.optim in float32 meets on the same inputs (host file).  Every output buffer sits between two runs of 64
canary elements that must come back untouched.  All calls go through sehip._lib.call.

Entry point                      covered by
  sehip_pack_bf16                test_pack_bf16, test_plan_tables_dccrn
  sehip_pack_f32                 test_pack_f32, test_plan_tables_demucs
  sehip_pack_head                test_pack_head, test_plan_tables_dccrn
  sehip_pack_bf16_runs           test_pack_runs
  sehip_pack_bf16_runs_to        test_pack_runs, test_plan_tables_demucs
  sehip_unpack_grad              test_unpack
  sehip_unpack_grad1             test_unpack
  sehip_unpack_grad_list         test_unpack
  sehip_unpack_grad_sums         test_unpack_sums, test_fused_entry_points_refuse_under_the_deterministic_flag
  sehip_unpack_grad_sums_perm    test_unpack_sums, test_fused_entry_points_refuse_under_the_deterministic_flag
  sehip_unpack_grad1_sums        test_unpack1_sums, test_fused_entry_points_refuse_under_the_deterministic_flag
  sehip_unpack_grad_list_sums    test_unpack1_sums
  sehip_grad_sumsq(_acc)         test_sumsq_and_metric
  sehip_grad_metric(_acc)        test_sumsq_and_metric
  sehip_opt_step                 test_opt_step_axes, test_opt_step_sizes_small, test_opt_step_sizes_large, test_opt_step_alignment
  sehip_opt_step_g               test_opt_step_axes, test_opt_step_sizes_small, test_opt_step_from_a_later_step, test_opt_step_guard
  sehip_opt_step_m               test_opt_step_axes, test_opt_step_sizes_small, test_opt_step_sizes_large, test_opt_step_guard
  sehip_opt_begin(_g)            test_opt_begin
  sehip_zero_regions             test_zero_regions
  sehip_counter_add              test_counter_add
(sehip_det_finish is internal.)  test_argument_checks_refuse_before_anything_is_launched goes through the refusals and the empty
problems of most of them."""
import functools
import itertools

import numpy as np
import pytest
import torch

import headtail_ref as R

pytestmark = pytest.mark.gpu

F32 = np.float32
PAD = 64
CANARY = {torch.float32: 12345.0, torch.float64: 777.0, torch.int16: 0x7B7B, torch.int32: 0x5A5A5A5A}


def _lib():
    from sehip._lib import call, stream, SehipError
    return call, stream, SehipError


class Buf:
    """n elements on the device between two runs of PAD canary elements; shift: the payload starts `shift` elements off 16 bytes"""

    def __init__(self, n, dtype=torch.float32, init=None, shift=0):
        self.n, self.lo = int(n), PAD + shift
        self.full = torch.full((self.n + 2 * PAD + shift,), CANARY[dtype], dtype=dtype, device="cuda")
        self.t = self.full[self.lo:self.lo + self.n]
        assert self.full.data_ptr() % 16 == 0
        if init is not None:
            self.put(init)

    def put(self, a):
        self.t.copy_(torch.from_numpy(np.ascontiguousarray(a)).view(self.t.dtype).reshape(-1))

    @property
    def ptr(self):
        return self.t.data_ptr()

    def get(self):
        return self.t.cpu().numpy().copy()

    def bits(self):
        a = self.get()
        return a.view(np.uint16) if a.dtype == np.int16 else a

    def intact(self):
        c = CANARY[self.full.dtype]
        return bool((self.full[:self.lo] == c).all()) and bool((self.full[self.lo + self.n:] == c).all())


_alive = []


@pytest.fixture(autouse=True)
def _inputs_live_as_long_as_the_test():
    """dev() hands out tensors whose pointer goes into a launch at once: they are kept until the test is over, or the allocator would
    give the memory of one input to the next"""
    yield
    torch.cuda.synchronize()
    _alive.clear()


def dev(a):
    """a read-only input on the device (tables, packed buffers); None for an empty one"""
    a = np.array(a, copy=True, order="C")                   # (a copy: the shared cases are write-protected)
    if not a.size:
        return None
    _alive.append(torch.from_numpy(a).cuda())
    return _alive[-1]


def p(t):
    return None if t is None else t.data_ptr()


def assert_bf16(buf, want, what):
    torch.cuda.synchronize()
    got = buf.bits()
    bad = R.bf16_mismatch(got, want)
    assert bad.size == 0, (what, bad.size, [(int(i), hex(got[i]), hex(want[i])) for i in bad[:8]])
    assert buf.intact(), what


def assert_f32(buf, want, what):
    torch.cuda.synchronize()
    got = buf.get()
    bad = R.f32_mismatch(got, want)
    assert bad.size == 0, (what, bad.size, [(int(i), float(got[i]), float(want[i])) for i in bad[:8]])
    assert buf.intact(), what


# ---- a. packing --------------------------------------------------------------------------------------------------------------------
# The parameters begin with headtail_ref.value_list(): signed zeros, infinities, NaN (NaN out, whichever), bf16 ties to an even and to
# an odd mantissa, the neighbours of the bf16 overflow threshold, float32 subnormals.  Everything is round to nearest even, the
# subnormals included: the conversion instruction of gfx950 does not flush them, so there is no "or signed zero" allowance here.
N_SRC = 20011
SPECIALS = len(R.value_list())


@pytest.mark.parametrize("n", [5, 8, 1029, 4096 * 256 * 8 + 13])           # the last: more than 4096 workgroups of 256 threads x 8
def test_pack_bf16(n):
    call, stream, _ = _lib()
    rng = np.random.default_rng(n)
    params = R.params_with_specials(N_SRC, rng)
    tab = R.entries(n, N_SRC, rng, specials=SPECIALS)
    assert (tab == 1).any() and (tab == -1).any() and ((tab & 1) == 1).any() and (n < 100 or (tab >> 1 == N_SRC // 2).sum() > 10)
    out = Buf(n, torch.int16)
    call("sehip_pack_bf16", p(dev(params)), p(dev(tab)), n, out.ptr, stream())
    assert_bf16(out, R.pack_bf16(params, tab), n)


@pytest.mark.parametrize("n", [1, 257, 70001])
def test_pack_f32(n):
    call, stream, _ = _lib()
    rng = np.random.default_rng(n)
    params = R.params_with_specials(N_SRC, rng)
    tab = R.entries(2 * n, N_SRC, rng, p_absent=0.35, specials=SPECIALS).reshape(n, 2)
    if n >= 3:
        tab[0], tab[1, 1], tab[2] = (-1, -1), -1, (2 * SPECIALS + 2, 2 * SPECIALS + 5)   # no term, one term, two terms
        terms = (tab >= 0).sum(1)
        assert all((terms == k).any() for k in (0, 1, 2))
    out = Buf(n)
    call("sehip_pack_f32", p(dev(params)), p(dev(tab)), n, out.ptr, stream())
    assert_f32(out, R.pack_f32(params, tab), n)


@pytest.mark.parametrize("nw,nb,nz", [(1029, 257, 1000), (0, 70001, 0), (8, 0, 300001), (0, 0, 5)])   # the grid follows nw alone
def test_pack_head(nw, nb, nz):
    call, stream, _ = _lib()
    rng = np.random.default_rng(nw + nb + nz)
    params = R.params_with_specials(N_SRC, rng)
    wtab = R.entries(nw, N_SRC, rng, specials=SPECIALS)
    btab = R.entries(2 * nb, N_SRC, rng, p_absent=0.35, specials=SPECIALS).reshape(nb, 2)
    wout, bout, zero = Buf(nw, torch.int16), Buf(nb), Buf(nz, init=np.full(nz, 3.5, dtype=F32))
    call("sehip_pack_head", p(dev(params)), p(dev(wtab)), nw, wout.ptr if nw else None, p(dev(btab)), nb, bout.ptr if nb else None,
         zero.ptr if nz else None, nz, stream())
    assert_bf16(wout, R.pack_bf16(params, wtab), "weights")
    assert_f32(bout, R.pack_f32(params, btab), "biases")
    assert_f32(zero, np.zeros(nz, dtype=F32), "cleared region")


@pytest.mark.parametrize("n8", [1, 300, 256 * 256 + 77])                    # the last: more runs than 256 workgroups x 256 threads
def test_pack_runs(n8):
    call, stream, SehipError = _lib()
    rng = np.random.default_rng(n8)
    params = R.params_with_specials(N_SRC, rng)
    runs, side = R.run_table(n8, N_SRC, rng)
    if n8 >= 3:
        assert (runs[:, 0] >= 0).any() and (runs[:, 0] == -1).any() and (runs[:, 0] <= -2).any()
        assert set(runs[runs[:, 0] >= 0, 1].tolist()) == {1, 8, 24, 513}
    d_params, d_runs, d_side = dev(params), dev(runs), dev(side)
    out = Buf(8 * n8, torch.int16)
    call("sehip_pack_bf16_runs", p(d_params), p(d_runs), p(d_side), 8 * n8, out.ptr, stream())
    assert_bf16(out, R.pack_runs(params, runs, side), "table order")
    dst = rng.permutation(n8).astype(np.int32)
    out = Buf(8 * n8, torch.int16)
    call("sehip_pack_bf16_runs_to", p(d_params), p(d_runs), p(dev(dst)), p(d_side), 8 * n8, out.ptr, stream())
    assert_bf16(out, R.pack_runs(params, runs, side, dst), "through the destination table")
    # refusals: a size that is no multiple of 8, a missing destination table; nothing is written
    out = Buf(8 * n8, torch.int16)
    with pytest.raises(SehipError, match="multiple of 8"):
        call("sehip_pack_bf16_runs", p(d_params), p(d_runs), p(d_side), 8 * n8 - 3, out.ptr, stream())
    with pytest.raises(SehipError, match="destination"):
        call("sehip_pack_bf16_runs_to", p(d_params), p(d_runs), None, p(d_side), 8 * n8, out.ptr, stream())
    torch.cuda.synchronize()
    assert (out.t == CANARY[torch.int16]).all() and out.intact()


# ---- b. un-packing -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 4099, 1100003])
def test_unpack(n):
    call, stream, _ = _lib()
    rng = np.random.default_rng(n)
    n_src = n + 500
    packed = rng.standard_normal(n_src).astype(F32)
    tab4 = R.rows4(n, n_src, rng)
    if n == 3:
        tab4[0], tab4[1, 1:] = -1, (7, -1, -1)
    terms = (tab4 >= 0).sum(1)
    assert (terms == 0).any() and (n < 100 or all((terms == k).any() for k in (1, 2, 3, 4)))
    want = R.unpack(packed, tab4)
    assert (want[terms == 0].view(np.uint32) == 0).all()
    d_packed = dev(packed)
    grads = Buf(n)
    call("sehip_unpack_grad", p(d_packed), p(dev(tab4)), n, grads.ptr, stream())
    assert_f32(grads, want, "four-entry table")
    # the one-entry form: the first entry of every parameter, then the rows with more by index
    tab1 = np.ascontiguousarray(tab4[:, 0])
    lst = np.flatnonzero(terms >= 2).astype(np.int32)
    grads = Buf(n)
    call("sehip_unpack_grad1", p(d_packed), p(dev(tab1)), n, grads.ptr, stream())
    first = R.unpack1(packed, tab1)
    assert_f32(grads, first, "one-entry table")
    call("sehip_unpack_grad_list", p(d_packed), p(dev(lst)), p(dev(tab4[lst])), lst.size, grads.ptr, stream())
    assert_f32(grads, R.unpack_list(packed, lst, tab4[lst], first), "index list")
    assert R.f32_mismatch(R.unpack_list(packed, lst, tab4[lst], first), want).size == 0


# ---- c. un-packing with sums: integer gradients, equality ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def integer_case(which):
    case = R.integer_case(*R.INTEGER_CASES[which])
    cond = R.integer_conditions(case)
    assert all(cond.values()), cond                       # non-zero integers, sum |g| and sum g^2 below 2^24, the size list's conditions
    g = R.unpack(case["packed"], case["tab4"])
    case.update(g=g, tsums=R.tensor_sums(g, case["offsets"]), sumsq=R.sumsq(g), n=g.size, nt=len(case["sizes"]))
    for a in case.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return case


PRE_TSUM, PRE_SUMSQ = 3.0, 11.0                           # what the accumulators hold before a launch that adds to them


def _accumulators(nt):
    return Buf(1, torch.float64, init=np.array([PRE_SUMSQ])), Buf(nt, init=np.full(nt, PRE_TSUM, dtype=F32))


def _assert_sums(case, sumsq, tsums, pre, what):
    torch.cuda.synchronize()
    assert float(sumsq.get()[0]) == pre * PRE_SUMSQ + case["sumsq"], what
    got = tsums.get().astype(np.float64)
    bad = np.flatnonzero(got != pre * PRE_TSUM + case["tsums"])
    assert bad.size == 0, (what, [(int(t), got[t], case["tsums"][t], case["sizes"][t]) for t in bad[:8]])
    assert sumsq.intact() and tsums.intact(), what


@pytest.mark.parametrize("variant", ["plain", "perm"])
@pytest.mark.parametrize("which", ["small", "large"])
def test_unpack_sums(which, variant):
    call, stream, _ = _lib()
    c = integer_case(which)
    n, nt = c["n"], c["nt"]
    d_packed, d_off = dev(c["packed"]), dev(c["offsets"])
    d_tab = dev(c["tab4p"] if variant == "perm" else c["tab4"])
    d_perm = dev(c["perm"])
    # the guard word: absent, zero (the step counts), non-zero (it does not); the un-pack itself happens every time
    for guard, counts in ((None, 1), (0, 1), (9, 0)):
        grads, counter = Buf(n), Buf(1, torch.int32, init=np.array([7], dtype=np.int32))
        sumsq, tsums = _accumulators(nt)
        d_guard = None if guard is None else dev(np.array([guard], dtype=np.uint32).view(np.int32))
        if variant == "perm":
            call("sehip_unpack_grad_sums_perm", p(d_packed), p(d_tab), p(d_perm), n, grads.ptr, p(d_off), nt, sumsq.ptr, tsums.ptr,
                 counter.ptr, p(d_guard), stream())
        else:
            call("sehip_unpack_grad_sums", p(d_packed), p(d_tab), n, grads.ptr, p(d_off), nt, sumsq.ptr, tsums.ptr, counter.ptr,
                 p(d_guard), stream())
        assert_f32(grads, c["g"], (variant, guard))         # the perm variant's gradients are the plain variant's
        _assert_sums(c, sumsq, tsums, 1, (variant, guard))
        assert int(counter.get()[0]) == 7 + counts and counter.intact(), guard
    # without a counter
    grads = Buf(n)
    sumsq, tsums = _accumulators(nt)
    if variant == "perm":
        call("sehip_unpack_grad_sums_perm", p(d_packed), p(d_tab), p(d_perm), n, grads.ptr, p(d_off), nt, sumsq.ptr, tsums.ptr, None, None,
             stream())
    else:
        call("sehip_unpack_grad_sums", p(d_packed), p(d_tab), n, grads.ptr, p(d_off), nt, sumsq.ptr, tsums.ptr, None, None, stream())
    assert_f32(grads, c["g"], variant)
    _assert_sums(c, sumsq, tsums, 1, variant)


@pytest.mark.parametrize("which", ["small", "large"])
def test_unpack1_sums(which):
    call, stream, _ = _lib()
    c = integer_case(which)
    n, nt = c["n"], c["nt"]
    d_packed, d_off, d_tab1, d_lst, d_tab4l = dev(c["packed"]), dev(c["offsets"]), dev(c["tab1"]), dev(c["lst"]), dev(c["tab4l"])
    assert c["lst"].size > 2 * nt
    for guard, counts in ((None, 1), (0, 1), (9, 0)):
        grads, counter = Buf(n), Buf(1, torch.int32, init=np.array([7], dtype=np.int32))
        sumsq, tsums = _accumulators(nt)
        d_guard = None if guard is None else dev(np.array([guard], dtype=np.uint32).view(np.int32))
        call("sehip_unpack_grad1_sums", p(d_packed), p(d_tab1), n, grads.ptr, p(d_off), nt, sumsq.ptr, tsums.ptr, counter.ptr, p(d_guard),
             stream())
        if guard is None:       # the first launch alone: the first entries and THEIR sums
            first = R.unpack1(c["packed"], c["tab1"])
            assert_f32(grads, first, "first entries")
            torch.cuda.synchronize()
            assert float(sumsq.get()[0]) == PRE_SUMSQ + R.sumsq(first)
            assert np.array_equal(tsums.get().astype(np.float64), PRE_TSUM + R.tensor_sums(first, c["offsets"]))
        call("sehip_unpack_grad_list_sums", p(d_packed), p(d_lst), p(d_tab4l), c["lst"].size, grads.ptr, p(d_off), nt, sumsq.ptr, tsums.ptr,
             stream())
        assert_f32(grads, c["g"], guard)
        _assert_sums(c, sumsq, tsums, 1, guard)
        assert int(counter.get()[0]) == 7 + counts and counter.intact(), guard


@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("which", ["small", "large"])
def test_sumsq_and_metric(which, deterministic):
    from sehip.utils import set_deterministic
    call, stream, _ = _lib()
    c = integer_case(which)
    n, nt = c["n"], c["nt"]
    d_g, d_off = dev(c["g"]), dev(c["offsets"])
    want = (float(np.sqrt((c["tsums"] ** 2).sum())), float(np.sqrt(c["sumsq"])))
    set_deterministic(deterministic)
    try:
        for fn_s, fn_m, pre in (("sehip_grad_sumsq", "sehip_grad_metric", 0), ("sehip_grad_sumsq_acc", "sehip_grad_metric_acc", 1)):
            sumsq, tsums = _accumulators(nt)                # the plain variants clear them, the _acc variants add
            metric = Buf(2)
            call(fn_s, p(d_g), n, sumsq.ptr, stream())
            call(fn_m, p(d_g), p(d_off), nt, int(max(c["sizes"])), sumsq.ptr, tsums.ptr, metric.ptr, stream())
            _assert_sums(c, sumsq, tsums, pre, (fn_s, deterministic))
            if pre == 0:
                m = metric.get().astype(np.float64)
                assert abs(m[0] - want[0]) <= 1e-5 * want[0] and abs(m[1] - want[1]) <= 1e-5 * want[1], m
            assert metric.intact()
        # a gradient range that starts in the middle of the buffer, 2 elements off 16 bytes for the per-tensor sums
        t0 = next(t for t in range(nt) if c["offsets"][t] % 4 == 2)
        sub_off = c["offsets"][t0:] - 0
        tsums, metric = Buf(nt - t0, init=np.full(nt - t0, PRE_TSUM, dtype=F32)), Buf(2)
        call("sehip_grad_metric", p(d_g), p(dev(sub_off)), nt - t0, int(max(c["sizes"][t0:])), None, tsums.ptr, metric.ptr, stream())
        torch.cuda.synchronize()
        assert np.array_equal(tsums.get().astype(np.float64), c["tsums"][t0:]) and tsums.intact()
        assert float(metric.get()[1]) == 0.0
    finally:
        set_deterministic(False)


def test_fused_entry_points_refuse_under_the_deterministic_flag():
    from sehip.utils import set_deterministic
    call, stream, SehipError = _lib()
    c = integer_case("small")
    n, nt = c["n"], c["nt"]
    d_packed, d_off, d_tab4, d_tab1, d_perm = dev(c["packed"]), dev(c["offsets"]), dev(c["tab4"]), dev(c["tab1"]), dev(c["perm"])
    grads, counter = Buf(n), Buf(1, torch.int32, init=np.array([7], dtype=np.int32))
    sumsq, tsums = _accumulators(nt)
    set_deterministic(True)
    try:
        with pytest.raises(SehipError, match="deterministic"):
            call("sehip_unpack_grad_sums", p(d_packed), p(d_tab4), n, grads.ptr, p(d_off), nt, sumsq.ptr, tsums.ptr, counter.ptr, None, stream())
        with pytest.raises(SehipError, match="deterministic"):
            call("sehip_unpack_grad_sums_perm", p(d_packed), p(d_tab4), p(d_perm), n, grads.ptr, p(d_off), nt, sumsq.ptr, tsums.ptr,
                 counter.ptr, None, stream())
        with pytest.raises(SehipError, match="deterministic"):
            call("sehip_unpack_grad1_sums", p(d_packed), p(d_tab1), n, grads.ptr, p(d_off), nt, sumsq.ptr, tsums.ptr, counter.ptr, None,
                 stream())
    finally:
        set_deterministic(False)
    torch.cuda.synchronize()
    assert (grads.t == CANARY[torch.float32]).all() and int(counter.get()[0]) == 7
    assert float(sumsq.get()[0]) == PRE_SUMSQ and (tsums.t == PRE_TSUM).all()


# ---- d. the optimizer update against float64 ------------------------------------------------------------------------------------------
WD = R.hyper(1e-2)
MOMENTUM = R.hyper(0.9)
N_MID, N_BIG = 40007, 2048 * 4096 + 4099
MODES = [("adam", None), ("sgd", 0.0), ("sgd", MOMENTUM)]
_worst = dict(p=0.0, g=0.0, m=0.0, v=0.0)
NT_OPT = 7                                                  # tensors the per-tensor sums of sehip_opt_step_m are taken over


def _opt_cfg(kind, b1, wd):
    if kind == "adam":
        return dict(mode=0, lr=R.ADAM["lr"], b1=R.ADAM["b1"], b2=R.ADAM["b2"], eps=R.ADAM["eps"], wd=wd)
    return dict(mode=1, lr=R.SGD_LR, b1=b1, b2=0.0, eps=0.0, wd=wd)


def opt_run(n, kind, b1, wd, clip, gscale, entry, step_from, shift=None, start=1, guard=None, seed=9):
    """3 consecutive steps of `entry` from non-zero m and v; every step is compared with the float64 step from the state the device
    held (float32) inside the gate's bounds.  step_from "device": the counter on the device decides, the host argument is wrong on
    purpose.  shift: which of p, g, m, v starts one float off 16 bytes."""
    call, stream, _ = _lib()
    cfg = _opt_cfg(kind, b1, wd)
    p0, m0, v0, gs = R.opt_inputs(n, seed)
    sh = lambda k: 1 if shift == k else 0
    bp, bg, bm, bv = Buf(n, init=p0, shift=sh("p")), Buf(n, shift=sh("g")), Buf(n, init=m0, shift=sh("m")), Buf(n, init=v0, shift=sh("v"))
    offsets = np.linspace(0, n, NT_OPT + 1).astype(np.int64)
    sumsq_d, metric, step_dev = Buf(1, torch.float64), Buf(2), Buf(1, torch.int32)
    nxt_sumsq, nxt_tsums = Buf(1, torch.float64), Buf(NT_OPT)
    d_guard = None if guard is None else dev(np.array([guard], dtype=np.uint32).view(np.int32))
    for k, g in enumerate(gs):
        step = start + k
        cfg["step"] = step
        cur = [b.get() for b in (bp, bg, bm, bv)]
        cur[1] = g
        bg.put(g)
        ss = R.sumsq(g)
        max_norm = R.clip_norm(clip, ss, gscale)
        sumsq_d.put(np.array([ss]))
        host_step = step
        if step_from == "device":
            step_dev.put(np.array([step], dtype=np.int32))
            host_step = 5 if step == 1 else 1
        head = (bp.ptr, bg.ptr, bm.ptr, bv.ptr, n, sumsq_d.ptr, max_norm, cfg["lr"], cfg["b1"], cfg["b2"], cfg["eps"], host_step,
                step_dev.ptr if step_from == "device" else None, wd, cfg["mode"], gscale)
        if entry == "sehip_opt_step":
            assert guard is None
            call(entry, *head, stream())
        elif entry == "sehip_opt_step_g":
            call(entry, *head, p(d_guard), stream())
        else:
            tsums32 = R.tensor_sums(g, offsets).astype(F32)
            nxt_sumsq.put(np.array([5.0])); nxt_tsums.put(np.full(NT_OPT, 5.0, dtype=F32))
            call(entry, *head, p(d_guard), p(dev(tsums32)), NT_OPT, metric.ptr, nxt_sumsq.ptr, nxt_tsums.ptr, stream())
        torch.cuda.synchronize()
        new = [b.get() for b in (bp, bg, bm, bv)]
        assert all(b.intact() for b in (bp, bg, bm, bv, sumsq_d, metric, step_dev, nxt_sumsq, nxt_tsums)), (entry, k)
        coef = R.clip_coef(ss, max_norm, gscale)
        if entry == "sehip_opt_step_m":
            want = (float(np.sqrt((tsums32.astype(np.float64) ** 2).sum()) * coef), float(np.sqrt(ss)))
            got = metric.get().astype(np.float64)
            assert abs(got[0] - want[0]) <= 1e-5 * want[0] and abs(got[1] - want[1]) <= 1e-5 * want[1], (got, want)
            assert float(nxt_sumsq.get()[0]) == 0.0 and (nxt_tsums.get() == 0).all()       # the next step's accumulators are cleared
        if guard:                                        # a guarded-out step applies nothing
            for a, b in zip(cur, new):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
            continue
        ref = R.opt_step(*cur, ss, max_norm, cfg["lr"], cfg["b1"], cfg["b2"], cfg["eps"], step, wd, cfg["mode"], gscale)
        bound = R.opt_bounds(ref, cur, cfg)
        for key, got, want in zip("pgmv", new, ref):
            if bound[key] is None:
                continue
            ratio = float((np.abs(got.astype(np.float64) - want) / bound[key]).max())
            _worst[key] = max(_worst[key], ratio)
            print(f"[headtail_gate] {entry} n={n} {kind} b1={b1} wd={wd} clip={clip} gscale={gscale} {step_from} shift={shift} step={step} "
                  f"{key}: error / bound = {ratio:.4f}")
            assert ratio <= 1.0, (key, ratio, entry, k)
        if cfg["mode"] == 1:
            assert np.array_equal(new[3].view(np.uint32), cur[3].view(np.uint32))           # SGD never touches v
        if coef == 1.0:
            assert np.array_equal(new[1].view(np.uint32), g.view(np.uint32))                # nothing to scale: g is not rewritten
        else:
            assert not np.array_equal(new[1], g)


ENTRIES = ["sehip_opt_step", "sehip_opt_step_g", "sehip_opt_step_m"]
AXES = list(itertools.product(MODES, [0.0, WD], ["off", "clips", "loose"], [1.0, 0.25]))


@pytest.mark.parametrize("i", range(len(AXES)), ids=lambda i: "{0[0]}-{0[1]}-wd{1}-{2}-gs{3}".format(*AXES[i]).replace("None", "x"))
def test_opt_step_axes(i):
    """mode x weight decay x clipping x gradient scale in full; the entry point and the source of the step number go round with the
    case number, so that every one of them meets every mode, every weight decay and every kind of clipping"""
    (kind, b1), wd, clip, gscale = AXES[i]
    entry = ENTRIES[(i + i // 12) % 3]
    step_from = ("host", "device")[(i // 2 + i // 12) % 2]
    opt_run(N_MID, kind, b1, wd, clip, gscale, entry, step_from, start=1)


@pytest.mark.parametrize("step_from", ["host", "device"])
@pytest.mark.parametrize("kind,b1", MODES)
def test_opt_step_from_a_later_step(kind, b1, step_from):
    """steps 6, 7, 8: SGD's buffer is m * momentum + g from the first of them on, Adam's bias corrections are those of the step"""
    opt_run(N_MID, kind, b1, WD, "clips", 1.0, "sehip_opt_step_g", step_from, start=6)


@pytest.mark.parametrize("shift", [None, "p", "g", "m", "v"])
@pytest.mark.parametrize("kind,b1", [("adam", None), ("sgd", MOMENTUM)])
def test_opt_step_alignment(kind, b1, shift):
    """all four buffers on 16 bytes (vector path, n % 4 tail), or one of them one float off (scalar path for everything)"""
    opt_run(N_MID, kind, b1, WD, "clips", 0.25, "sehip_opt_step", "host", shift=shift)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("kind,b1", MODES)
def test_opt_step_sizes_small(kind, b1, entry):
    opt_run(3, kind, b1, WD, "clips", 0.25, entry, "device", start=1)


@pytest.mark.parametrize("kind,b1,entry", [("adam", None, "sehip_opt_step_m"), ("sgd", MOMENTUM, "sehip_opt_step")])
def test_opt_step_sizes_large(kind, b1, entry):
    """more quads than 2048 workgroups x 256 threads: the grid-stride loop, and the n % 4 = 3 tail behind it"""
    opt_run(N_BIG, kind, b1, WD, "clips", 0.25, entry, "device", start=1)


@pytest.mark.parametrize("entry", ["sehip_opt_step_g", "sehip_opt_step_m"])
@pytest.mark.parametrize("kind,b1", [("adam", None), ("sgd", MOMENTUM)])
def test_opt_step_guard(kind, b1, entry):
    """a non-zero guard word: p, g, m, v bit-unchanged, the metric still written and the next accumulators still cleared; a zero word
    is no guard"""
    opt_run(N_MID, kind, b1, WD, "clips", 1.0, entry, "device", guard=3)
    opt_run(N_MID, kind, b1, WD, "clips", 1.0, entry, "device", guard=0)


def test_opt_step_worst_ratios_are_reported():
    """(runs after the gates above in file order; the figures are those of profiles/headtail_gate.json)"""
    print("[headtail_gate] device " + " ".join(f"{k}={v:.4f}" for k, v in _worst.items()))
    assert max(_worst.values()) <= 1.0


# ---- e. small launches ---------------------------------------------------------------------------------------------------------------
def test_zero_regions():
    call, stream, SehipError = _lib()
    big = 1024 * 256 * 4 + 7                               # more float4s than 1024 workgroups x 256 threads, and a 3-float tail
    bufs = [Buf(1, init=np.full(1, 2.5, dtype=F32)), Buf(3, init=np.full(3, 2.5, dtype=F32)), Buf(big, init=np.full(big, 2.5, dtype=F32))]
    call("sehip_zero_regions", bufs[0].ptr, 4, bufs[1].ptr, 12, None, 0, bufs[2].ptr, 4 * big, stream())
    for b in bufs:
        assert_f32(b, np.zeros(b.n, dtype=F32), b.n)
    keep = Buf(8, init=np.full(8, 2.5, dtype=F32))
    with pytest.raises(SehipError, match="aligned"):
        call("sehip_zero_regions", keep.ptr + 4, 8, None, 0, None, 0, None, 0, stream())
    with pytest.raises(SehipError, match="multiple of 4"):
        call("sehip_zero_regions", keep.ptr, 6, None, 0, None, 0, None, 0, stream())
    assert_f32(keep, np.full(8, 2.5, dtype=F32), "refused")


def test_opt_begin():
    call, stream, _ = _lib()
    nt = 300                                               # more tensors than the launch has threads
    for fn, guard, value, want in (("sehip_opt_begin", None, 1, 8), ("sehip_opt_begin", None, 0, 7), ("sehip_opt_begin_g", None, 1, 8),
                                   ("sehip_opt_begin_g", 0, 1, 8), ("sehip_opt_begin_g", 9, 1, 7)):
        counter = Buf(1, torch.int32, init=np.array([7], dtype=np.int32))
        sumsq, tsums = _accumulators(nt)
        d_guard = None if guard is None else dev(np.array([guard], dtype=np.uint32).view(np.int32))
        tail = (p(d_guard), stream()) if fn.endswith("_g") else (stream(),)
        call(fn, counter.ptr, value, sumsq.ptr, tsums.ptr, nt, *tail)
        torch.cuda.synchronize()
        assert int(counter.get()[0]) == want, (fn, guard, value)
        assert float(sumsq.get()[0]) == 0.0 and (tsums.get() == 0).all()         # cleared whatever the guard says
        assert counter.intact() and sumsq.intact() and tsums.intact()
    # every pointer is optional
    sumsq, tsums = _accumulators(nt)
    call("sehip_opt_begin", None, 1, None, tsums.ptr, nt, stream())
    torch.cuda.synchronize()
    assert (tsums.get() == 0).all() and float(sumsq.get()[0]) == PRE_SUMSQ


def test_counter_add():
    call, stream, SehipError = _lib()
    counter = Buf(1, torch.int32, init=np.array([7], dtype=np.int32))
    call("sehip_counter_add", counter.ptr, 3, stream())
    call("sehip_counter_add", counter.ptr, -1, stream())
    torch.cuda.synchronize()
    assert int(counter.get()[0]) == 9 and counter.intact()
    with pytest.raises(SehipError, match="null"):
        call("sehip_counter_add", None, 1, stream())


def test_argument_checks_refuse_before_anything_is_launched():
    call, stream, SehipError = _lib()
    src, tab = dev(np.ones(64, dtype=F32)), dev(np.zeros(64, dtype=np.int32))
    out, g, sumsq = Buf(64, torch.int16), Buf(64), Buf(1, torch.float64)
    four = (g.ptr, g.ptr, g.ptr, g.ptr)
    adam = (1e-3, 0.9, 0.999, 1e-8)
    for name, args, msg in (
            ("sehip_pack_bf16", (p(src), p(tab), 16, out.ptr + 2), "aligned"),
            ("sehip_pack_bf16", (p(src), p(tab), -1, out.ptr), "negative"),
            ("sehip_pack_head", (p(src), p(tab) + 4, 16, out.ptr, None, 0, None, None, 0), "aligned"),
            ("sehip_pack_bf16_runs", (p(src), p(tab) + 4, p(tab), 16, out.ptr), "misaligned"),
            ("sehip_unpack_grad1", (p(src), p(tab), 16, g.ptr + 4), "aligned"),
            ("sehip_unpack_grad1_sums", (p(src), p(tab), 16, g.ptr + 4, p(tab), 1, sumsq.ptr, g.ptr, None, None), "aligned"),
            ("sehip_unpack_grad_sums", (p(src), p(tab), 16, g.ptr, p(tab), 0, sumsq.ptr, g.ptr, None, None), "bad arguments"),
            ("sehip_grad_sumsq_acc", (g.ptr + 4, 16, sumsq.ptr), "aligned"),
            ("sehip_grad_metric", (g.ptr, p(tab), 0, 1, sumsq.ptr, g.ptr, g.ptr), "no tensors"),
            ("sehip_opt_step", four + (16, sumsq.ptr, 0.0) + adam + (0, None, 0.0, 0, 1.0), "bad n/step"),
            ("sehip_opt_step", four + (16, sumsq.ptr, 0.0) + adam + (1, None, 0.0, 2, 1.0), "mode must be"),
            ("sehip_opt_step", four + (16, sumsq.ptr, 0.0) + adam + (1, None, 0.0, 0, 0.0), "grad_scale"),
            ("sehip_opt_step", four + (16, None, 5.0) + adam + (1, None, 0.0, 0, 1.0), "clipping needs"),
            ("sehip_opt_step_m", four + (16, sumsq.ptr, 0.0) + adam + (1, None, 0.0, 0, 1.0, None, None, 1, None, None, None), "bad arguments")):
        with pytest.raises(SehipError, match=msg):
            call(name, *args, stream())
    # an empty problem is no error and no launch
    call("sehip_pack_bf16", None, None, 0, None, stream())
    call("sehip_pack_f32", None, None, 0, None, stream())
    call("sehip_unpack_grad", None, None, 0, None, stream())
    call("sehip_unpack_grad_list", None, None, None, 0, None, stream())
    call("sehip_opt_step", None, None, None, None, 0, None, 0.0, *adam, 1, None, 0.0, 0, 1.0, stream())
    torch.cuda.synchronize()
    assert (out.t == CANARY[torch.int16]).all() and (g.t == CANARY[torch.float32]).all() and out.intact() and g.intact()
    assert float(sumsq.get()[0]) == CANARY[torch.float64]


# ---- f. the plans' own tables ----------------------------------------------------------------------------------------------------------
def _bf16_bits(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def test_plan_tables_dccrn():
    """the smallest DCCRN of tests/test_gpu_fused_tail.py: what one forward pass packed is the reference on the plan's tables"""
    from sehip.model import DCCRN
    torch.manual_seed(5)
    model = DCCRN(kernel_num=[16, 16, 32, 32, 64, 64], rnn_units=128, length=4000).cuda().train()
    model((0.1 * torch.randn(2, 1, 4000)).cuda())
    torch.cuda.synchronize()
    st, tb = model.static, model.workspace(2, 4000).tb
    flat = model.flat_params.detach().cpu().numpy()
    assert ((st.wtab >= 0) & (st.wtab & 1 == 1)).any()                                      # the complex block matrix negates
    assert R.bf16_mismatch(_bf16_bits(tb.wpack)[:st.n_wpack], R.pack_bf16(flat, st.wtab[:st.n_wpack])).size == 0
    assert R.f32_mismatch(tb.bpack.cpu().numpy()[:st.n_bpack], R.pack_f32(flat, st.btab.reshape(-1, 2)[:st.n_bpack])).size == 0


def test_plan_tables_demucs():
    """the smallest Demucs of tests/test_gpu_deterministic.py: run descriptors, side entries and the destination table"""
    from sehip.model import Demucs
    torch.manual_seed(5)
    model = Demucs(sources=["clean"], audio_channels=2, channels=32, depth=4).cuda().train()
    model((0.1 * torch.randn(3, 2, 9000)).cuda())
    torch.cuda.synchronize()
    st, tb = model.static, model._tables
    flat = model.flat_params.detach().cpu().numpy()
    n = st.n_wpack_dev
    want = R.pack_runs(flat, st.runs, st.side, st.pack_dst)
    assert want.size == n and R.bf16_mismatch(want, R.pack_bf16(flat, st.wtab[:n])).size == 0
    assert R.bf16_mismatch(_bf16_bits(tb.wpack)[:n], want).size == 0
    assert R.f32_mismatch(tb.bpack.cpu().numpy()[:st.n_bpack], R.pack_f32(flat, st.btab.reshape(-1, 2)[:st.n_bpack])).size == 0
