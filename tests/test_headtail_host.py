"""CPU: tests/headtail_ref.py, the reference of tests/test_gpu_headtail.py, against what is already trusted -- torch.optim.Adam / SGD in
float64, tests/cabi_emulator.py's table calls, the run decoding of tests/test_host_plan_demucs.py -- and the proof that the bounds of the
optimizer gate can be met: torch.optim in float32 on the gate's own inputs stays inside them.  The worst error / bound ratios it prints
are the "cpu_float32" half of profiles/headtail_gate.json."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import headtail_ref as R

F32 = np.float32
WD = R.hyper(1e-2)
MOMENTUM = R.hyper(0.9)
N_MID = 40007


def test_bf16_bits_is_round_to_nearest_even_on_the_special_values():
    want = [0x0000, 0x8000, 0x7F80, 0xFF80, 0x7FC0, 0x3F80, 0xBF80, 0x3F82, 0xBF82, 0x3F81, 0x3F80, 0x7F7F, 0x7F80, 0x7F80, 0xFF7F,
            0xFF80, 0x0000, 0x8000, 0x0080, 0x0000, 0x0002, 0x8080]
    got = R.bf16_bits(R.value_list())
    assert R.bf16_mismatch(got, want).size == 0, [hex(x) for x in got]
    assert (got[4] & 0x7F80) == 0x7F80 and (got[4] & 0x7F) != 0            # NaN stays NaN; which NaN is the converter's business
    assert R.bf16_mismatch([0x7F80, 0x3F80], [0x7FC0, 0x3F81]).tolist() == [0, 1]
    assert R.is_subnormal(R.value_list()).tolist() == [False] * 16 + [True] * 6


def test_term_negates_the_sign_bit_and_absent_is_zero():
    src = R.value_list()
    e = np.arange(2 * src.size)
    got = R.term(src, e).view(np.uint32).reshape(-1, 2)
    assert np.array_equal(got[:, 0], src.view(np.uint32)) and np.array_equal(got[:, 1], src.view(np.uint32) ^ 0x80000000)
    assert R.term(src, [-1, 1]).view(np.uint32).tolist() == [0, 0x80000000]
    # the fixed order of the four terms: ((x + y) + z) + w
    packed = np.array([1.0, 2.0 ** -24, 2.0 ** -24, -1.0], dtype=F32)
    assert R.unpack(packed, [[0, 2, 4, 6]])[0] == 0.0 and R.unpack(packed, [[2, 4, 0, 6]])[0] == F32(2.0 ** -23)


# ---- the update in float64 against torch.optim --------------------------------------------------------------------------------------
def _torch_opt(kind, p, m, v, start, lr, b1, b2, eps, wd, dtype):
    pt = torch.tensor(p, dtype=dtype, requires_grad=True)
    if kind == "adam":
        opt = torch.optim.Adam([pt], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
        opt.state[pt] = dict(step=torch.tensor(float(start - 1)), exp_avg=torch.tensor(m, dtype=dtype), exp_avg_sq=torch.tensor(v, dtype=dtype))
    else:
        opt = torch.optim.SGD([pt], lr=lr, momentum=b1, weight_decay=wd)
        if b1 != 0 and start > 1:
            opt.state[pt] = dict(momentum_buffer=torch.tensor(m, dtype=dtype))
    return pt, opt


def _torch_state(kind, pt, opt, b1):
    st = opt.state[pt]
    p = pt.detach().numpy().copy()
    if kind == "adam":
        return p, st["exp_avg"].numpy().copy(), st["exp_avg_sq"].numpy().copy()
    return p, (st["momentum_buffer"].numpy().copy() if b1 != 0 else None), None


@pytest.mark.parametrize("start", [1, 3])
@pytest.mark.parametrize("gscale", [1.0, 0.25])
@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("kind,b1", [("adam", 0.9), ("sgd", 0.0), ("sgd", 0.9)])
def test_opt_step_in_float64_is_torch_optim_in_float64(kind, b1, wd, gscale, start):
    n = 1031
    p32, m32, v32, gs = R.opt_inputs(n, 5, steps=4)
    gs[1] = gs[1] * F32(40.0)                                       # the clip bites on the second step only
    p, m, v = (a.astype(np.float64) for a in (p32, m32, v32))
    lr, b2, eps, mode = (3e-3, 0.999, 1e-8, 0) if kind == "adam" else (1e-2, 0.0, 0.0, 1)
    pt, opt = _torch_opt(kind, p, m, v, start, lr, b1, b2, eps, wd, torch.float64)
    max_norm = 5.0
    clipped = []
    for k, g in enumerate(gs):
        ss = R.sumsq(g)
        coef = R.clip_coef(ss, max_norm, gscale)
        clipped.append(coef != gscale)
        p, gc, m, v, dp = R.opt_step(p, g, m, v, ss, max_norm, lr, b1, b2, eps, start + k, wd, mode, gscale)
        assert np.array_equal(gc, g.astype(np.float64) * coef)
        pt.grad = torch.tensor(g.astype(np.float64) * coef)
        opt.step()
        tp, tm, tv = _torch_state(kind, pt, opt, b1)
        for got, want in ((p, tp), (m, tm), (v, tv)):
            if want is not None:
                assert (np.abs(got - want) <= 1e-12 * np.abs(want)).all(), (kind, k)
    assert clipped == [False, True, False, False]


# ---- the optimizer gate's bounds can be met: torch.optim in float32 on the gate's inputs ------------------------------------------------
def _coef32(ss, max_norm, gscale):
    """the clipping coefficient as an fp32 implementation computes it"""
    c = F32(gscale)
    if max_norm > 0:
        c = F32(gscale) * min(F32(1), F32(max_norm) / (F32(np.sqrt(ss)) * F32(gscale) + F32(1e-6)))
    return F32(c)


def float32_run(n, kind, b1, wd, clip, gscale, start=1, seed=9):
    """3 steps of torch.optim in float32 on opt_inputs(n); every step is compared with the float64 step FROM THE SAME float32 STATE.
    -> worst error / bound per quantity"""
    p, m, v, gs = R.opt_inputs(n, seed)
    if kind == "adam":
        cfg = dict(mode=0, lr=R.ADAM["lr"], b1=R.ADAM["b1"], b2=R.ADAM["b2"], eps=R.ADAM["eps"])
    else:
        cfg = dict(mode=1, lr=R.SGD_LR, b1=b1, b2=0.0, eps=0.0)
    cfg["wd"] = wd
    pt, opt = _torch_opt(kind, p, m, v, start, cfg["lr"], cfg["b1"], cfg["b2"], cfg["eps"], wd, torch.float32)
    worst = dict(p=0.0, g=0.0, m=0.0, v=0.0)
    for k, g in enumerate(gs):
        ss = R.sumsq(g)
        max_norm = R.clip_norm(clip, ss, gscale)
        cfg["step"] = start + k
        ref = R.opt_step(p, g, m, v, ss, max_norm, cfg["lr"], cfg["b1"], cfg["b2"], cfg["eps"], cfg["step"], wd, cfg["mode"], gscale)
        bound = R.opt_bounds(ref, (p, g, m, v), cfg)
        gc = (g * _coef32(ss, max_norm, gscale)).astype(F32)
        pt.grad = torch.from_numpy(gc.copy())
        opt.step()
        tp, tm, tv = _torch_state(kind, pt, opt, cfg["b1"])
        for key, got, want in (("p", tp, ref[0]), ("g", gc, ref[1]), ("m", tm, ref[2]), ("v", tv, ref[3])):
            if got is not None and bound[key] is not None:      # (SGD without momentum keeps no buffer in torch: nothing to compare)
                ratio = np.abs(got.astype(np.float64) - want) / bound[key]
                worst[key] = max(worst[key], float(ratio.max()))
        p, m = tp, (tm if tm is not None else ref[2].astype(F32))
        v = tv if tv is not None else v
    return worst


CASES = [(kind, b1, wd, clip, gs) for (kind, b1), wd, clip, gs in
         itertools.product([("adam", None), ("sgd", 0.0), ("sgd", MOMENTUM)], [0.0, WD], ["off", "clips", "loose"], [1.0, 0.25])]
_worst = dict(p=0.0, g=0.0, m=0.0, v=0.0)


@pytest.mark.parametrize("kind,b1,wd,clip,gscale", CASES)
def test_torch_optim_in_float32_stays_inside_the_gate_bounds(kind, b1, wd, clip, gscale):
    for n, start in ((N_MID, 1), (N_MID, 6), (3, 1)):
        w = float32_run(n, kind, b1, wd, clip, gscale, start=start)
        for k in w:
            _worst[k] = max(_worst[k], w[k])
        assert max(w.values()) <= 1.0, (n, w)


@pytest.mark.parametrize("kind,b1", [("adam", None), ("sgd", MOMENTUM)])
def test_torch_optim_in_float32_stays_inside_the_gate_bounds_at_the_largest_size(kind, b1):
    w = float32_run(2048 * 4096 + 4099, kind, b1, WD, "clips", 0.25)
    for k in w:
        _worst[k] = max(_worst[k], w[k])
    assert max(w.values()) <= 1.0, w


def test_float32_worst_ratios_are_reported():
    print("[headtail_gate] cpu_float32 " + " ".join(f"{k}={v:.4f}" for k, v in _worst.items()))
    assert max(_worst.values()) <= 1.0


# ---- the gathers against what the project already trusts -----------------------------------------------------------------------------
def test_gathers_match_the_cabi_emulator():
    from cabi_emulator import Emulator
    rng = np.random.default_rng(1)
    n, n_src = 4099, 1500
    params = torch.from_numpy(rng.standard_normal(n_src).astype(F32))
    # (the emulator's tables carry no negate bit: the plans it serves never negate)
    tab = torch.from_numpy((R.entries(2 * n, n_src, rng) & ~1).astype(np.int32))
    tab[tab < 0] = -1
    em = Emulator()
    out = torch.zeros(n, dtype=torch.bfloat16)
    em("sehip_pack_bf16", params.data_ptr(), tab.data_ptr(), n, out.data_ptr(), None)
    assert np.array_equal(out.view(torch.int16).numpy().view(np.uint16), R.pack_bf16(params.numpy(), tab.numpy()[:n]))
    out = torch.zeros(n)
    em("sehip_pack_f32", params.data_ptr(), tab.data_ptr(), n, out.data_ptr(), None)
    assert np.array_equal(out.numpy().view(np.uint32), R.pack_f32(params.numpy(), tab.numpy()).view(np.uint32))
    out = torch.zeros(n)
    em("sehip_unpack_grad1", params.data_ptr(), tab.data_ptr(), n, out.data_ptr(), None)
    assert np.array_equal(out.numpy().view(np.uint32), R.unpack1(params.numpy(), tab.numpy()[:n]).view(np.uint32))


def test_pack_runs_matches_the_element_table_on_the_demucs_plan():
    """the tables tests/test_host_plan_demucs.py::test_pack_run_descriptors_reproduce_the_index_table decodes"""
    from sehip import plan_demucs as P
    from test_host_plan_demucs import SMALL
    st = P.DemucsStatic(P.DemucsConfig(**SMALL))
    rng = np.random.default_rng(2)
    flat = R.params_with_specials(st.layout.n_params, rng)
    n = st.n_wpack_dev
    want = R.pack_bf16(flat, st.wtab[:n])
    got = R.pack_runs(flat, st.runs, st.side, st.pack_dst)
    assert got.size == n and np.array_equal(got, want)
    # a segment on its own, as the plan launches it: absolute run numbers
    a, b = st.n_wpack_head // 8, st.n_wpack_fwd // 8
    if b > a:
        seg = R.pack_runs(flat, st.runs[a:b], st.side, st.pack_dst[a:b])
        assert np.array_equal(seg[8 * a:8 * b], want[8 * a:8 * b])


def test_unpack_forms_agree():
    rng = np.random.default_rng(3)
    n, n_src = 1029, 700
    packed = rng.standard_normal(n_src).astype(F32)
    tab4 = R.rows4(n, n_src, rng)
    want = R.unpack(packed, tab4)
    assert (want[(tab4 < 0).all(1)] == 0).all() and (tab4 < 0).all(1).any()
    lst = np.flatnonzero(tab4[:, 1] >= 0)
    assert np.array_equal(R.unpack_list(packed, lst, tab4[lst], R.unpack1(packed, tab4[:, 0])).view(np.uint32), want.view(np.uint32))
    perm = rng.permutation(n)
    assert np.array_equal(R.unpack_perm(packed, tab4[perm], perm).view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("which", sorted(R.INTEGER_CASES))
def test_the_integer_gradient_sets_keep_their_conditions(which):
    n, boundary, seed = R.INTEGER_CASES[which]
    case = R.integer_case(n, boundary, seed)
    cond = R.integer_conditions(case)
    assert all(cond.values()), cond
    assert all(boundary % r == 0 for r in R.block_ranges(n))
    if which == "large":
        assert R.block_ranges(n)[:2] == (1280, 1024)
    # the sums are what the test is after: they differ from tensor to tensor
    g = R.unpack(case["packed"], case["tab4"])
    assert len(set(R.tensor_sums(g, case["offsets"]).tolist())) > 20
