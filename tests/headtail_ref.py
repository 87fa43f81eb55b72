"""Plain numpy restatement of the head and the tail of every train step (csrc/pack.hip, csrc/optim.hip), written for this project from
the documented semantics of include/sehip.h, for tests/test_headtail_host.py (CPU) and tests/test_gpu_headtail.py (GPU).  The inputs
are the arrays the kernels get; nothing of the package is imported and no GPU is used.

A table entry e is (index << 1) | negate, -1 = absent.  The gathers only select, negate and add at most four fp32 terms in the fixed
order ((x + y) + z) + w, so they are restated in float32 in that order and compared BIT FOR BIT; the reductions and the optimizer
update are restated in float64.

    term(src, e)                                  the signed fp32 value of an entry (0.0 where absent)
    bf16_bits(x)                                  float32 -> bfloat16 (round to nearest even, torch's CPU conversion) as uint16
    pack_bf16(params, tab)                        uint16 [n]
    pack_f32(params, tab2)                        float32 [n] = term(x) + term(y)
    pack_runs(params, runs2, side, dst=None)      uint16 [8 * runs]: run.x >= 0 base with stride run.y, -1 eight zeros,
                                                  <= -2 the eight entries at side[8 * (-2 - run.x)]; entry i fills run dst[i]
    unpack(packed, tab4) / unpack1(packed, tab1)  float32 [n]
    unpack_list(packed, lst, tab4, grads)         grads with grads[lst[i]] = row i of tab4
    unpack_perm(packed, tab4, perm)               grads[perm[i]] = row i
    tensor_sums(g, offsets) / sumsq(g)            float64
    clip_coef(sumsq, max_norm, gscale)            gscale * min(1, max_norm / (sqrt(sumsq) * gscale + 1e-6)), gscale without clipping
    metric(g, offsets, coef=1.0)                  (sqrt(sum_t (sum g_t)^2) * coef, sqrt(sum g^2))
    opt_step(...)                                 one Adam (mode 0) / SGD-with-momentum (mode 1) step, the formulas of csrc/optim.hip's header

and the synthetic tables both test files share (tensor_sizes, layout_conditions, integer_case, value_list, ...)."""
import numpy as np
import torch

F32 = np.float32


# ---- gathers (float32, bit-exact) ---------------------------------------------------------------------------------------------------
def term(src, e):
    e = np.asarray(e, dtype=np.int64)
    v = np.asarray(src, dtype=F32)[np.maximum(e, 0) >> 1]
    v = np.where((e & 1) == 1, -v, v)                        # the negation flips the sign bit: -0.0, -inf and NaN included
    return np.where(e < 0, F32(0), v).astype(F32)


def bf16_bits(x):
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=F32)).to(torch.bfloat16)
    return t.view(torch.int16).numpy().view(np.uint16).copy()


def bf16_mismatch(got, want):
    """indices where two uint16 bf16 arrays differ; a NaN matches any NaN (its payload and sign are the converter's business)"""
    got, want = np.asarray(got, dtype=np.uint16), np.asarray(want, dtype=np.uint16)
    nan = lambda u: ((u & 0x7F80) == 0x7F80) & ((u & 0x007F) != 0)
    return np.flatnonzero((got != want) & ~(nan(got) & nan(want)))


def f32_mismatch(got, want):
    """the same for float32 arrays compared bit for bit"""
    got, want = np.asarray(got, dtype=F32), np.asarray(want, dtype=F32)
    return np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want)))


def pack_bf16(params, tab):
    return bf16_bits(term(params, np.asarray(tab).reshape(-1)))


def pack_f32(params, tab2):
    t = np.asarray(tab2).reshape(-1, 2)
    return (term(params, t[:, 0]) + term(params, t[:, 1])).astype(F32)


def pack_runs(params, runs2, side, dst=None):
    runs = np.asarray(runs2, dtype=np.int64).reshape(-1, 2)
    side = np.asarray(side, dtype=np.int64).reshape(-1, 8)
    params = np.asarray(params, dtype=F32)
    vals = np.zeros((runs.shape[0], 8), dtype=F32)
    aff = runs[:, 0] >= 0
    vals[aff] = params[runs[aff, :1] + np.arange(8, dtype=np.int64)[None] * runs[aff, 1:]]
    irr = runs[:, 0] <= -2
    vals[irr] = term(params, side[-2 - runs[irr, 0]])
    where = np.arange(runs.shape[0]) if dst is None else np.asarray(dst, dtype=np.int64)
    out = np.zeros((int(where.max()) + 1, 8), dtype=F32)
    out[where] = vals
    return bf16_bits(out.reshape(-1))


def unpack(packed, tab4):
    t = np.asarray(tab4).reshape(-1, 4)
    return (((term(packed, t[:, 0]) + term(packed, t[:, 1])) + term(packed, t[:, 2])) + term(packed, t[:, 3])).astype(F32)


def unpack1(packed, tab1):
    return term(packed, np.asarray(tab1).reshape(-1))


def unpack_list(packed, lst, tab4, grads):
    out = np.array(grads, dtype=F32, copy=True)
    out[np.asarray(lst, dtype=np.int64)] = unpack(packed, tab4)
    return out


def unpack_perm(packed, tab4, perm):
    rows = unpack(packed, tab4)
    out = np.zeros_like(rows)
    out[np.asarray(perm, dtype=np.int64)] = rows
    return out


# ---- reductions and the update (float64) --------------------------------------------------------------------------------------------
def tensor_sums(g, offsets):
    g = np.asarray(g, dtype=np.float64)
    return np.array([g[offsets[t]:offsets[t + 1]].sum() for t in range(len(offsets) - 1)], dtype=np.float64)


def sumsq(g):
    g = np.asarray(g, dtype=np.float64)
    return float((g * g).sum())


def clip_coef(sumsq_, max_norm, gscale=1.0):
    if max_norm > 0:
        return gscale * min(1.0, max_norm / (np.sqrt(float(sumsq_)) * gscale + 1e-6))
    return float(gscale)


def metric(g, offsets, coef=1.0):
    return float(np.sqrt((tensor_sums(g, offsets) ** 2).sum()) * coef), float(np.sqrt(sumsq(g)))


def opt_step(p, g, m, v, sumsq_, max_norm, lr, b1, b2, eps, step, wd, mode, gscale=1.0):
    """-> (p, g, m, v, dp) in float64.  g comes back scaled by coef WITHOUT the weight-decay term, as the kernel writes it back.
    mode 0: torch.optim.Adam (amsgrad False, L2 weight decay); mode 1: torch.optim.SGD (b1 = momentum, dampening 0, nesterov False),
    m = the momentum buffer, which is g on step 1, and the value the kernel stores (g) without momentum; v is untouched."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    gc = g * clip_coef(sumsq_, max_norm, gscale)
    gi = gc + wd * p if wd != 0 else gc
    if mode == 0:
        m = m * b1 + (1.0 - b1) * gi
        v = v * b2 + (1.0 - b2) * gi * gi
        dp = -(lr / (1.0 - b1 ** step)) * (m / (np.sqrt(v) / np.sqrt(1.0 - b2 ** step) + eps))
    else:
        m = gi.copy() if step == 1 else m * b1 + gi
        dp = -lr * (m if b1 != 0 else gi)
    return p + dp, gc, m, v, dp


# ---- synthetic inputs shared by the host and the GPU file ----------------------------------------------------------------------------
def value_list():
    """The values a conversion can get wrong: signed zeros, infinities, NaN, bf16 ties (to an even and to an odd mantissa), the two
    neighbours of the bf16 overflow threshold, float32 subnormals."""
    bits = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000,
                     0x3F808000, 0xBF808000,            # 1 + 2^-8: tie, the even neighbour is below
                     0x3F818000, 0xBF818000,            # 1 + 3 * 2^-8: tie, the even neighbour is above
                     0x3F808001, 0x3F807FFF,            # just off a tie on either side
                     0x7F7F7FFF, 0x7F7F8000, 0x7F7F8001,   # the largest value that stays finite in bf16, the tie that rounds to inf, the next
                     0xFF7F7FFF, 0xFF7F8000,
                     0x00000001, 0x80000001, 0x007FFFFF, 0x00008000, 0x00018000, 0x807F8000], dtype=np.uint32)
    return bits.view(F32).copy()


def is_subnormal(x):
    x = np.asarray(x, dtype=F32)
    return (x != 0) & (np.abs(x) < F32(2.0 ** -126))


def params_with_specials(n, rng):
    """n Gaussian parameters whose first len(value_list()) entries are the special values"""
    p = rng.standard_normal(n).astype(F32)
    s = value_list()
    assert n >= s.size
    p[:s.size] = s
    return p


def entries(n, n_src, rng, p_absent=0.1, specials=0):
    """n table entries over n_src sources: a tenth absent, half negated; entry 1 (index 0, negated) and a much-used source are there;
    the first `specials` sources appear with both signs"""
    idx = rng.integers(0, n_src, n)
    idx[rng.random(n) < 0.05] = n_src // 2                    # one parameter referenced many times
    e = (idx << 1) | rng.integers(0, 2, n)
    e[rng.random(n) < p_absent] = -1
    fixed = [1, 0, -1] + [2 * i + s for i in range(specials) for s in (0, 1)]
    m = min(n, len(fixed))
    at = rng.permutation(n)[:m]
    e[at] = fixed[:m]
    return e.astype(np.int32)


def rows4(n, n_src, rng):
    """[n, 4] un-pack rows with 1..4 terms in the leading columns; one row in sixteen has none"""
    t = entries(4 * n, n_src, rng, p_absent=0.0).reshape(n, 4)
    t[t < 0] = 2                                               # (the absent entry entries() always plants)
    k = rng.integers(1, 5, n)
    k[rng.random(n) < 1 / 16] = 0
    t[np.arange(4)[None] >= k[:, None]] = -1
    return np.ascontiguousarray(t)


def run_table(n8, n_params, rng):
    """(runs [n8, 2], side [8 * irregular]): affine runs with strides 1, 8, 24, 513, zero runs and irregular runs"""
    runs = np.zeros((n8, 2), dtype=np.int32)
    kind = rng.integers(0, 8, n8)
    kind[:7] = [0, 6, 7, 0, 0, 0, 0][:n8]                     # every kind appears wherever there are three runs
    stride = np.array([1, 8, 24, 513])[rng.integers(0, 4, n8)]
    stride[:1] = 513
    assert n_params > 7 * 513
    runs[:, 0] = rng.integers(0, n_params - 7 * stride)       # base + 7 * stride stays inside the parameters
    runs[:, 1] = stride
    if n8 >= 7:
        runs[3] = (n_params - 1 - 7 * 513, 513)               # the last parameter is read
        runs[4:7] = [(0, 1), (8, 1), (14, 1)]                 # the special values at the head of the parameters through affine runs
    runs[kind == 6] = (-1, 0)
    irr = np.flatnonzero(kind == 7)
    runs[irr, 0] = -2 - np.arange(irr.size)
    runs[irr, 1] = 0
    side = entries(8 * max(irr.size, 1), n_params, rng, specials=len(value_list()))
    return runs, side


SMALL_RUN = 44             # consecutive tensors of 1..5 elements
NAMED_SIZES = [1, 3, 63, 64, 65, 255, 256, 257, 1023, 1025]


def tensor_sizes(n, boundary):
    """Tensor sizes that add up to n: the named sizes, a filler that ENDS exactly at `boundary` (a multiple of every kernel's block
    range at this n), a one-element tensor there, so that the next one starts one past it, a run of tiny tensors, one tensor of more than half of
    everything, and a 2, 7, 6 tail."""
    head = NAMED_SIZES[:8]
    sizes = head + [boundary - sum(head), 1] + NAMED_SIZES[8:] + [1 + i % 5 for i in range(SMALL_RUN)]
    tail = [2, 7, 6]
    big = n - sum(sizes) - sum(tail)
    sizes += [big] + tail
    assert big > n // 2 and sum(sizes) == n
    return sizes


def layout_conditions(sizes, boundary):
    """The conditions the size list is built for, as a dict of booleans (every one must be True)"""
    s = np.asarray(sizes)
    off = np.concatenate([[0], np.cumsum(s)])
    small = s <= 5
    run = best = 0
    for x in small:
        run = run + 1 if x else 0
        best = max(best, run)
    return dict(named=all(x in s for x in NAMED_SIZES), small_run=best >= 40, big=bool(s.max() > off[-1] // 2),
                odd_offset=bool((off[:-1] % 2 == 1).any()), offset_2_mod_4=bool((off[:-1] % 4 == 2).any()),
                ends_on_boundary=bool((off[1:] == boundary).any()), starts_one_after=bool((off[:-1] == boundary + 1).any()))


def block_ranges(n):
    """The contiguous range a workgroup owns in unpack_grad_sums_kernel (1024 workgroups, multiples of 256), unpack_grad1_sums_kernel
    (2048, multiples of 1024) and tensor_sums_flat_kernel (1024, multiples of 1024)"""
    up = lambda a, b: (a + b - 1) // b
    return up(up(n, 1024), 256) * 256, up(up(n, 2048), 1024) * 1024, up(up(n, 1024), 1024) * 1024


def integer_case(n, boundary, seed):
    """A packed buffer of small non-zero integers and tables whose gradients are non-zero integers with sum |g| < 2^24 and
    sum g^2 < 2^24 over the whole buffer: every fp32 partial sum of g and of g^2 is then an integer below 2^24, exact in ANY order,
    atomics included, so the device sums must EQUAL the float64 ones.  -> dict(packed, tab4, tab1, lst, tab4l, perm, tab4p, offsets)
    tab1 / lst / tab4l: the one-entry form (first entry per parameter + the rows with several entries, by index)."""
    rng = np.random.default_rng(seed)
    sizes = tensor_sizes(n, boundary)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n_src = n + 1000
    packed = (rng.choice([1, 1, 1, 2, 2, 3], n_src) * rng.choice([-1, 1], n_src)).astype(F32)
    tab4 = entries(4 * n, n_src, rng, p_absent=0.0).reshape(n, 4)
    tab4[tab4 < 0] = 2                                                         # (the absent entry entries() always plants)
    k = np.where(rng.random(n) < 0.75, 1, rng.integers(2, 5, n))            # mostly one entry per parameter
    k[offsets[:-1]] = 4                                                        # the first and the last element of every tensor have four
    k[offsets[1:] - 1] = 4
    tab4[np.arange(4)[None] >= k[:, None]] = -1
    zero = unpack(packed, tab4) == 0                                           # a cancelled sum: keep the first entry only
    tab4[zero, 1:] = -1
    tab4 = np.ascontiguousarray(tab4)
    lst = np.flatnonzero(tab4[:, 1] >= 0).astype(np.int32)
    perm = np.concatenate([offsets[t] + rng.permutation(sizes[t]) for t in range(len(sizes))]).astype(np.int32)
    return dict(packed=packed, tab4=tab4, tab1=np.ascontiguousarray(tab4[:, 0]), lst=lst, tab4l=np.ascontiguousarray(tab4[lst]),
                perm=perm, tab4p=np.ascontiguousarray(tab4[perm]), offsets=offsets, sizes=sizes, boundary=boundary)


def integer_conditions(case):
    g = unpack(case["packed"], case["tab4"]).astype(np.float64)
    return dict(integers=bool((g == np.round(g)).all()), nonzero=bool((g != 0).all()), sum_abs=bool(np.abs(g).sum() < 2 ** 24),
                sum_sq=bool((g * g).sum() < 2 ** 24), first_entries_nonzero=bool((unpack1(case["packed"], case["tab1"]) != 0).all()),
                perm_within_tensors=all(np.array_equal(np.sort(case["perm"][a:b]), np.arange(a, b))
                                        for a, b in zip(case["offsets"][:-1], case["offsets"][1:])),
                **layout_conditions(case["sizes"], case["boundary"]))


# n, boundary, seed.  The small one cannot be smaller: the named sizes, the filler and the tiny tensors are 3218 elements, and one
# tensor has to be more than half of everything
INTEGER_CASES = {"small": (6501, 1024, 21), "large": (1100003, 10240, 22)}


# the optimizer gate's inputs: Adam's betas, the learning rate and eps are exact in float32, so the float64 reference, a float32
# implementation and the kernel (which gets them as C floats) all compute with the same numbers; the weight decay 1e-2 and the momentum
# 0.9 of the issue are rounded to float32 BEFORE anybody uses them (hyper() does it)
ADAM = dict(lr=2.0 ** -8, b1=0.875, b2=1.0 - 2.0 ** -9, eps=2.0 ** -27)
SGD_LR = 2.0 ** -6


def hyper(x):
    return float(F32(x))


def clip_norm(clip, sumsq_, gscale):
    """max_norm of a step: "off" none, "clips" half the norm of the scaled gradient, "loose" four times it (armed, never bites)"""
    return {"off": 0.0, "clips": hyper(0.5 * np.sqrt(sumsq_) * gscale), "loose": hyper(4.0 * np.sqrt(sumsq_) * gscale)}[clip]


def opt_inputs(n, seed, steps=3):
    """p, m, v and `steps` gradients (float32).  The bounds of the optimizer gate are relative to |dp| and to the magnitudes of the
    two terms m and v are built from, so a correct fp32 implementation can only meet them where those terms do not cancel: p, m
    and every gradient of an element share ONE random sign (with weight decay g + wd p keeps it), magnitudes stay within [0.5, 1.5]
    of their scale.  The signs differ from element to element."""
    rng = np.random.default_rng(seed)
    s = rng.choice([-1.0, 1.0], n)
    mag = lambda scale: (scale * (0.5 + rng.random(n)))
    p = (s * mag(1.0)).astype(F32)
    m = (s * mag(3e-2)).astype(F32)
    v = mag(1e-3).astype(F32)
    gs = [(s * mag(3e-2)).astype(F32) for _ in range(steps)]
    return p, m, v, gs


def opt_bounds(ref_new, ref_old, cfg):
    """The per-element bounds of the optimizer gate from the float64 reference: ref_new = opt_step(...), ref_old = (p, g, m, v) it
    started from.  -> dict(p, g, m, v) of float64 arrays (v: None in SGD mode, where v is untouched)"""
    p1, g1, m1, v1, dp = ref_new
    p0, _, m0, v0 = (np.asarray(a, dtype=np.float64) for a in ref_old)
    gi = g1 + cfg["wd"] * p0 if cfg["wd"] != 0 else g1
    if cfg["mode"] == 0:
        mt = np.abs(m0 * cfg["b1"]) + np.abs((1.0 - cfg["b1"]) * gi)
        vt = np.abs(v0 * cfg["b2"]) + np.abs((1.0 - cfg["b2"]) * gi * gi)
    else:
        mt = np.abs(gi) if cfg["step"] == 1 else np.abs(m0 * cfg["b1"]) + np.abs(gi)
        vt = None
    return dict(p=2.0 ** -23 * np.abs(p1) + 2.0 ** -20 * np.abs(dp), g=2.0 ** -22 * np.abs(g1), m=2.0 ** -21 * mt,
                v=None if vt is None else 2.0 ** -21 * vt)
