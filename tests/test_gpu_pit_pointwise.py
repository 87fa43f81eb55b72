"""GPU: the fused permutation-invariant l1 / mse (sehip.loss.pit_loss_pointwise, csrc/loss.hip sehip_pit_pointwise_*) against
oracle/pit_oracle.py in float64 on the CPU with torch.nn.functional.l1_loss / mse_loss (that oracle is pinned to the reference by
tests/test_pit.py).  Tolerances are those of tests/test_pit.py: loss within 2e-4 relative, d loss / d enhance rel_err < 2e-4, the
permutation identical.  Speakers are drawn at different levels and every case asserts that the best and the second-best permutation
differ in float64 by more than 1e-3 relative, so a tie never decides the permutation.

Shapes (B, S, C, n), each for both modes: the smallest input; odd n (rows not 16-byte aligned: the scalar variant and its tail);
more than one block per row; PIT_MAXS speakers (720 permutations, the full register load); and the targets in swapped order."""
import functools
from itertools import permutations

import numpy as np
import pytest
import torch

from util import rel_err

pytestmark = pytest.mark.gpu

SHAPES = ((1, 2, 1, 1), (3, 2, 2, 1003), (2, 3, 1, 4096 + 5), (2, 6, 1, 257), (2, 2, 1, 8000))
MODES = ("l1", "mse")
SEED = 7


def _fn64(mode):
    return torch.nn.functional.l1_loss if mode == "l1" else torch.nn.functional.mse_loss


def _hip_fn(mode):
    from sehip import loss as L
    return L.l1_loss if mode == "l1" else L.mse_loss


def make_inputs(shape, seed=SEED, assign=None, zeros=False):
    """fp32 (est, tgt, assign): target speaker s at level 0.6^s, estimated speaker i = target assign[i] + 20 % noise.  With zeros
    every 5th sample of each estimated speaker EQUALS its target's sample (l1's gradient is 0 there)."""
    b, s, c, n = shape
    g = torch.Generator().manual_seed(seed)
    levels = torch.tensor([0.6 ** k for k in range(s)]).view(1, s, 1, 1)
    tgt = 0.1 * torch.randn(b, s, c, n, generator=g) * levels
    if assign is None:
        assign = [(k + 1) % s for k in range(s)]          # a rotation: never the identity
    est = tgt[:, assign] + 0.2 * 0.1 * levels[:, assign] * torch.randn(b, s, c, n, generator=g)
    if zeros:
        est[..., ::5] = tgt[:, assign][..., ::5]
    return est.contiguous(), tgt.contiguous(), assign


def oracle64(est, tgt, mode):
    """(loss, perm [S] with perm[j] = estimated speaker of target j, pairs, gradient) in float64, and the margin assertion."""
    from oracle import pit_oracle
    fn = _fn64(mode)
    e = est.double().requires_grad_(True)
    t = tgt.double()
    s = e.shape[1]
    with torch.no_grad():
        m = np.array([[float(fn(e[:, i], t[:, j])) for j in range(s)] for i in range(s)])
    perms = np.array(list(permutations(range(s))))
    sums = np.sort(m[perms, np.arange(s)].sum(1))
    if len(sums) > 1:
        assert sums[1] - sums[0] > 1e-3 * abs(sums[0]), f"input condition: best {sums[0]!r} second {sums[1]!r}"
    loss, comb, _ = pit_oracle.pit(e, t, fn)
    loss.backward()
    perm = [i for i, _ in sorted(comb, key=lambda p: p[1])]
    return float(loss.detach()), perm, [tuple(p) for p in comb], e.grad.clone()


@functools.lru_cache(maxsize=None)
def case(shape, mode, zeros=False):
    est, tgt, assign = make_inputs(shape, zeros=zeros)
    return est, tgt, assign, oracle64(est, tgt, mode)


def run_hip(est, tgt, mode):
    from sehip import loss as L
    dev = torch.device("cuda:0")
    e = est.to(dev).requires_grad_(True)
    loss, perm = L.pit_loss_pointwise(e, tgt.to(dev), mode, return_comb=True)
    loss.backward()
    return loss.detach(), perm, e.grad


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_matches_float64_oracle(shape, mode):
    est, tgt, assign, (want, want_perm, _, want_grad) = case(shape, mode)
    inv = [assign.index(j) for j in range(shape[1])]
    assert want_perm == inv                                # the generator's assignment is what the oracle finds
    loss, perm, grad = run_hip(est, tgt, mode)
    print(f"pit {mode} {shape}: loss hip {float(loss):.9g} oracle {want:.9g} rel {abs(float(loss) - want) / abs(want):.2e} | "
          f"perm {perm.tolist()} | grad rel_err {rel_err(grad.cpu(), want_grad):.2e}")
    assert perm.dtype == torch.int32 and perm.is_cuda and perm.tolist() == want_perm
    assert abs(float(loss) - want) < 2e-4 * abs(want)
    assert grad.shape == est.shape and rel_err(grad.cpu(), want_grad) < 2e-4


@pytest.mark.parametrize("mode", MODES)
def test_swapped_targets(mode):
    """Targets in swapped order: perm == [1, 0], and the loss is the un-swapped loss."""
    shape = (2, 2, 1, 8000)
    est, tgt, assign, (want, want_perm, _, _) = case(shape, mode)
    assert assign == [1, 0] and want_perm == [1, 0]
    loss_sw, perm_sw, grad_sw = run_hip(est, tgt, mode)
    loss_id, perm_id, grad_id = run_hip(est, tgt.flip(1).contiguous(), mode)
    print(f"pit {mode} swapped {float(loss_sw):.9g} un-swapped {float(loss_id):.9g}")
    assert perm_sw.tolist() == [1, 0] and perm_id.tolist() == [0, 1]
    assert abs(float(loss_sw) - float(loss_id)) < 2e-4 * abs(want) and abs(float(loss_sw) - want) < 2e-4 * abs(want)
    assert rel_err(grad_sw, grad_id) < 2e-4                # est is the same tensor: the same gradient reaches the same speakers


def test_l1_gradient_at_exact_zeros():
    shape = (3, 2, 2, 1003)
    est, tgt, assign, (want, want_perm, _, want_grad) = case(shape, "l1", True)
    hit = est == tgt[:, assign]
    assert int(hit.sum()) >= est.numel() // 5 and bool((want_grad[hit] == 0).all())
    loss, perm, grad = run_hip(est, tgt, "l1")
    g = grad.cpu()
    assert perm.tolist() == want_perm and abs(float(loss) - want) < 2e-4 * abs(want)
    assert bool(torch.isfinite(g).all()) and bool((g[hit] == 0).all()) and bool((g[~hit] != 0).all())
    assert rel_err(g, want_grad) < 2e-4


def test_return_comb_forms():
    from sehip import loss as L
    dev = torch.device("cuda:0")
    est, tgt, _, (want, want_perm, want_pairs, _) = case((2, 3, 1, 4096 + 5), "l1")
    loss, comb = L.pit_loss(est.to(dev), tgt.to(dev), L.l1_loss, return_comb=True)
    assert isinstance(comb, list) and [tuple(p) for p in comb] == want_pairs
    assert abs(float(loss) - want) < 2e-4 * abs(want)
    loss2, perm = L.pit_loss_pointwise(est.to(dev), tgt.to(dev), "l1", return_comb=True)
    assert torch.is_tensor(perm) and perm.is_cuda and perm.dtype == torch.int32 and perm.tolist() == want_perm
    assert torch.equal(loss, loss2)
    assert torch.is_tensor(L.pit_loss(est.to(dev), tgt.to(dev), L.l1_loss)) and L.pit_loss(est.to(dev), tgt.to(dev), L.l1_loss).dim() == 0


def test_seven_speakers_keep_the_host_path():
    from sehip import loss as L
    dev = torch.device("cuda:0")
    est, tgt, assign = make_inputs((2, 7, 1, 64))
    want, want_perm, want_pairs, want_grad = oracle64(est, tgt, "l1")
    e = est.to(dev).requires_grad_(True)
    loss, comb = L.pit_loss(e, tgt.to(dev), L.l1_loss, return_comb=True)
    loss.backward()
    assert [tuple(p) for p in comb] == want_pairs
    assert abs(float(loss.detach()) - want) < 2e-4 * abs(want) and rel_err(e.grad.cpu(), want_grad) < 2e-4


@pytest.mark.parametrize("mode", MODES)
def test_run_to_run_and_deterministic_switch(mode):
    from sehip import utils
    from sehip._lib import lib
    est, tgt, _, _ = case((2, 3, 1, 4096 + 5), mode)
    a = run_hip(est, tgt, mode)
    b = run_hip(est, tgt, mode)
    was = lib().sehip_get_deterministic()
    try:
        utils.set_deterministic(True)
        c = run_hip(est, tgt, mode)
    finally:
        utils.set_deterministic(bool(was))
    for other in (b, c):
        assert torch.equal(a[0], other[0]) and torch.equal(a[1], other[1]) and torch.equal(a[2], other[2])


def test_capture_replays_with_a_new_permutation():
    """Forward and backward of pit_loss(est, tgt, mse_loss) recorded into ONE graph on static tensors, replayed with new contents whose
    speakers are swapped relative to the recorded ones: no host synchronisation on the path, and perm is read on the device at
    replay, not baked in at capture."""
    import sehip.loss as L
    assert hasattr(L, "pit_loss_pointwise")
    dev = torch.device("cuda:0")
    shape = (2, 2, 1, 8000)
    est0, tgt0, _ = make_inputs(shape, seed=11, assign=[0, 1])
    est1, tgt1, _ = make_inputs(shape, seed=12, assign=[1, 0])
    # Eager warm-up (code objects loaded, the workspace cached) on tensors of its OWN, dropped before the capture: a leaf that an
    # eager forward has used keeps a gradient sink bound to the stream of that forward for as long as that graph lives, and a
    # recorded backward would then hand its gradient over to that stream -- the legacy default stream, which no capture may touch.
    est_w = est0.to(dev).requires_grad_(True)
    warm = L.pit_loss(est_w, tgt0.to(dev), L.mse_loss)
    torch.autograd.grad(warm, est_w)
    del warm, est_w
    torch.cuda.synchronize()
    est_s = est0.to(dev).requires_grad_(True)              # first used inside the capture
    tgt_s = tgt0.to(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss_s = L.pit_loss(est_s, tgt_s, L.mse_loss)
        (grad_s,) = torch.autograd.grad(loss_s, est_s)
    for est, tgt, want_perm in ((est1, tgt1, [1, 0]), (est0, tgt0, [0, 1])):
        with torch.no_grad():
            est_s.copy_(est.to(dev))
            tgt_s.copy_(tgt.to(dev))
        graph.replay()
        torch.cuda.synchronize()
        e = est.to(dev).requires_grad_(True)
        loss, perm = L.pit_loss_pointwise(e, tgt.to(dev), "mse", return_comb=True)
        loss.backward()
        want = oracle64(est, tgt, "mse")
        assert perm.tolist() == want_perm == want[1]
        print(f"capture replay perm {want_perm}: loss graph {float(loss_s):.9g} eager {float(loss):.9g} oracle {want[0]:.9g}")
        assert abs(float(loss_s) - float(loss)) < 2e-4 * abs(float(loss)) and abs(float(loss_s) - want[0]) < 2e-4 * abs(want[0])
        assert rel_err(grad_s, e.grad) < 2e-4 and rel_err(grad_s.cpu(), want[3]) < 2e-4


@pytest.mark.parametrize("loss_name", ("mse", "si-sdr"))
def test_solver_graphed_step_honours_pit_apply(loss_name):
    """Tiny ConvTasNet Solver (the C4 configuration of tests/test_gpu_convtasnet.py, B = 2, n = 8000) with optim.pit_apply: one
    train_step and one train_step_graphed from the same initial state and batch give the same loss, and the graphed loss does not
    move when the targets' speakers are swapped (it did before the captured step called the PIT loss)."""
    import copy
    import tempfile
    from sehip import distrib
    from sehip.solver import Solver
    from test_gpu_convtasnet import c4_config
    cfg = c4_config(tempfile.mkdtemp(prefix="sehip_pitpw_"))
    cfg.optim.loss = loss_name
    cfg.optim.pit_apply = True
    torch.manual_seed(0)
    state = copy.deepcopy(distrib.get_model(cfg.model).state_dict())
    g = torch.Generator().manual_seed(1)
    B, N = 2, 8000
    src = 0.1 * torch.randn(B, 2, 1, N, generator=g)
    src[:, 1] *= 0.3                      # speakers of different level: the two orders give different plain losses
    mix = src.sum(1)

    def step(graphed, swap):
        c = copy.deepcopy(cfg)
        m = distrib.get_model(c.model)
        m.load_state_dict(state)
        s = Solver(c, m, distrib.get_optimizer(c.optim, m), distrib.get_loss_function(c.optim), device="gpu")
        mx, sr = s._prepare_batch(mix, src.flip(1) if swap else src)
        loss, _ = (s.train_step_graphed if graphed else s.train_step)(mx, sr)
        return float(loss)
    eager, graphed, graphed_sw = step(False, False), step(True, False), step(True, True)
    print(f"solver pit_apply {loss_name}: eager {eager:.9g} graphed {graphed:.9g} graphed, targets swapped {graphed_sw:.9g}")
    assert abs(eager - graphed) < 2e-4 * abs(eager)
    assert abs(graphed_sw - graphed) < 1e-4 * abs(graphed)
