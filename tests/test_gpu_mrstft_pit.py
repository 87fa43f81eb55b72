"""GPU: sehip.loss.pit_mrstft_loss / pit_mrstft_terms / PitMRSTFTLoss (the sehip_mrl_pair_* kernels of csrc/mrstft_loss.hip) against
tests/mrstft_pit_ref.py, the torch restatement on top of mrstft_ref, in float64.

Shapes (B, S, C, n): (2, 2, 1, 4000); (1, 3, 2, 1025), one sample above n_fft / 2 of the 2048 resolution, where every frame reflects;
(3, 6, 1, 1300), six speakers at 2048: the largest LDS image of the forward kernel; (2, 1, 1, 1200), the 1 x 1 matrix.  The frame counts
are odd and even.  Resolution sets: the default three together, and (64, 16, 64), (128, 128, 128), (2048, 240, 1200) alone; each with
wave_l1 0 and 1: 32 combinations.  Inputs: mrstft_pit_ref.planted -- coloured targets of different levels, every estimate one target
plus a little noise, so the answer is known.  On the float64 oracle the runner-up permutation is at least 2.4 best sums away from the
best one with every weighting used here while the float32 restatement's pair matrix moves by less than 1e-6, so the choice cannot flip
inside fp32 error; each case asserts that gap (>= 1.0) on the oracle before it is trusted.

Every gate is COMPUTED here and printed: 8 x the largest deviation, over these 32 combinations, of the restatement in float32 from the one
in float64 (the convention of tests/test_gpu_mrstft_loss.py): the pair terms, the pair matrix and the loss (relative) and the gradient per
row (relative L2) with mag_weight = 0, with sc_weight = 0 and of the full loss.  The permutation must be the oracle's exactly.

Bits: the pair terms are those of mrstft_terms on the slices (the workgroup sums and the order of the final sum are the same); equal
inputs give the identity, every matched sc exactly 0 and a finite gradient; equal estimates tie every permutation and give the identity;
two runs and a graph replay agree; pit_loss with an MRSTFTLoss module is PitMRSTFTLoss."""
import pytest
import torch

import mrstft_pit_ref as PR
import mrstft_ref as MR

pytestmark = pytest.mark.gpu

SHAPES = ((2, 2, 1, 4000), (1, 3, 2, 1025), (3, 6, 1, 1300), (2, 1, 1, 1200))
RESOLUTION_SETS = (MR.RESOLUTIONS, ((64, 16, 64),), ((128, 128, 128),), ((2048, 240, 1200),))
WAVE_L1 = (0.0, 1.0)
TAGS = tuple((name, name[2:], scw, magw) for name, scw, magw in PR.WEIGHTS)
_cache = {}


def res_id(r):
    return "default" if len(r) == 3 else "x".join(map(str, r[0]))


def planted(shape):
    if shape not in _cache:
        _cache[shape] = PR.planted(*shape)
    return _cache[shape]


def reference(shape, res, wave_l1):
    """the restatement in both dtypes, computed once per case and left unchanged"""
    key = ("ref", shape, res, wave_l1)
    if key not in _cache:
        enh, tgt, _ = planted(shape)
        _cache[key] = {dt: PR.all_grads(enh, tgt, res, wave_l1, dt) for dt in (torch.float64, torch.float32)}
    return _cache[key]


def all_cases():
    return [(shape, res, wl) for shape in SHAPES for res in RESOLUTION_SETS for wl in WAVE_L1]


def rel_max(a, b):
    a, b = a.double().cpu(), b.double()
    return float(((a - b).abs() / b.abs()).max())


def row_rel(g, want):
    """the largest per-row ||g - want|| / ||want|| over the B S C rows"""
    n = want.shape[-1]
    g, want = g.double().cpu().reshape(-1, n), want.double().reshape(-1, n)
    return float(((g - want).norm(dim=1) / want.norm(dim=1)).max())


def gates():
    """{name: (gate, worst deviation of the float32 restatement)}"""
    if "gates" not in _cache:
        worst = dict(terms=0.0, matrix=0.0, loss=0.0, g_sc=0.0, g_mag=0.0, g_full=0.0)
        for shape, res, wl in all_cases():
            ref = reference(shape, res, wl)
            r64, r32 = ref[torch.float64], ref[torch.float32]
            worst["terms"] = max(worst["terms"], rel_max(r32["terms"], r64["terms"]))
            for name, tag, _, _ in TAGS:
                assert r32["perm_" + tag] == r64["perm_" + tag]
                worst["matrix"] = max(worst["matrix"], rel_max(r32["matrix_" + tag], r64["matrix_" + tag]))
                worst["loss"] = max(worst["loss"], rel_max(r32["loss_" + tag], r64["loss_" + tag]))
                worst[name] = max(worst[name], row_rel(r32[name], r64[name]))
        _cache["gates"] = {k: (8 * v, v) for k, v in worst.items()}
    return _cache["gates"]


def device_run(enh, tgt, res, scw, magw, wl):
    from sehip import pit_mrstft_loss
    e = enh.cuda().requires_grad_(True)
    t = tgt.cuda().requires_grad_(True)
    loss, perm = pit_mrstft_loss(e, t, res, scw, magw, wl, return_comb=True)
    loss.backward()
    assert t.grad is None                                            # the target receives no gradient
    assert not perm.requires_grad and perm.dtype == torch.int32
    return loss.detach(), e.grad, perm


def test_gates_from_the_restatement():
    g = gates()
    for name, (gate, worst) in g.items():
        print(f"[mrstft-pit] float32 restatement, {name}: worst deviation {worst:.3e}, gate {gate:.3e}")
    gaps = [reference(*case)[torch.float64]["gap_" + tag] for case in all_cases() if case[0][1] > 1 for _, tag, _, _ in TAGS]
    devs = [float((reference(*case)[torch.float32]["matrix_" + tag].double() - reference(*case)[torch.float64]["matrix_" + tag]).abs().max())
            for case in all_cases() for _, tag, _, _ in TAGS]
    print(f"[mrstft-pit] oracle: relative gap of the runner-up permutation {min(gaps):.2f} .. {max(gaps):.2f}; "
          f"float32 pair matrix deviates by at most {max(devs):.2e}")
    assert all(gate > 0 for gate, _ in g.values())
    assert max(g["terms"][0], g["matrix"][0], g["loss"][0], g["g_sc"][0]) < 1e-4    # the sharp ones (mag-only is ill-conditioned)
    assert min(gaps) >= 1.0 and max(devs) < 1e-5


@pytest.mark.parametrize("res", RESOLUTION_SETS, ids=res_id)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_values_gradients_and_permutation(shape, res):
    from sehip import pit_mrstft_terms
    g = gates()
    enh, tgt, planted_perm = planted(shape)
    S = shape[1]
    worst = dict(terms=0.0, matrix=0.0, loss=0.0, g_sc=0.0, g_mag=0.0, g_full=0.0)
    for wl in WAVE_L1:
        want = reference(shape, res, wl)[torch.float64]
        for _, tag, _, _ in TAGS:                                    # the case is trusted only with a choice that cannot flip
            assert want["perm_" + tag] == planted_perm and want["gap_" + tag] >= 1.0, (tag, want["perm_" + tag], want["gap_" + tag])
        for name, tag, scw, magw in TAGS:
            terms, matrix, perm = pit_mrstft_terms(enh.cuda(), tgt.cuda(), res, scw, magw, wl)
            assert terms.shape == (len(res), S, S, 2) and matrix.shape == (S, S) and perm.shape == (S,)
            assert terms.dtype == matrix.dtype == torch.float32 and perm.dtype == torch.int32
            assert perm.tolist() == want["perm_" + tag]
            worst["terms"] = max(worst["terms"], rel_max(terms, want["terms"]))
            worst["matrix"] = max(worst["matrix"], rel_max(matrix, want["matrix_" + tag]))
            loss, grad, perm2 = device_run(enh, tgt, res, scw, magw, wl)
            assert loss.shape == () and loss.dtype == torch.float32 and grad.shape == shape and perm2.tolist() == want["perm_" + tag]
            assert bool(torch.isfinite(grad).all())
            worst["loss"] = max(worst["loss"], rel_max(loss, want["loss_" + tag]))
            worst[name] = max(worst[name], row_rel(grad, want[name]))
    print(f"[mrstft-pit] {shape} {res}: " + ", ".join(f"{k} {v:.3e} (gate {g[k][0]:.3e})" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= g[k][0], (k, v, g[k])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pair_terms_carry_the_bits_of_mrstft_terms(shape):
    """one transform per signal, but the sums of a pair are those of the plain kernels on (enhance[:, i], target[:, j]), bit for bit"""
    from sehip import mrstft_terms, pit_mrstft_terms
    enh, tgt, _ = planted(shape)
    e, t = enh.cuda(), tgt.cuda()
    for res in RESOLUTION_SETS:
        terms = pit_mrstft_terms(e, t, res)[0]
        for i in range(shape[1]):
            for j in range(shape[1]):
                want = mrstft_terms(e[:, i].contiguous(), t[:, j].contiguous(), res)
                assert torch.equal(terms[:, i, j], want), (res, i, j, terms[:, i, j], want)


@pytest.mark.parametrize("wl", WAVE_L1)
def test_equal_inputs_give_the_identity_and_an_exactly_zero_sc(wl):
    from sehip import pit_mrstft_terms
    for shape in ((1, 3, 2, 1025), (3, 6, 1, 1300)):
        tgt = planted(shape)[1]
        S = shape[1]
        terms, matrix, perm = pit_mrstft_terms(tgt.cuda(), tgt.cuda(), MR.RESOLUTIONS, 1.0, 1.0, wl)
        assert perm.tolist() == list(range(S))
        diag = terms[:, torch.arange(S), torch.arange(S)]
        assert not diag.any() and not matrix.diagonal().any()        # sc (and mag) of every matched pair exactly 0
        assert bool((matrix + torch.eye(S, device="cuda") > 0).all())
        loss, grad, perm = device_run(tgt, tgt, MR.RESOLUTIONS, 1.0, 1.0, wl)
        assert float(loss) == 0.0 and perm.tolist() == list(range(S)) and bool(torch.isfinite(grad).all())
        assert not device_run(tgt, tgt, MR.RESOLUTIONS, 1.0, 0.0, wl)[1].any()      # ||Y - X|| = 0: an exactly zero gradient, not a NaN


def test_equal_estimates_tie_every_permutation_and_give_the_identity():
    for shape in ((1, 3, 2, 1025), (3, 6, 1, 1300)):
        enh, tgt, _ = planted(shape)
        same = enh[:, :1].expand_as(enh).contiguous()
        for wl in WAVE_L1:
            loss, grad, perm = device_run(same, tgt, MR.RESOLUTIONS, 1.0, 1.0, wl)
            assert perm.tolist() == list(range(shape[1])) and bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all())


def test_two_runs_and_a_captured_replay_give_the_same_bits():
    from sehip import PitMRSTFTLoss
    shape = (3, 6, 1, 1300)
    ea, ta, pa = planted(shape)
    eb, tb = ea.flip(1).contiguous(), ta                             # the estimates the other way round: another permutation
    eager = [[device_run(e, t, MR.RESOLUTIONS, 1.0, 1.0, 1.0) for e, t in ((ea, ta), (eb, tb))] for _ in range(2)]
    for (l0, g0, p0), (l1, g1, p1) in zip(*eager):
        assert torch.equal(l0, l1) and torch.equal(g0, g1) and torch.equal(p0, p1)
    assert eager[0][0][2].tolist() == pa and eager[0][1][2].tolist() != pa
    mod = PitMRSTFTLoss(wave_l1=1.0)
    # eager warm-up on tensors of its own: a leaf that an eager forward has used stays bound to that forward's stream
    warm = ea.cuda().requires_grad_(True)
    torch.autograd.grad(mod(warm, ta.cuda()), warm)
    del warm
    torch.cuda.synchronize()
    e_s, t_s = ea.cuda().requires_grad_(True), ta.cuda()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss_s, perm_s = mod(e_s, t_s, return_comb=True)
        (grad_s,) = torch.autograd.grad(loss_s, e_s)
    for (e, t), (loss, grad, perm) in (((eb, tb), eager[0][1]), ((ea, ta), eager[0][0])):
        with torch.no_grad():
            e_s.copy_(e.cuda())
            t_s.copy_(t.cuda())
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(loss_s, loss) and torch.equal(grad_s, grad) and torch.equal(perm_s, perm)


def test_a_stale_backward_is_refused():
    from sehip import PitMRSTFTLoss, SehipError
    enh, tgt, _ = planted((2, 1, 1, 1200))
    mod = PitMRSTFTLoss(((128, 50, 100),))
    e = enh.cuda().requires_grad_(True)
    first = mod(e, tgt.cuda())
    second = mod(e, tgt.cuda())                                      # the same workspace: only the latest forward can be differentiated
    with pytest.raises(SehipError, match="another forward pass"):
        first.backward()
    second.backward()
    assert bool(torch.isfinite(e.grad).all()) and bool(e.grad.any())
    with pytest.raises(SehipError, match="pit_mrstft_loss.*n=1024"):
        PitMRSTFTLoss()(e[..., :1024], tgt.cuda()[..., :1024])      # 1024 samples: one too few for the 2048 resolution
    with pytest.raises(ValueError, match="pit_mrstft_loss"):
        mod(e, tgt.cuda()[..., :1000])
    with pytest.raises(SehipError, match="batch, speakers"):
        mod(e[0, 0], tgt.cuda()[0, 0])
    with pytest.raises(SehipError, match="S=7"):
        mod(torch.zeros(1, 7, 1, 1200, device="cuda"), torch.zeros(1, 7, 1, 1200, device="cuda"))


def test_pit_loss_with_an_mrstft_module_is_the_pit_module():
    from sehip import MRSTFTLoss, PitMRSTFTLoss, mrstft_loss, pit_mrstft_loss
    from sehip.loss import pit_loss
    enh, tgt, want_perm = planted((1, 3, 2, 1025))
    res = ((512, 128, 512), (256, 64, 200))
    e1 = enh.cuda().requires_grad_(True)
    plain = MRSTFTLoss(res, sc_weight=0.5, mag_weight=2.0, wave_l1=0.25)
    loss1, comb = pit_loss(e1, tgt.cuda(), plain, return_comb=True)
    (grad1,) = torch.autograd.grad(loss1, e1)
    e2 = enh.cuda().requires_grad_(True)
    loss2, perm = PitMRSTFTLoss(res, 0.5, 2.0, 0.25)(e2, tgt.cuda(), return_comb=True)
    (grad2,) = torch.autograd.grad(loss2, e2)
    assert torch.equal(loss1, loss2) and torch.equal(grad1, grad2)
    assert comb == [(i, j) for j, i in enumerate(perm.tolist())] and perm.tolist() == want_perm
    assert torch.equal(pit_loss(e1, tgt.cuda(), plain), loss1)      # again on the module's own workspace
    assert "_pit" not in dict(plain.named_modules())                 # the module itself is unchanged
    assert torch.equal(pit_loss(enh.cuda(), tgt.cuda(), mrstft_loss), pit_mrstft_loss(enh.cuda(), tgt.cuda()))
    # the matched pairs' plain losses, added up by hand, within the value gate
    by_hand = sum(plain(enh.cuda()[:, i].contiguous(), tgt.cuda()[:, j].contiguous()) for i, j in comb) / 3
    assert abs(float(by_hand.detach()) - float(loss1.detach())) <= gates()["loss"][0] * float(loss1.detach())


# ---- Solver --------------------------------------------------------------------------------------------------------------------------------
def solver_config(tmp, loss, use_graph):
    from sehip.utils import dict2obj
    return dict2obj({
        "seed": 10, "root": None, "ha": None,
        "model": {"name": "conv-tasnet", "audio_channels": 1, "num_spk": 2, "sources": ["None", "None"], "skip": False, "sample_rate": 8000,
                  "segment": 1, "causal": True, "norm_type": "cLN", "N": 32, "L": 8, "B": 32, "H": 96, "P": 3, "X": 3, "R": 2},
        "optim": {"optim": "adam", "lr": 3e-4, "beta1": 0.9, "beta2": 0.999, "loss": loss, "clip_grad": 5, "pit": False, "load": False},
        "dset": {"name": "synthetic", "sample_rate": 8000},
        "solver": {"epochs": 1, "save_checkpoint_interval": 1000, "all_steps": True, "total_steps": 0, "patience": 0, "use_graph": use_graph,
                   "root": str(tmp), "resume": None, "preloaded_model": None,
                   "validation": {"interval": 1000, "metric": "loss", "total_steps": 0}, "test": {"interval": 1000}},
    })


def test_solver_trains_on_pit_l1_mrstft_eager_and_graphed(tmp_path):
    """one train_step and one train_step_graphed of the small causal ConvTasNet (2 speakers, [2, 2, 1, 8000]) with optim.loss
    'pit-l1+mrstft' and no pit_apply, from the same initial state: every gradient is finite and not all are zero, the graphed step gives
    the eager loss bits, and the loss does not care which way round the targets' speakers are"""
    import copy
    from sehip import distrib
    from sehip.loss import PitMRSTFTLoss
    from sehip.solver import ScalarLog, Solver
    torch.manual_seed(0)
    state = copy.deepcopy(distrib.get_model(solver_config(tmp_path, "pit-l1+mrstft", False).model).state_dict())
    src = 0.1 * torch.randn(2, 2, 1, 8000, generator=torch.Generator().manual_seed(5))
    src[:, 1] *= 0.3                                                 # (two speakers that differ, so that the order matters to a plain loss)
    mix = src.sum(1)
    out = []
    for graphed in (False, True):
        cfg = solver_config(tmp_path, "pit-l1+mrstft", graphed)
        model = distrib.get_model(cfg.model)
        model.load_state_dict(state)
        loss_fn = distrib.get_loss_function(cfg.optim)
        assert isinstance(loss_fn, PitMRSTFTLoss) and loss_fn.wave_l1 == 1.0
        solver = Solver(copy.deepcopy(cfg), model, distrib.get_optimizer(cfg.optim, model), loss_fn, device="gpu", writer=ScalarLog())
        seen = {}
        loss_fn.register_forward_hook(lambda m, inp, res: seen.update(enhanced=inp[0].detach().clone(), sources=inp[1].detach().clone()))
        mx, sr = solver._prepare_batch(mix, src)
        loss, _ = (solver.train_step_graphed if graphed else solver.train_step)(mx, sr)
        torch.cuda.synchronize()
        grads = solver.model.flat_grads
        assert bool(torch.isfinite(grads).all()) and bool(grads.any())
        if not graphed:                                              # (the hook of the graphed step saw the capture's placeholders)
            assert seen["enhanced"].shape == seen["sources"].shape == (2, 2, 1, 8000)
            fresh = PitMRSTFTLoss(wave_l1=1.0)
            straight = fresh(seen["enhanced"], seen["sources"])
            swapped = fresh(seen["enhanced"], seen["sources"].flip(1).contiguous())
            assert torch.equal(loss, straight) and 0 < float(loss) < 100
            assert abs(float(swapped) - float(straight)) <= gates()["loss"][0] * float(straight)
        out.append(loss.clone())
    print(f"[mrstft-pit] solver: eager {float(out[0]):.9g} graphed {float(out[1]):.9g}")
    assert torch.equal(out[0], out[1])
