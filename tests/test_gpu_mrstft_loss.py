"""GPU: sehip.loss.mrstft_loss / mrstft_terms / MRSTFTLoss and sehip.ops.stft_magnitudes (csrc/mrstft_loss.hip) against
tests/mrstft_ref.py, the torch restatement with torch.stft and autograd, in float64.

Every gate is COMPUTED here and printed: 8 x the largest deviation, over this file's cases, of the restatement in float32 from the one in
float64 (one restatement is one sample of fp32 rounding; 8 is the factor of the STOI loss's gate).  Five gates: the magnitudes (worst cell
over its row's largest), the loss and each (sc, mag) term (relative), and the gradient per row (relative L2) with mag_weight = 0, with
sc_weight = 0 and of the full loss.  The sc-only gate is the sharp one for the transforms and their adjoints; the mag-only restatement
is ill-conditioned next to the clamp (1 / X at X ~ 3e-4).  Measured on an MI355X: DESIGN.md section 21.

Shapes: (3, 4000); (2, 1025), the shortest legal input of the 2048 resolution, where every frame reflects; (1, 1200), a multiple of all
three default hops; (4, 1300).  Resolutions: the default three together, and five single ones that take every transform size from 64 to
512, a window shorter than n_fft, hop = win_length and a hop that divides nothing.  Inputs: noise; enhanced = sources x 0.5 / 2
alternating by row; both signals with the second half exact zeros; enhanced == sources."""
import pytest
import torch

import mrstft_ref as MR

pytestmark = pytest.mark.gpu

SHAPES = ((3, 4000), (2, 1025), (1, 1200), (4, 1300))
SINGLES = ((512, 128, 512), (256, 64, 200), (64, 16, 64), (128, 50, 100), (128, 128, 128))
RESOLUTION_SETS = (MR.RESOLUTIONS,) + tuple((r,) for r in SINGLES)
KINDS = ("noise", "scaled", "halfzero", "equal")
GRADS = (("g_sc", 1.0, 0.0), ("g_mag", 0.0, 1.0), ("g_full", 1.0, 1.0))
_cache = {}


def pair(rows, n, kind):
    """(enhanced, sources) float32 on the host"""
    key = (rows, n, kind)
    if key not in _cache:
        g = torch.Generator().manual_seed(1000 * rows + n)
        src = 0.1 * torch.randn(rows, n, generator=g)
        enh = src + 0.05 * torch.randn(rows, n, generator=g)
        if kind == "scaled":
            enh = src * torch.tensor([0.5, 2.0]).repeat(rows)[:rows, None]
        elif kind == "halfzero":
            src[:, n // 2:] = 0.0
            enh[:, n // 2:] = 0.0
        elif kind == "equal":
            enh = src.clone()
        _cache[key] = (enh, src)
    return _cache[key]


def reference(rows, n, kind, res):
    """the restatement in both dtypes, computed once per case and left unchanged: terms, loss, the three gradients, the magnitudes"""
    key = ("ref", rows, n, kind, res)
    if key not in _cache:
        enh, src = pair(rows, n, kind)
        out = {}
        for dt in (torch.float64, torch.float32):
            out[dt] = MR.all_grads(enh, src, res, dt)
            out[dt]["mags"] = [MR.magnitudes(enh.to(dt), *r) for r in res]
        _cache[key] = out
    return _cache[key]


def all_cases():
    return [(rows, n, kind, res) for rows, n in SHAPES for res in RESOLUTION_SETS for kind in KINDS]


def rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


def row_rel(g, want):
    """the largest per-row ||g - want|| / ||want|| over the rows with a gradient (a row without one must be exact zeros: asserted apart)"""
    g, want = g.double().cpu(), want.double()
    norm = want.norm(dim=1)
    keep = norm > 0
    return float(((g - want).norm(dim=1)[keep] / norm[keep]).max()) if bool(keep.any()) else 0.0


def mag_dev(m, want):
    return float(((m.double().cpu() - want.double()).abs().amax(dim=(1, 2)) / want.double().amax(dim=(1, 2))).max())


def gates():
    """{name: (gate, worst deviation of the float32 restatement)}"""
    if "gates" not in _cache:
        worst = dict(mags=0.0, value=0.0, g_sc=0.0, g_mag=0.0, g_full=0.0)
        for rows, n, kind, res in all_cases():
            ref = reference(rows, n, kind, res)
            r64, r32 = ref[torch.float64], ref[torch.float32]
            worst["mags"] = max([worst["mags"]] + [mag_dev(a, b) for a, b in zip(r32["mags"], r64["mags"])])
            vals = [(r32["loss"], r64["loss"])] + list(zip(r32["terms"].flatten(), r64["terms"].flatten()))
            worst["value"] = max([worst["value"]] + [rel(a, b) for a, b in vals if float(b) != 0.0])
            for name, _, _ in GRADS:
                worst[name] = max(worst[name], row_rel(r32[name], r64[name]))
        _cache["gates"] = {k: (8 * v, v) for k, v in worst.items()}
    return _cache["gates"]


def device_run(enh, src, res, scw, magw):
    from sehip import mrstft_loss
    e = enh.cuda().requires_grad_(True)
    s = src.cuda().requires_grad_(True)
    loss = mrstft_loss(e, s, res, scw, magw)
    loss.backward()
    assert s.grad is None                                            # sources receives no gradient
    return loss.detach(), e.grad


def test_gates_from_the_restatement():
    g = gates()
    for name, (gate, worst) in g.items():
        print(f"[mrstft] float32 restatement, {name}: worst deviation {worst:.3e}, gate {gate:.3e}")
    assert all(gate > 0 for gate, _ in g.values())
    assert max(g["mags"][0], g["value"][0], g["g_sc"][0]) < 1e-4     # the sharp ones (the mag-only restatement is ill-conditioned)


@pytest.mark.parametrize("res", RESOLUTION_SETS, ids=lambda r: "default" if len(r) == 3 else "x".join(map(str, r[0])))
@pytest.mark.parametrize("rows,n", SHAPES)
def test_values_gradients_and_magnitudes(rows, n, res):
    from sehip import mrstft_terms, ops
    g = gates()
    worst = dict(mags=0.0, value=0.0, g_sc=0.0, g_mag=0.0, g_full=0.0)
    for kind in KINDS:
        enh, src = pair(rows, n, kind)
        want = reference(rows, n, kind, res)[torch.float64]
        for r, m64 in zip(res, want["mags"]):
            m = ops.stft_magnitudes(enh.cuda(), *r)
            assert m.shape == m64.shape and m.dtype == torch.float32
            worst["mags"] = max(worst["mags"], mag_dev(m, m64))
        terms = mrstft_terms(enh.cuda(), src.cuda(), res).cpu()
        assert terms.shape == (len(res), 2) and terms.dtype == torch.float32
        losses = {}
        for name, scw, magw in GRADS:
            loss, grad = device_run(enh, src, res, scw, magw)
            assert loss.shape == () and loss.dtype == torch.float32 and grad.shape == (rows, n)
            assert bool(torch.isfinite(grad).all())                  # (the zero half of 'halfzero' included)
            losses[name] = loss.cpu()
            dead = want[name].norm(dim=1) == 0
            assert not grad.cpu()[dead].any()                        # a row without a gradient has exact zeros
            worst[name] = max(worst[name], row_rel(grad, want[name]))
        vals = [(losses["g_full"], want["loss"])] + list(zip(terms.flatten(), want["terms"].flatten()))
        vals += [(losses["g_sc"], want["terms"][:, 0].mean()), (losses["g_mag"], want["terms"][:, 1].mean())]
        for got, ref in vals:
            if float(ref) == 0.0:
                assert float(got) == 0.0
            else:
                worst["value"] = max(worst["value"], rel(got, ref))
        if kind == "equal":                                          # exactly: sc == 0 and no gradient at all, not a NaN
            assert not terms.any() and all(float(v) == 0.0 for v in losses.values())
            assert not device_run(enh, src, res, 1.0, 0.0)[1].any()
    print(f"[mrstft] rows {rows} n {n} {res}: " + ", ".join(f"{k} {v:.3e} (gate {g[k][0]:.3e})" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= g[k][0], (k, v, g[k])


def test_halfzero_gradient_is_finite_and_equal_is_exactly_zero():
    """the two exact statements once more on their own, on the default resolutions at the shape where every 2048 frame reflects"""
    from sehip import mrstft_terms
    rows, n = 2, 1025
    enh, src = pair(rows, n, "halfzero")
    loss, grad = device_run(enh, src, MR.RESOLUTIONS, 1.0, 1.0)
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad[:, n // 2:]).all()) and bool(grad[:, :n // 2].any())
    enh, src = pair(rows, n, "equal")
    loss, grad = device_run(enh, src, MR.RESOLUTIONS, 1.0, 0.0)
    assert float(loss) == 0.0 and not grad.any()
    assert not mrstft_terms(enh.cuda(), src.cuda(), MR.RESOLUTIONS)[:, 0].any()


def test_two_runs_and_a_captured_replay_give_the_same_bits():
    from sehip import MRSTFTLoss
    (ea, sa), (eb, sb) = pair(4, 1300, "noise"), pair(4, 1300, "halfzero")
    eager = [[device_run(e, s, MR.RESOLUTIONS, 1.0, 1.0) for e, s in ((ea, sa), (eb, sb))] for _ in range(2)]
    for (l0, g0), (l1, g1) in zip(*eager):
        assert torch.equal(l0, l1) and torch.equal(g0, g1)
    mod = MRSTFTLoss()
    # eager warm-up on tensors of its own: a leaf that an eager forward has used stays bound to that forward's stream
    warm = ea.cuda().requires_grad_(True)
    torch.autograd.grad(mod(warm, sa.cuda()), warm)
    del warm
    torch.cuda.synchronize()
    e_s, s_s = ea.cuda().requires_grad_(True), sa.cuda()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss_s = mod(e_s, s_s)
        (grad_s,) = torch.autograd.grad(loss_s, e_s)
    for (e, s), (loss, grad) in (((eb, sb), eager[0][1]), ((ea, sa), eager[0][0])):
        with torch.no_grad():
            e_s.copy_(e.cuda())
            s_s.copy_(s.cuda())
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(loss_s, loss) and torch.equal(grad_s, grad)


def test_wave_l1_module_is_the_sum_of_its_parts():
    from sehip import MRSTFTLoss, mrstft_loss
    from sehip.loss import l1_loss
    enh, src = pair(3, 4000, "noise")
    res = ((512, 128, 512), (256, 64, 200))
    e = enh.cuda().reshape(3, 1, 4000).requires_grad_(True)
    s = src.cuda().reshape(3, 1, 4000)
    mod = MRSTFTLoss(res, sc_weight=0.5, mag_weight=2.0, wave_l1=0.25)
    loss = mod(e, s)
    (grad,) = torch.autograd.grad(loss, e)
    e2 = enh.cuda().reshape(3, 1, 4000).requires_grad_(True)
    parts = mrstft_loss(e2, s, res, 0.5, 2.0) + 0.25 * l1_loss(e2, s)
    (grad2,) = torch.autograd.grad(parts, e2)
    assert grad.shape == (3, 1, 4000) and torch.equal(loss, parts) and torch.equal(grad, grad2)
    assert float(loss.detach()) > float(mrstft_loss(e2, s, res, 0.5, 2.0).detach()) > 0


def test_a_stale_backward_is_refused():
    from sehip import MRSTFTLoss, SehipError
    enh, src = pair(1, 1200, "noise")
    mod = MRSTFTLoss(((128, 50, 100),))
    e = enh.cuda().requires_grad_(True)
    first = mod(e, src.cuda())
    second = mod(e, src.cuda())                                      # the same workspace: only the latest forward can be differentiated
    with pytest.raises(SehipError, match="another forward pass"):
        first.backward()
    second.backward()
    assert bool(torch.isfinite(e.grad).all()) and bool(e.grad.any())
    with pytest.raises(SehipError, match="mrstft_loss.*n=1024"):
        MRSTFTLoss()(e[:, :1024], src.cuda()[:, :1024])             # 1024 samples: one too few for the 2048 resolution
    with pytest.raises(ValueError, match="mrstft_loss"):
        mod(e, src.cuda()[:, :1000])


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


def test_solver_trains_on_l1_mrstft_eager_and_graphed(tmp_path):
    """one train_step and one train_step_graphed of a small causal ConvTasNet with optim.loss 'l1+mrstft', from the same initial state: the
    loss is the module's value on that batch, every gradient is finite, and the graphed step gives the eager loss bits"""
    import copy
    from sehip import distrib
    from sehip.loss import MRSTFTLoss, l1_loss, mrstft_loss
    from sehip.solver import ScalarLog, Solver
    torch.manual_seed(0)
    state = copy.deepcopy(distrib.get_model(solver_config(tmp_path, "l1+mrstft", False).model).state_dict())
    src = 0.1 * torch.randn(2, 2, 1, 8000, generator=torch.Generator().manual_seed(5))
    mix = src.sum(1)
    out = []
    for graphed in (False, True):
        cfg = solver_config(tmp_path, "l1+mrstft", graphed)
        model = distrib.get_model(cfg.model)
        model.load_state_dict(state)
        loss_fn = distrib.get_loss_function(cfg.optim)
        assert isinstance(loss_fn, MRSTFTLoss) and loss_fn.wave_l1 == 1.0
        solver = Solver(copy.deepcopy(cfg), model, distrib.get_optimizer(cfg.optim, model), loss_fn, device="gpu", writer=ScalarLog())
        seen = {}
        loss_fn.register_forward_hook(lambda m, inp, res: seen.update(enhanced=inp[0].detach().clone(), sources=inp[1].detach().clone()))
        mx, sr = solver._prepare_batch(mix, src)
        loss, _ = (solver.train_step_graphed if graphed else solver.train_step)(mx, sr)
        torch.cuda.synchronize()
        grads = solver.model.flat_grads
        assert bool(torch.isfinite(grads).all()) and bool(grads.any())
        if not graphed:                                              # (the hook of the graphed step saw the capture's placeholders)
            assert seen["enhanced"].shape == seen["sources"].shape and seen["enhanced"].numel() == 4 * 8000
            assert torch.equal(loss, mrstft_loss(seen["enhanced"], seen["sources"]) + l1_loss(seen["enhanced"], seen["sources"]))
            assert 0 < float(loss) < 100
        out.append(loss.clone())
    print(f"[mrstft] solver: eager {float(out[0]):.9g} graphed {float(out[1]):.9g}")
    assert torch.equal(out[0], out[1])
