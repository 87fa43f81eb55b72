"""GPU: what stoi_loss, mrstft_loss and pit_mrstft_loss share, through one parametrised body per property: the generation guard of the
workspace base (the functional form refuses the backward pass of an earlier forward pass, two modules each differentiate their own) and the
capture-aware cache (a workspace asked for before a capture serves the recording, whose replays equal the eager call bit for bit and
allocate nothing).  The smallest shapes the library takes; the numbers themselves are gated in test_gpu_stoi_loss.py,
test_gpu_mrstft_loss.py and test_gpu_mrstft_pit.py.  (4000 samples at 10 kHz are 29 spectra, one short of a STOI segment: that loss is
the constant -1e-5 with a zero gradient here, which the guard and the capture do not care about.)"""
import pytest
import torch

pytestmark = pytest.mark.gpu

RES = ((512, 128, 512),)


def losses():
    from sehip import loss as L
    return {
        "stoi_loss": ((2, 4000), lambda y, x: L.stoi_loss(y, x, 10000), lambda: L.StoiLoss(sr=10000), "a StoiLoss"),
        "mrstft_loss": ((2, 1, 4000), lambda y, x: L.mrstft_loss(y, x, RES), lambda: L.MRSTFTLoss(RES), "an MRSTFTLoss"),
        "pit_mrstft_loss": ((2, 2, 1, 4000), lambda y, x: L.pit_mrstft_loss(y, x, RES), lambda: L.PitMRSTFTLoss(RES), "a PitMRSTFTLoss"),
    }


def pair(shape, seed):
    g = torch.Generator().manual_seed(seed)
    clean = 0.1 * torch.randn(shape, generator=g)
    return clean.cuda(), (clean + 0.05 * torch.randn(shape, generator=g)).cuda()


@pytest.mark.parametrize("what", ["stoi_loss", "mrstft_loss", "pit_mrstft_loss"])
def test_shared_guard(what):
    from sehip import SehipError
    shape, functional, module, recommended = losses()[what]
    x, y0 = pair(shape, 1)
    y1, y2 = y0.clone().requires_grad_(True), (y0 * 0.5).requires_grad_(True)
    first, second = functional(y1, x), functional(y2, x)             # one shape: one workspace, the second forward pass is the latest
    with pytest.raises(SehipError) as err:
        torch.autograd.grad(first, y1)
    assert str(err.value) == (f"{what}: another forward pass ran on this workspace before this one's backward pass; give each loss that is "
                              f"live at the same time {recommended} module of its own")
    (g2,) = torch.autograd.grad(second, y2)
    a, b = module(), module()
    la, lb = a(y1, x), b(y2, x)                                      # two modules: two workspaces
    (ga,), (gb,) = torch.autograd.grad(la, y1), torch.autograd.grad(lb, y2)
    torch.cuda.synchronize()
    assert torch.equal(lb, second) and torch.equal(gb, g2) and torch.equal(la, first)
    assert bool(torch.isfinite(ga).all()) and ga.shape == y1.shape
    if what != "stoi_loss":
        assert bool(ga.any()) and not torch.equal(ga, gb)


@pytest.mark.parametrize("what", ["stoi_loss", "mrstft_loss", "pit_mrstft_loss"])
def test_capture_after_workspace_replays_the_eager_bits_and_allocates_nothing(what):
    shape, _, module, _ = losses()[what]
    x, y = pair(shape, 2)
    y_e = y.clone().requires_grad_(True)
    loss_e = module()(y_e, x)
    (grad_e,) = torch.autograd.grad(loss_e, y_e)
    mod = module()
    ws = mod.workspace(shape, x.device)                              # before the capture: the recording finds its buffers
    x_s, y_s = x.clone(), y.clone().requires_grad_(True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss_s = mod(y_s, x_s)
        (grad_s,) = torch.autograd.grad(loss_s, y_s)
    assert mod.workspace(shape, x.device) is ws and ws.generation == 1
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(loss_s, loss_e) and torch.equal(grad_s, grad_e)
    before = torch.cuda.memory_allocated()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before
    assert torch.equal(loss_s, loss_e) and torch.equal(grad_s, grad_e)
