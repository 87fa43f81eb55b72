"""GPU: the contract between the models' workspace cache (sehip/model/flat.py) and the plans' workspaces (sehip/workspace.py), the same
for all six models.  The activations of a forward live in the workspace of its input shape, not in autograd's saved tensors, so
  * a backward pass after a later forward of the same shape must raise,
  * an evicted workspace is closed, and a backward pass that still needs it raises too,
  * a pinned workspace (a captured hipGraph points into it) is never evicted,
  * .to() closes every workspace and moves storage_epoch,
  * a CPU tensor is refused.
Every model at the smallest configuration its own GPU test file builds, with a cache of ONE workspace (SEHIP_WS_CACHE=1)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# name -> (class name in sehip.model, constructor arguments, input shape); the second shape is the same clip at batch 1
MODELS = {
    "DCCRN": ("DCCRN", dict(kernel_num=[16, 16, 32, 32, 64, 64], rnn_units=128, length=4000), (2, 1, 4000)),
    "DCUnet": ("DCUnet", dict(data_type=True, model_complexity=8, model_depth=10), (2, 1, 257, 33, 2)),
    "Demucs": ("Demucs", dict(sources=["a", "b"], audio_channels=2, channels=32, depth=4, norm_starts=2, dconv_lstm=2, dconv_attn=2), (2, 2, 6000)),
    "ConvTasNet": ("ConvTasNet", dict(sources=["None", "None"], N=16, L=8, B=16, H=32, P=3, X=3, R=2, audio_channels=1), (2, 1, 404)),
    "WavUnet": ("WavUnet", dict(unet_nlayers=3, channels_interval=8), (2, 1, 200)),
    "RNNBaseSTFTMask": ("RNNBaseSTFTMask", dict(rnn_type="lstm", bidirectional=False, rnn_hidden=32, rnn_layer=2, num_spk=2, audio_channels=2,
                                                n_fft=30), (2, 2, 16, 16, 2)),
}


def live(model):
    """the workspace the last forward ran in (the cache keeps the most recently used one last)"""
    return next(reversed(model._ws.values()))


@pytest.mark.parametrize("name", sorted(MODELS))
def test_workspace_lifecycle(name, monkeypatch):
    import sehip.model
    from sehip import SehipError
    monkeypatch.setenv("SEHIP_WS_CACHE", "1")
    cls, kw, shape = MODELS[name]
    torch.manual_seed(5)
    model = getattr(sehip.model, cls)(**kw).cuda().train()
    assert model._ws_cap == 1
    g = torch.Generator().manual_seed(6)
    xa = (0.1 * torch.randn(*shape, generator=g)).cuda()
    xb = xa[:1].contiguous()
    stale = rf"{name}\.backward: .*overwritten by a later forward"
    loss = lambda y: (y * y).mean()

    # 1. a later forward of the same shape overwrites the activations of the first
    first = model(xa)
    model(0.5 * xa)
    with pytest.raises(SehipError, match=stale):
        loss(first).backward()

    # 2. a forward at a second shape evicts the only workspace and closes it; its pending backward raises the same
    pending = model(xa)
    ws_a = live(model)
    assert not ws_a.closed and len(model._ws) == 1
    model(xb)
    ws_b = live(model)
    assert ws_b is not ws_a and ws_a.closed and not ws_b.closed and list(model._ws.values()) == [ws_b]
    with pytest.raises(SehipError, match=stale):
        loss(pending).backward()

    # 3. a pinned workspace survives the eviction, and its backward runs
    kept = model(xb)
    ws_b.pinned = True
    model(xa)
    assert not ws_b.closed and ws_b in model._ws.values() and len(model._ws) == 2
    loss(kept).backward()
    torch.cuda.synchronize()
    gn = float(model.flat_grads.norm())
    assert gn > 0 and gn == gn

    # 4. .to() re-creates the flat buffers: every workspace is closed, captured graphs go stale
    old, epoch = list(model._ws.values()), model.storage_epoch
    assert len(old) == 2
    model.to("cuda")
    assert all(w.closed for w in old) and len(model._ws) == 0 and model.storage_epoch > epoch

    # 5. no CPU path
    with pytest.raises(SehipError, match=rf"{name}\.forward got a CPU tensor: the HIP path needs a gfx950 GPU \(no CPU fallback\)"):
        model(xa.cpu())
