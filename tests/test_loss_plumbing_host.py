"""CPU: what the losses with a workspace share (sehip/_cache.py and the bases in sehip/loss.py): the capture-aware cache and the device
spelling, every workspace entry point on that cache, the generation guard, the one pair check, and the Solver's table of refused
(optim.loss, model, optim.pit_apply) combinations against the behaviour before the table.  No GPU call."""
import pytest
import torch

RES = ((512, 128, 512),)
MR_SHAPE, PIT_SHAPE, STOI_SHAPE, STOI_SR = (2, 1, 4000), (2, 2, 1, 4000), (2, 4000), 10000     # 10 kHz: no resampling table is built


@pytest.fixture
def capturing(monkeypatch):
    state = {"on": False}
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)    # (the cache asks torch about a capture only where a GPU is visible)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: state["on"])
    return state


def test_cache_stores_unless_a_capture_is_recording(capturing):
    from sehip._cache import CaptureAwareCache
    made = []

    def make(*args):
        made.append(args)
        return object()
    cache = CaptureAwareCache()
    first = cache.get("k", make)
    assert cache.get("k", make) is first and made == [()]
    capturing["on"] = True
    a, b = cache.get("other", make, 1, 2), cache.get("other", make, 1, 2)
    assert a is not b and made == [(), (1, 2), (1, 2)] and "other" not in cache.store          # nothing born in a capture is kept
    assert cache.get("k", make) is first                                                       # what was there before still serves
    capturing["on"] = False
    c = cache.get("other", make)
    assert c is not a and c is not b and cache.get("other", make) is c and len(made) == 4


def test_canonical_device(monkeypatch):
    from sehip._cache import canonical_device
    assert canonical_device("cpu") == torch.device("cpu") and canonical_device(torch.device("cuda:1")) == torch.device("cuda", 1)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 3)
    assert canonical_device("cuda") == torch.device("cuda", 3) and str(canonical_device(torch.device("cuda"))) == "cuda:3"


ENTRY_POINTS = ("stoi_loss_workspace", "StoiLoss.workspace", "mrstft_loss_workspace", "MRSTFTLoss.workspace", "pit_mrstft_workspace",
                "PitMRSTFTLoss.workspace", "pit_pointwise_workspace", "metric.stoi_workspace")


def entry_point(name, monkeypatch):
    """the request at the smallest shapes the library takes, on 'cpu'; the process-wide caches start empty for the test"""
    from sehip import loss, metric
    from sehip._cache import CaptureAwareCache
    for mod, attr in ((loss, "_stoi_loss_workspaces"), (loss, "_mrstft_workspaces"), (loss, "_pit_mrstft_workspaces"), (loss, "_pit_workspaces"),
                      (metric, "_stoi_workspaces")):
        assert isinstance(getattr(mod, attr), CaptureAwareCache)
        monkeypatch.setattr(mod, attr, CaptureAwareCache())
    owner, _, method = name.rpartition(".")
    if owner == "metric":
        return lambda: metric.stoi_workspace(2, 4000, STOI_SR, "cpu")
    if owner:
        mod = {"StoiLoss": lambda: loss.StoiLoss(sr=STOI_SR), "MRSTFTLoss": lambda: loss.MRSTFTLoss(RES),
               "PitMRSTFTLoss": lambda: loss.PitMRSTFTLoss(RES)}[owner]()
        shape = {"StoiLoss": STOI_SHAPE, "MRSTFTLoss": MR_SHAPE, "PitMRSTFTLoss": PIT_SHAPE}[owner]
        return lambda: mod.workspace(shape, "cpu")
    return {"stoi_loss_workspace": lambda: loss.stoi_loss_workspace(STOI_SHAPE, STOI_SR, False, "cpu"),
            "mrstft_loss_workspace": lambda: loss.mrstft_loss_workspace(MR_SHAPE, RES, "cpu"),
            "pit_mrstft_workspace": lambda: loss.pit_mrstft_workspace(PIT_SHAPE, RES, "cpu"),
            "pit_pointwise_workspace": lambda: loss.pit_pointwise_workspace(PIT_SHAPE, "cpu")}[name]


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_every_workspace_entry_point_goes_through_the_cache(name, capturing, monkeypatch):
    get = entry_point(name, monkeypatch)
    capturing["on"] = True
    born_in_a_capture = get()
    assert get() is not born_in_a_capture                            # a fresh one for every request: nothing was kept
    capturing["on"] = False
    stored = get()
    assert stored is not born_in_a_capture and type(stored) is type(born_in_a_capture) and get() is stored
    capturing["on"] = True
    assert get() is stored                                           # what exists before a capture serves the recording, and stays in place
    capturing["on"] = False
    assert get() is stored


def test_the_keys_keep_their_contents(capturing):
    """which calls share a workspace, hence a generation counter, is behaviour"""
    from sehip import loss
    assert loss.stoi_loss_workspace(STOI_SHAPE, STOI_SR, True, "cpu") is not loss.stoi_loss_workspace(STOI_SHAPE, STOI_SR, False, "cpu")
    assert loss.stoi_loss_workspace((1, 2, 4000), STOI_SR, False, "cpu") is loss.stoi_loss_workspace(STOI_SHAPE, STOI_SR, False, "cpu")
    mod = loss.StoiLoss(sr=STOI_SR)
    assert mod.workspace((1, 2, 4000), "cpu") is not mod.workspace(STOI_SHAPE, "cpu")          # the module keys on the shape itself
    assert mod.workspace(torch.Size(STOI_SHAPE), "cpu") is mod.workspace(STOI_SHAPE, "cpu")
    assert loss.mrstft_loss_workspace(MR_SHAPE, [[512, 128, 512]], "cpu") is loss.mrstft_loss_workspace(MR_SHAPE, RES, "cpu")
    assert loss.mrstft_loss_workspace(MR_SHAPE, ((512, 128, 256),), "cpu") is not loss.mrstft_loss_workspace(MR_SHAPE, RES, "cpu")
    assert loss.pit_mrstft_workspace(PIT_SHAPE, [[512, 128, 512]], "cpu") is loss.pit_mrstft_workspace(PIT_SHAPE, RES, "cpu")
    assert loss.MRSTFTLoss(RES).workspace(MR_SHAPE, "cpu") is not loss.MRSTFTLoss(RES).workspace(MR_SHAPE, "cpu")      # a module owns its own


STALE = {
    "stoi_loss": ("a StoiLoss", "stoi_loss: another forward pass ran on this workspace before this one's backward pass; give each loss that "
                                "is live at the same time a StoiLoss module of its own"),
    "mrstft_loss": ("an MRSTFTLoss", "mrstft_loss: another forward pass ran on this workspace before this one's backward pass; give each "
                                     "loss that is live at the same time an MRSTFTLoss module of its own"),
    "pit_mrstft_loss": ("a PitMRSTFTLoss", "pit_mrstft_loss: another forward pass ran on this workspace before this one's backward pass; "
                                           "give each loss that is live at the same time a PitMRSTFTLoss module of its own"),
}


@pytest.mark.parametrize("what", sorted(STALE))
def test_generation_guard(what):
    from sehip import SehipError
    from sehip.loss import MRSTFTWorkspace, PitMRSTFTWorkspace, StoiLossWorkspace, _LossWorkspace
    assert all(issubclass(c, _LossWorkspace) for c in (MRSTFTWorkspace, PitMRSTFTWorkspace, StoiLossWorkspace))
    ws = MRSTFTWorkspace(2, 4000, RES, "cpu")
    assert ws.generation == 0
    mine = ws.forward_ran()
    assert mine == ws.generation == 1
    module, sentence = STALE[what]
    ws.refuse_stale(mine, what, module)                              # the latest forward pass: differentiable
    assert ws.forward_ran() == 2
    with pytest.raises(SehipError) as err:
        ws.refuse_stale(mine, what, module)
    assert str(err.value) == sentence
    ws.refuse_stale(2, what, module)


def test_nbytes_is_the_sum_over_the_declared_tensors():
    from sehip.loss import MRSTFTWorkspace, PitMRSTFTWorkspace, StoiLossWorkspace
    for ws in (MRSTFTWorkspace(2, 4000, RES, "cpu"), PitMRSTFTWorkspace(PIT_SHAPE, RES, "cpu"), StoiLossWorkspace(2, 4000, STOI_SR, "cpu")):
        assert ws.nbytes() == sum(4 * t.numel() for t in ws.tensors()) > 4 * ws.fgrad.numel()
    ws = MRSTFTWorkspace(2, 4000, RES, "cpu")                         # 32 frames -> 16 workgroups a row; 512 floats a frame
    assert ws.nbytes() == 4 * (2 * 16 * 3 + 2 + 2 + 1 + 2 * 32 * 512 + 512)


@pytest.fixture
def host_tensors_pass():
    """the device check stood down for host tensors: whatever passes here has allocated and launched nothing"""
    import sehip._lib as _lib
    real = _lib.require_gpu
    _lib.require_gpu = lambda t, what: None
    yield
    _lib.require_gpu = real


@pytest.mark.parametrize("what", ["stoi_loss", "mrstft_loss", "pit_mrstft_loss"])
def test_check_pair_refuses_in_order(what):
    """without the stand-down: a non-tensor is refused before the device is asked for, and a host tensor by the device check"""
    from sehip import SehipError
    from sehip.loss import _check_pair
    x = torch.zeros(2, 2, 1, 4000)
    with pytest.raises(SehipError, match=f"^{what}: needs device tensors$"):
        _check_pair(x.numpy(), x[..., :3000], what)                  # (its shapes differ as well: the order decides)
    with pytest.raises(SehipError, match=f"^{what}: needs device tensors$"):
        _check_pair(x, None, what)
    with pytest.raises(SehipError, match=what) as err:
        _check_pair(x, x[..., :3000], what)                          # host tensors: the device check comes before the shapes
    assert "shapes differ" not in str(err.value)


@pytest.mark.parametrize("what", ["stoi_loss", "mrstft_loss", "pit_mrstft_loss"])
def test_check_pair_shape_refusals(what, host_tensors_pass):
    from sehip import SehipError
    from sehip.loss import _check_pair, _pit_mrstft_shape_check
    x = torch.zeros(2, 2, 1, 4000)
    empty, seven = torch.zeros(0, 2, 1, 4000), torch.zeros(1, 7, 1, 4000)
    for check in (None, _pit_mrstft_shape_check):
        with pytest.raises(ValueError, match=f"^{what}: shapes differ: \\(2, 2, 1, 4000\\) vs \\(2, 2, 1, 3000\\)$"):
            _check_pair(x, x[..., :3000], what, check)
        with pytest.raises(ValueError, match="shapes differ"):
            _check_pair(empty, x, what, check)                       # the shapes before the emptiness
        with pytest.raises(SehipError, match=f"^{what}: empty input of shape \\(0, 2, 1, 4000\\)$"):
            _check_pair(empty, empty, what, check)
        _check_pair(x, x, what, check)
    _check_pair(x[0, 0], x[0, 0], what)                              # [1, 4000] and seven speakers: fine for a loss on rows ...
    _check_pair(seven, seven, what)
    with pytest.raises(SehipError, match=f"^{what}: expected \\[batch, speakers, ..., samples\\], got \\(1, 4000\\)$"):
        _check_pair(x[0, 0], x[0, 0], what, _pit_mrstft_shape_check)   # ... and refused only with the PIT shape check
    with pytest.raises(SehipError, match=f"^{what}: S=7 speakers outside \\[1, 6\\]"):
        _check_pair(seven, seven, what, _pit_mrstft_shape_check)
    with pytest.raises(SehipError, match=f"^{what}: empty input of shape \\(\\)$"):
        _check_pair(torch.zeros(()), torch.zeros(()), what)


LOSSES = ("l1", "mse", "si-sdr", "psa", "stoi", "estoi", "mrstft", "l1+mrstft", "pit-mrstft", "pit-l1+mrstft")    # distrib.get_loss_function's
MODELS = ("dcunet", "dccrn", "conv-tasnet")          # an STFT-domain model, a single-speaker waveform model, a separation model
SPECTRA = "optim.loss '{loss}' is taken on waveforms; model 'dcunet' returns spectra (an STFT-domain model): train it with l1, mse or psa"
NOT_BUILT = "optim.loss '{loss}' with optim.pit_apply is not built: the permutation-invariant losses are si-sdr, l1 and mse"
OWN_PIT = NOT_BUILT + ", and optim.loss 'pit-{loss}' ('pit-mrstft' / 'pit-l1+mrstft'), which is permutation-invariant by itself"
SPEAKERS = ("optim.loss '{loss}' matches estimated with target speakers; model 'dccrn' does not return [batch, speakers, ...] (those are "
            "['conv-tasnet', 'demucs', 'rnn-stft-mask']): train it with '{plain}'")
TWICE = "optim.loss '{loss}' is permutation-invariant by itself: with optim.pit_apply the permutation would be searched twice; drop optim.pit_apply"
# (optim.loss, optim.pit_apply, model) -> the refusal of Solver(config, model=None) with {loss} the name and {plain} the name without
# 'pit-', or None where the Solver went on to distrib.init_distributed(): recorded from the Solver as it was before its three blocks
# of refusals became one table
EXPECTED = {
    ('l1', False, 'dcunet'): None, ('l1', False, 'dccrn'): None, ('l1', False, 'conv-tasnet'): None,
    ('l1', True, 'dcunet'): None, ('l1', True, 'dccrn'): None, ('l1', True, 'conv-tasnet'): None,
    ('mse', False, 'dcunet'): None, ('mse', False, 'dccrn'): None, ('mse', False, 'conv-tasnet'): None,
    ('mse', True, 'dcunet'): None, ('mse', True, 'dccrn'): None, ('mse', True, 'conv-tasnet'): None,
    ('si-sdr', False, 'dcunet'): None, ('si-sdr', False, 'dccrn'): None, ('si-sdr', False, 'conv-tasnet'): None,
    ('si-sdr', True, 'dcunet'): None, ('si-sdr', True, 'dccrn'): None, ('si-sdr', True, 'conv-tasnet'): None,
    ('psa', False, 'dcunet'): None, ('psa', False, 'dccrn'): None, ('psa', False, 'conv-tasnet'): None,
    ('psa', True, 'dcunet'): None, ('psa', True, 'dccrn'): None, ('psa', True, 'conv-tasnet'): None,
    ('stoi', False, 'dcunet'): SPECTRA, ('stoi', False, 'dccrn'): None, ('stoi', False, 'conv-tasnet'): None,
    ('stoi', True, 'dcunet'): SPECTRA, ('stoi', True, 'dccrn'): NOT_BUILT, ('stoi', True, 'conv-tasnet'): NOT_BUILT,
    ('estoi', False, 'dcunet'): SPECTRA, ('estoi', False, 'dccrn'): None, ('estoi', False, 'conv-tasnet'): None,
    ('estoi', True, 'dcunet'): SPECTRA, ('estoi', True, 'dccrn'): NOT_BUILT, ('estoi', True, 'conv-tasnet'): NOT_BUILT,
    ('mrstft', False, 'dcunet'): SPECTRA, ('mrstft', False, 'dccrn'): None, ('mrstft', False, 'conv-tasnet'): None,
    ('mrstft', True, 'dcunet'): SPECTRA, ('mrstft', True, 'dccrn'): OWN_PIT, ('mrstft', True, 'conv-tasnet'): OWN_PIT,
    ('l1+mrstft', False, 'dcunet'): SPECTRA, ('l1+mrstft', False, 'dccrn'): None, ('l1+mrstft', False, 'conv-tasnet'): None,
    ('l1+mrstft', True, 'dcunet'): SPECTRA, ('l1+mrstft', True, 'dccrn'): OWN_PIT, ('l1+mrstft', True, 'conv-tasnet'): OWN_PIT,
    ('pit-mrstft', False, 'dcunet'): SPECTRA, ('pit-mrstft', False, 'dccrn'): SPEAKERS, ('pit-mrstft', False, 'conv-tasnet'): None,
    ('pit-mrstft', True, 'dcunet'): SPECTRA, ('pit-mrstft', True, 'dccrn'): SPEAKERS, ('pit-mrstft', True, 'conv-tasnet'): TWICE,
    ('pit-l1+mrstft', False, 'dcunet'): SPECTRA, ('pit-l1+mrstft', False, 'dccrn'): SPEAKERS, ('pit-l1+mrstft', False, 'conv-tasnet'): None,
    ('pit-l1+mrstft', True, 'dcunet'): SPECTRA, ('pit-l1+mrstft', True, 'dccrn'): SPEAKERS, ('pit-l1+mrstft', True, 'conv-tasnet'): TWICE,
}


def test_solver_refuses_what_it_refused_before_the_table(monkeypatch):
    from sehip import SehipError, distrib
    from sehip.solver import Solver
    from sehip.utils import dict2obj

    class PastTheRefusals(Exception):
        pass

    def init_distributed():
        raise PastTheRefusals()
    monkeypatch.setattr(distrib, "init_distributed", init_distributed)          # the Solver's first step after the refusals
    assert len(EXPECTED) == len(LOSSES) * 2 * len(MODELS)
    for loss in LOSSES:
        assert distrib.get_loss_function(dict2obj({"loss": loss})) is not None   # a name of the registry
        for pit in (False, True):
            for model in MODELS:
                cfg = dict2obj({"model": {"name": model}, "optim": {"loss": loss, "pit_apply": pit}, "dset": {"sample_rate": 16000},
                                "solver": {"epochs": 1}})
                want = EXPECTED[(loss, pit, model)]
                if want is None:
                    with pytest.raises(PastTheRefusals):
                        Solver(cfg, model=None)
                else:
                    with pytest.raises(SehipError) as err:
                        Solver(cfg, model=None)
                    assert str(err.value) == want.format(loss=loss, plain=loss[4:]), (loss, pit, model)
