"""CPU: ConvTasNet with causal in (False, True) x norm_type in ('gLN', 'cLN') -- module schema against the reference's checkpoint keys
(they move behind Chomp1d when causal), the gradient un-packing table, rejections; the restatement tests/ctn_variants_ref.py against
vectors of the imported reference (tests/golden/convtasnet_variants_*.npz, tools/gen_golden_ctn_variants.py); the new C entry points
(declared, bound, scratch sizes, argument validation before any HIP call)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ctn_variants_ref as V
from oracle import dccrn_oracle as O
from util import load_golden, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = dict(V.VARIANTS, default=dict(causal=False, norm_type="gLN"))
NEW_ENTRY_POINTS = ("sehip_ctn_dwconv_fwd_causal", "sehip_ctn_gln_bwd_causal", "sehip_ctn_cln_apply", "sehip_ctn_cln_dwconv_fwd",
                    "sehip_ctn_cln_bwd_scratch_floats", "sehip_ctn_cln_bwd")


def golden_sd(tag):
    g = load_golden(f"convtasnet_variants_{tag}.npz")
    return g, {k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd.")}


@pytest.mark.parametrize("tag", sorted(ALL))
def test_constructor_schema_and_unpack_table(tag):
    from sehip.model import ConvTasNet
    from sehip import distrib, utils
    m = ConvTasNet(sources=["None", "None"], **V.FIXTURE_KW, **ALL[tag])
    sd = m.state_dict()
    if tag == "default":          # (no fixture of its own at this width: the non-causal cLN file has the same keys and shapes)
        _, ref = golden_sd("cln")
    else:
        _, ref = golden_sd(tag)
    assert list(sd) == list(ref) and all(tuple(sd[k].shape) == tuple(v.shape) for k, v in ref.items())
    assert [n for n, _ in m.named_parameters()] == list(ref)              # optimizer state indices interchange
    second_prelu = "separator.network.2.0.0.net.3.net.2.weight" if ALL[tag]["causal"] else "separator.network.2.0.0.net.3.net.1.weight"
    assert second_prelu in sd and tuple(sd[second_prelu].shape) == (1,)
    m.load_state_dict(ref)
    assert all(torch.equal(m.state_dict()[k], v) for k, v in ref.items())
    st = m.static
    L = st.layout
    real = np.concatenate([L.index_array(n).reshape(-1) for n in L.param_names])
    assert (st.utab[real, 0] >= 0).all() and (st.utab[:, 1:] == -1).all()   # exactly one packed-gradient entry per parameter
    assert len(np.unique(st.utab[real, 0])) == len(real)
    opt = distrib.get_optimizer(utils.dict2obj({"optim": "adam", "lr": 3e-4, "beta1": 0.9, "beta2": 0.999}), m)
    assert len(opt.state_dict()["state"]) == len(ref)


def test_plans_are_cached_per_variant_and_rejections_stay():
    from sehip.model import ConvTasNet
    from sehip import SehipError
    kw = dict(sources=["None", "None"], **V.FIXTURE_KW)
    statics = [ConvTasNet(**kw, **v).static for v in ALL.values()]
    assert len({id(s) for s in statics}) == len(statics)
    assert ConvTasNet(**kw, causal=True, norm_type="cLN").static is ConvTasNet(**kw, **ALL["causal_cln"]).static
    with pytest.raises(SehipError, match="BN"):
        ConvTasNet(**kw, norm_type="BN")
    with pytest.raises(SehipError, match="norm_type"):
        ConvTasNet(**kw, norm_type="id")
    with pytest.raises(SehipError, match="skip"):
        ConvTasNet(**kw, skip=True)
    with pytest.raises(SehipError):
        ConvTasNet(**kw, causal=True, norm_type="cLN")(torch.zeros(1, 1, 400))      # CPU tensor: no fallback


def test_registry_passes_the_options():
    """the configuration block reaches the constructor as keyword arguments (sehip/distrib.py)"""
    from sehip import distrib, utils
    cfg = utils.dict2obj({"name": "conv-tasnet", "num_spk": 2, "sources": ["None", "None"], "skip": False, "sample_rate": 8000,
                          "segment": 4, "causal": True, "norm_type": "cLN", **V.FIXTURE_KW})
    m = distrib.get_model(cfg)
    assert m.cfg.causal and m.cfg.norm_type == "cLN" and "separator.network.2.1.2.net.3.net.3.gamma" in m.state_dict()


@pytest.mark.parametrize("tag", sorted(V.VARIANTS))
def test_restatement_matches_reference_vectors(tag):
    g, p = golden_sd(tag)
    kw = dict(C=2, **V.FIXTURE_KW, **V.VARIANTS[tag])
    leaves = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    taps = {}
    mix = torch.from_numpy(g["mix"])
    est = V.variants_forward(leaves, mix, taps=taps, **kw)
    assert len(taps) == 7
    for k, v in taps.items():
        assert rel_err(v.detach(), g["tap." + k]) < 2e-5, k
    assert est.shape == (2, 2, 1, V.FIXTURE_T) and rel_err(est.detach(), g["est"]) < 2e-5
    loss = O.loss_sisdr(est, torch.from_numpy(g["target"]))
    assert abs(float(loss.detach()) - float(g["loss"])) < 1e-4
    names = sorted(leaves)
    assert len(names) == len([k for k in g if k.startswith("grad.")]) == len([k for k in g if k.startswith("gradG.")])
    worst = 0.0
    for pref, grads in (("grad.", torch.autograd.grad(loss, [leaves[k] for k in names], retain_graph=True)),
                        ("gradG.", torch.autograd.grad((est * torch.from_numpy(g["G"])).sum(), [leaves[k] for k in names]))):
        for k, gr in zip(names, grads):
            ref = torch.from_numpy(g[pref + k])
            worst = max(worst, float((gr - ref).norm()) / (float(ref.norm()) + 1e-30))
            assert float((gr - ref).norm()) <= 5e-4 * float(ref.norm()) + 1e-6, (pref, k)
    print(f"ConvTasNet variant {tag}: restatement vs reference vectors, worst gradient tensor {worst:.2e}")


def test_causal_restatement_does_not_look_ahead():
    g, p = golden_sd("causal_cln")
    kw = dict(C=2, **V.FIXTURE_KW, **V.VARIANTS["causal_cln"])
    mix = torch.from_numpy(g["mix"])
    mix2 = mix.clone()
    t0, L = 500, V.FIXTURE_KW["L"]
    mix2[..., t0:] += 0.1
    s0 = ((t0 - L) // (L // 2) + 1) * (L // 2)
    with torch.no_grad():
        a, b = V.variants_forward(p, mix, **kw), V.variants_forward(p, mix2, **kw)
    assert float((a[..., :s0] - b[..., :s0]).abs().max()) < 1e-6 * float(a.abs().max()) and not torch.equal(a[..., s0:], b[..., s0:])


def test_new_entry_points_declared_and_bound():
    from sehip import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sehip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(sehip_[a-z0-9_]+)\s*\(", text))
    lib = _lib.lib()
    for name in NEW_ENTRY_POINTS:
        assert name in declared and name in _lib.declared_symbols() and hasattr(lib, name), name
    # one row of at most (2 + 7) values per channel + the slope sum per workgroup; at least one workgroup per utterance
    n = lib.sehip_ctn_cln_bwd_scratch_floats(32, 1599, 256)
    assert n >= 32 * (9 * 256 + 1) and n % (9 * 256 + 1) == 0
    assert lib.sehip_ctn_cln_bwd_scratch_floats(2, 200, 96) >= 2 * (9 * 96 + 1)
    assert lib.sehip_ctn_cln_bwd_scratch_floats(0, 200, 96) == 0


def test_new_entry_points_validate_before_any_hip_call():
    from sehip import _lib
    lib = _lib.lib()
    err = lambda: lib.sehip_last_error()
    assert lib.sehip_ctn_cln_apply(None, None, None, None, 2, 100, 100, None, None) != 0 and b"multiple of 8" in err()
    assert lib.sehip_ctn_cln_apply(None, None, None, None, 0, 100, 96, None, None) != 0 and b"empty" in err()
    assert lib.sehip_ctn_cln_dwconv_fwd(None, None, None, None, None, 4, 1, 1, 2, 100, 96, None, None) != 0 and b"3, 5 or 7" in err()
    assert lib.sehip_ctn_cln_dwconv_fwd(None, None, None, None, None, 3, 1, 0, 2, 100, 520, None, None) != 0 and b"multiple of 8" in err()
    assert lib.sehip_ctn_cln_dwconv_fwd(None, None, None, None, None, 3, 0, 0, 2, 100, 96, None, None) != 0 and b"dilation" in err()
    assert lib.sehip_ctn_cln_bwd(None, None, None, None, None, None, 9, 1, 1, 1, 2, 100, 96, None, None, None, None, None) != 0 and b"3, 5 or 7" in err()
    assert lib.sehip_ctn_cln_bwd(None, None, None, None, None, None, 3, 1, 1, 1, 2, 100, 12, None, None, None, None, None) != 0 and b"multiple of 8" in err()
    assert lib.sehip_ctn_cln_bwd(None, None, None, None, None, None, 3, 1, 1, 1, 2, 100, 96, None, None, None, None, None) != 0 and b"missing scratch" in err()
    assert lib.sehip_ctn_dwconv_fwd_causal(None, None, None, None, None, None, 4, 1, None, 2, 100, 96, None, None, None) != 0 and b"3, 5 or 7" in err()
    assert lib.sehip_ctn_gln_bwd_causal(None, None, None, None, None, None, None, 6, 1, 1, 2, 100, 96, None, None, None, None, None, None) != 0 and b"3, 5 or 7" in err()
    assert lib.sehip_ctn_gln_bwd_causal(None, None, None, None, None, None, None, 3, 1, 1, 2, 100, 96, None, None, None, None, None, None) != 0 and b"missing scratch" in err()
    with pytest.raises(_lib.SehipError):
        _lib.call("sehip_ctn_cln_bwd", None, None, None, None, None, None, 3, 1, 1, 1, 2, 100, 96, None, None, None, None, None)
