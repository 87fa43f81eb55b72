#!/usr/bin/env python3
"""tests/golden/convtasnet_variants_{causal_gln,cln,causal_cln}.npz from the IMPORTED reference (build container only; the path of
the reference checkout is the first argument or $SEHIP_REFERENCE).

One file per ConvTasNet variant that the shipped-options fixture (oracle/gen_golden_convtasnet.py) does not cover: causal + gLN,
non-causal + cLN, causal + cLN.  N=32, L=8, B=32, H=96, P=3, X=3, R=2, mono, two sources, a [2, 1, 804] mixture, model seed 7, data
seed 8 (H = 96: 12 sixteen-byte pieces per frame, not a power of two; wide enough that bf16 storage alone leaves the reference's
gradients inside the whole-chain gates, which the 16/16/32 network does not).  Per file: state_dict (sd.*), mix, target, the
bottleneck and every temporal block's output (tap.*), the separated sources (est), the reference's SI-SNR loss and its parameter
gradients (grad.*), a fixed upstream gradient G and the parameter gradients of <est, G> (gradG.*).
Run:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_ctn_variants.py /path/to/reference"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
REFERENCE = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SEHIP_REFERENCE")
if not REFERENCE:
    sys.exit("usage: gen_golden_ctn_variants.py /path/to/reference")
sys.path.insert(0, REFERENCE)
GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
KW = dict(N=32, L=8, B=32, H=96, P=3, X=3, R=2, audio_channels=1)
T = 804
VARIANTS = {"causal_gln": dict(causal=True, norm_type="gLN"), "cln": dict(causal=False, norm_type="cLN"),
            "causal_cln": dict(causal=True, norm_type="cLN")}

from src.model.conv_tasnet import ConvTasNet  # noqa: E402
from src.loss import loss_sisdr  # noqa: E402


def build(out_path, extra):
    torch.manual_seed(7)
    model = ConvTasNet(sources=["None", "None"], **KW, **extra)
    g = torch.Generator().manual_seed(8)
    with torch.no_grad():   # non-trivial norm affine terms and PReLU slopes
        for name, prm in model.named_parameters():
            if name.endswith("gamma"):
                prm.copy_(1 + 0.2 * torch.randn(prm.shape, generator=g))
            if name.endswith("beta"):
                prm.copy_(0.1 * torch.randn(prm.shape, generator=g))
            if prm.numel() == 1:
                prm.copy_(0.25 + 0.1 * torch.randn(prm.shape, generator=g))
    mix = 0.3 * torch.randn(2, 1, T, generator=g)
    with torch.no_grad():   # targets = the untrained network's own output + 30 % noise: SI-SNR around +10 dB (see gen_golden_convtasnet.py)
        e0 = model(mix)
    tgt = e0 + 0.3 * e0.std() * torch.randn(e0.shape, generator=g)
    G = torch.randn(e0.shape, generator=g) / e0.numel() ** 0.5
    out = {"sd." + k: v.detach().clone().numpy() for k, v in model.state_dict().items()}
    taps = {}
    net = model.separator.network
    hooks = [net[1].register_forward_hook(lambda m, a, o: taps.__setitem__("bottleneck", o.detach().clone()))]
    for r in range(KW["R"]):
        for i in range(KW["X"]):
            hooks.append(net[2][r][i].register_forward_hook(lambda m, a, o, r=r, i=i: taps.__setitem__(f"block{r}.{i}", o.detach().clone())))
    est = model(mix)
    loss = loss_sisdr(est, tgt)
    loss.backward()
    for h in hooks:
        h.remove()
    for k, v in taps.items():
        out["tap." + k] = v.numpy()
    out.update(mix=mix.numpy(), target=tgt.numpy(), est=est.detach().numpy(), loss=np.float32(loss.item()), G=G.numpy())
    for k, prm in model.named_parameters():
        out["grad." + k] = prm.grad.clone().numpy()
    model.zero_grad()
    for prm in model.parameters():
        prm.grad = None
    (model(mix) * G).sum().backward()
    for k, prm in model.named_parameters():
        out["gradG." + k] = prm.grad.clone().numpy()
    np.savez_compressed(out_path, **out)
    print(os.path.basename(out_path), len(out), "entries; est", tuple(est.shape), "loss", loss.item(), os.path.getsize(out_path), "bytes")


if __name__ == "__main__":
    for tag, extra in VARIANTS.items():
        build(os.path.join(GOLDEN, f"convtasnet_variants_{tag}.npz"), extra)
