"""fp32 / float64 restatement of ConvTasNet for causal in (False, True) x norm_type in ('gLN', 'cLN') -- TEST INFRASTRUCTURE ONLY
(reference: src/model/conv_tasnet.py:243 + :374-383 + :405-419 causal padding and Chomp1d, :422-435 chose_norm, :439-461 cLN).

The functions of oracle/convtasnet_oracle.py (cln, gln, _prelu, overlap_and_add) with the two options the oracle module does not
have: the padding (P - 1) d in front of the depthwise convolution when causal, norm_type applied to BOTH norms of every temporal
block, and the checkpoint keys one slot further behind Chomp1d.  Same hooks as convtasnet_forward: taps=, act_masks= ({"block{r}.{i}":
(mask1, mask2), "mask": mask}: given PReLU / mask-ReLU branches), sim= (Bf16Sim: bf16 storage at the HIP path's layer boundaries),
plus pre= (a dict that receives the branches this run took, in act_masks format).  Pinned against vectors of the imported
reference by tests/test_ctn_variants_host.py (tests/golden/convtasnet_variants_*.npz, tools/gen_golden_ctn_variants.py)."""
import torch
import torch.nn.functional as F

from oracle import convtasnet_oracle as CT
from oracle.convtasnet_oracle import Bf16Sim, NoSim   # noqa: F401  (re-exported for the tests)

FIXTURE_KW = dict(N=32, L=8, B=32, H=96, P=3, X=3, R=2, audio_channels=1)
FIXTURE_T = 804
VARIANTS = {"causal_gln": dict(causal=True, norm_type="gLN"), "cln": dict(causal=False, norm_type="cLN"),
            "causal_cln": dict(causal=True, norm_type="cLN")}


def inner_keys(q, causal):
    """second PReLU / norm of the block with prefix q ('...net.')"""
    o = 1 if causal else 0
    return q + f"3.net.{1 + o}.weight", q + f"3.net.{2 + o}.gamma", q + f"3.net.{2 + o}.beta"


def depthwise(h, w, dilation, causal):
    """h [M, H, K], w [H, 1, P]: h2[t] = sum_j w[j] h[t + (j - c) d], c = P - 1 (causal: zeros before frame 0) or P/2"""
    P = w.shape[-1]
    if causal:
        return F.conv1d(F.pad(h, ((P - 1) * dilation, 0)), w, dilation=dilation, groups=h.shape[1])
    return F.conv1d(h, w, padding=(P - 1) * dilation // 2, dilation=dilation, groups=h.shape[1])


def norm_fn(norm_type):
    return {"cLN": CT.cln, "gLN": CT.gln}[norm_type]


def variants_forward(p, mixture, causal=False, norm_type="gLN", C=2, N=128, L=40, B=128, H=256, P=3, X=7, R=2, audio_channels=1,
                     taps=None, act_masks=None, sim=NoSim, pre=None):
    """mixture [M, ac, T] -> separated sources [M, C, ac, T]"""
    nf = norm_fn(norm_type)
    w = F.relu(F.conv1d(mixture, p["encoder.conv1d_U.weight"], stride=L // 2))
    net = "separator.network."
    x = sim.act(CT.cln(w, p[net + "0.gamma"], p[net + "0.beta"]))
    x = sim.act(F.conv1d(x, sim.weight(p[net + "1.weight"])))
    if taps is not None:
        taps["bottleneck"] = x
    for r in range(R):
        for i in range(X):
            q, b = f"{net}2.{r}.{i}.net.", f"block{r}.{i}"
            a2, g2, b2 = inner_keys(q, causal)
            m1, m2 = (None, None) if act_masks is None else act_masks[b]
            h1 = sim.act(F.conv1d(x, sim.weight(p[q + "0.weight"])))
            n1 = sim.act(nf(CT._prelu(h1, p[q + "1.weight"], m1), p[q + "2.gamma"], p[q + "2.beta"]))
            h2 = sim.act(depthwise(n1, p[q + "3.net.0.weight"], 2 ** i, causal))
            u = sim.act(nf(CT._prelu(h2, p[a2], m2), p[g2], p[b2]))
            if pre is not None:
                pre[b] = (h1.detach() > 0, h2.detach() > 0)
            x = sim.act(F.conv1d(u, sim.weight(p[q + "3.pointwise_conv.weight"])) + x)
            if taps is not None:
                taps[b] = x
    m, n, k = w.shape
    score = sim.act(F.conv1d(x, sim.weight(p[net + "3.weight"]))).view(m, C, n, k)
    if pre is not None:
        pre["mask"] = score.detach() > 0
    mask = F.relu(score) if act_masks is None else score * act_masks["mask"].to(score.dtype)
    est = F.linear((w.unsqueeze(1) * mask).transpose(2, 3), p["decoder.basis_signals.weight"])
    est = CT.overlap_and_add(est.view(m, C, k, audio_channels, L).transpose(2, 3), L // 2)
    return F.pad(est, (0, mixture.shape[-1] - est.shape[-1]))


def grad_dev(ga, gb, names):
    """(global relative difference, worst relative difference among the tensors that carry > 3 % of the gradient's norm)"""
    num = sum(float((ga[k].double() - gb[k].double()).norm()) ** 2 for k in names)
    den = sum(float(gb[k].double().norm()) ** 2 for k in names)
    worst = max((float((ga[k].double() - gb[k].double()).norm() / gb[k].double().norm()) for k in names
                 if float(gb[k].double().norm()) > 0.03 * den ** 0.5), default=0.0)
    return (num / den) ** 0.5, worst


def fixed_g_grads(sd, mixture, G, variant, sim=NoSim, act_masks=None, pre=None, **kw):
    """({name: gradient of <est, G>}, est) of the restatement"""
    p = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    est = variants_forward(p, mixture, sim=sim, act_masks=act_masks, pre=pre, **variant, **kw)
    (est * G).sum().backward()
    return {k: p[k].grad for k in sd}, est.detach()
