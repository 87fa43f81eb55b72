"""The permutation-invariant multi-resolution STFT loss (sehip.loss.pit_mrstft_loss) restated in torch on top of tests/mrstft_ref.py, in
the dtype it is asked for: in float64 the oracle of the sehip_mrl_pair_* kernels of csrc/mrstft_loss.hip, in float32 the yardstick their
deviation is measured with.

enhance / target [B, S, ..., n], speakers on axis 1.  For estimated speaker i and target speaker j, with the rows of a pair the B C rows of
(enhance[:, i], target[:, j]):

    terms[r, i, j] = (sc, mag) of resolution r, norms and mean over those rows (mrstft_ref.terms on the two slices)
    M[i, j]        = (1 / R) sum_r (sc_weight sc + mag_weight mag) + wave_l1 mean |enhance[:, i] - target[:, j]|
    perm           = the first minimum of sum_j M[perm[j], j] over itertools.permutations(range(S)), strict '<' from 1e9, j ascending
    loss           = (1 / S) sum_j M[perm[j], j]

Every signal's magnitudes are taken once per resolution and shared by the pairs it is part of.  No gradient flows through the choice of
the permutation, the target gets none, and the conventions of mrstft_ref (gsqrt, gabs, gclamp) carry over; |.| of the waveform term has
derivative 0 at exactly 0 as well."""
from itertools import permutations

import torch

import mrstft_ref as MR


def rows_of(x, k):
    """speaker k of x [B, S, ..., n] as rows [B C, n]"""
    return x[:, k].reshape(-1, x.shape[-1])


def pair_terms(enhance, target, resolutions=MR.RESOLUTIONS):
    """[R, S, S, 2] in the inputs' dtype, differentiable with respect to enhance"""
    S = enhance.shape[1]
    out = []
    for n_fft, hop, win in resolutions:
        X = [MR.magnitudes(rows_of(enhance, i), n_fft, hop, win) for i in range(S)]
        Y = [MR.magnitudes(rows_of(target.detach(), j), n_fft, hop, win) for j in range(S)]
        norm = [torch.sqrt((y * y).sum()) for y in Y]
        logx, logy = [torch.log(x) for x in X], [torch.log(y) for y in Y]
        out.append(torch.stack([torch.stack([torch.stack([MR.gsqrt(((Y[j] - X[i]) ** 2).sum()) / norm[j],
                                                          MR.gabs(logy[j] - logx[i]).mean()]) for j in range(S)]) for i in range(S)]))
    return torch.stack(out)


def wave_l1_pairs(enhance, target):
    """[S, S]: mean |enhance[:, i] - target[:, j]|"""
    S = enhance.shape[1]
    return torch.stack([torch.stack([MR.gabs(rows_of(enhance, i) - rows_of(target.detach(), j)).mean() for j in range(S)])
                        for i in range(S)])


def pair_matrix(terms, l1_pairs, sc_weight=1.0, mag_weight=1.0, wave_l1=0.0):
    m = (sc_weight * terms[..., 0] + mag_weight * terms[..., 1]).sum(0) / terms.shape[0]
    return m + wave_l1 * l1_pairs if wave_l1 else m


def walk(matrix):
    """-> (perm, [(sum, permutation) of every permutation in itertools order]); the sums are taken in the matrix's dtype, j ascending"""
    S = matrix.shape[0]
    m = matrix.detach()
    best, lmin, sums = None, 1e9, []
    for pe in permutations(range(S)):
        l = m[pe[0], 0]
        for j in range(1, S):
            l = l + m[pe[j], j]
        sums.append((float(l), pe))
        if lmin > float(l):
            best, lmin = list(pe), float(l)
    return best, sums


def gap(matrix):
    """(second smallest permutation sum - smallest) / smallest: how far the choice is from flipping; inf for one speaker"""
    sums = sorted(s for s, _ in walk(matrix)[1])
    return float("inf") if len(sums) < 2 else (sums[1] - sums[0]) / sums[0]


def chosen_loss(matrix, perm):
    S = matrix.shape[0]
    l = matrix[perm[0], 0]
    for j in range(1, S):
        l = l + matrix[perm[j], j]
    return l / S


def loss(enhance, target, resolutions=MR.RESOLUTIONS, sc_weight=1.0, mag_weight=1.0, wave_l1=0.0):
    m = pair_matrix(pair_terms(enhance, target, resolutions), wave_l1_pairs(enhance, target), sc_weight, mag_weight, wave_l1)
    return chosen_loss(m, walk(m)[0])


WEIGHTS = (("g_sc", 1.0, 0.0), ("g_mag", 0.0, 1.0), ("g_full", 1.0, 1.0))


def all_grads(enhance, target, resolutions=MR.RESOLUTIONS, wave_l1=0.0, dtype=torch.float64):
    """one forward in `dtype` -> dict: terms [R, S, S, 2]; and for the weights (1, 0), (0, 1), (1, 1) under the names g_sc, g_mag, g_full:
    matrix_*, perm_*, gap_*, loss_* and the gradient with respect to enhance (its shape); wave_l1 is part of all three"""
    e = enhance.detach().to(dtype).clone().requires_grad_(True)
    t = target.detach().to(dtype)
    terms = pair_terms(e, t, resolutions)
    l1 = wave_l1_pairs(e, t)
    out = {"terms": terms.detach()}
    for k, (name, scw, magw) in enumerate(WEIGHTS):
        m = pair_matrix(terms, l1, scw, magw, wave_l1)
        perm = walk(m)[0]
        value = chosen_loss(m, perm)
        tag = name[2:]
        out["matrix_" + tag], out["perm_" + tag], out["gap_" + tag], out["loss_" + tag] = m.detach(), perm, gap(m), value.detach()
        out[name], = torch.autograd.grad(value, e, retain_graph=k + 1 < len(WEIGHTS))
    return out


def planted(B, S, C, n):
    """(enhance, target, perm) float32 on the host with a known answer.  Seed 1000 B + 100 S + 10 C + n.  Target speaker j is white noise
    through y[t] = x[t] + 0.15 j y[t - 1], scaled by 0.05 (j + 1): the speakers differ in colour and in level.  enhance[:, i] is
    target[:, (i + 1) % S] + 0.01 randn, so perm[j] = (j - 1) % S."""
    g = torch.Generator().manual_seed(1000 * B + 100 * S + 10 * C + n)
    x = torch.randn(B, S, C, n, generator=g, dtype=torch.float64)
    noise = torch.randn(B, S, C, n, generator=g, dtype=torch.float64)
    y = torch.empty_like(x)
    a = 0.15 * torch.arange(S, dtype=torch.float64).reshape(1, S, 1)
    prev = torch.zeros(B, S, C, dtype=torch.float64)
    for t in range(n):
        prev = x[..., t] + a * prev
        y[..., t] = prev
    target = (y * (0.05 * (torch.arange(S, dtype=torch.float64) + 1)).reshape(1, S, 1, 1)).float()
    enhance = (target[:, [(i + 1) % S for i in range(S)]].double() + 0.01 * noise).float()
    return enhance, target, [(j - 1) % S for j in range(S)]
