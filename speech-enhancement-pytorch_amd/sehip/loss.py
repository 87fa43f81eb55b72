"""Loss functions of the train step (reference: src/loss.py:14-29 si_snr / loss_sisdr; l1 / mse are
torch.nn.functional in the reference, src/distrib.py:263-275)."""
import torch

from . import ops
from ._lib import SehipError


class _SiSdrLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, est, ref):
        n = est.shape[-1]
        e2 = est.reshape(-1, n).contiguous().float()
        r2 = ref.reshape(-1, n).contiguous().float()
        loss, rowstat = ops.sisnr_fwd(e2, r2)
        ctx.save_for_backward(e2, r2, rowstat)
        ctx.shape = est.shape
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        e2, r2, rowstat = ctx.saved_tensors
        d = ops.sisnr_bwd(e2, r2, rowstat, g.reshape(1).contiguous().float())
        return d.view(ctx.shape), None


def loss_sisdr(inputs, targets):
    """-mean(si_snr(inputs, targets)) over all leading dims (src/loss.py:25-29)."""
    if inputs.shape != targets.shape:
        raise SehipError(f"loss_sisdr: shape mismatch {tuple(inputs.shape)} vs {tuple(targets.shape)}")
    return _SiSdrLoss.apply(inputs, targets)


def si_snr(s1, s2):
    return -loss_sisdr(s1, s2)


class _PitSiSdrLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, est, ref):
        b, s = est.shape[0], est.shape[1]
        n = est.shape[-1]
        e4 = est.reshape(b, s, -1, n).contiguous().float()
        r4 = ref.reshape(b, s, -1, n).contiguous().float()
        loss, rowstat, pairloss, perm = ops.sisnr_pit_fwd(e4, r4)
        ctx.save_for_backward(e4, r4, rowstat, perm)
        ctx.shape = est.shape
        ctx.mark_non_differentiable(perm, pairloss)
        return loss.reshape(()), perm, pairloss

    @staticmethod
    def backward(ctx, g, _gp, _gl):
        e4, r4, rowstat, perm = ctx.saved_tensors
        d = ops.sisnr_pit_bwd(e4, r4, rowstat, perm, g.reshape(1).contiguous().float())
        return d.view(ctx.shape), None


def pit_loss_sisdr(enhance, target, return_comb=False):
    """UtterenceBaasedPermutationInvariantTraining(enhance, target, loss_function=loss_sisdr) of src/loss.py:58-100 on the
    device: enhance / target [B, S, ...], speakers on axis 1.  As in the reference the permutation is chosen once per BATCH
    (on the batch-mean pair losses, no gradient through the choice) and the result is the mean of the matched pairs' losses.
    With return_comb the device tensor perm [S] (perm[j] = estimated speaker matched with target j) is returned as well --
    the reference's list of (ienhance, itarget) pairs without the host round trip."""
    if enhance.shape != target.shape:
        raise SehipError(f"enhance and target shape did not match...{tuple(enhance.shape)}, {tuple(target.shape)}")
    if enhance.dim() < 3:
        raise SehipError("pit_loss_sisdr: expected [batch, speakers, ..., samples]")
    loss, perm, _ = _PitSiSdrLoss.apply(enhance, target)
    return (loss, perm) if return_comb else loss


PIT_POINTWISE_MAX_ROWS = 1 << 20      # PITPW_MAXROWS of csrc/loss.hip: B * C, the pair-matrix kernel's grid extent


def _pit_pointwise_view(shape):
    """(B, S, C, n) the pair-matrix kernel sees for enhance / target [B, S, ..., n]: the last axis is a row's samples and the axes
    between are its rows.  A tensor with more rows than the kernel's grid takes (an STFT-domain estimate [B, S, C, F, T, 2] at the
    shipped size has B C F T rows of 2 samples) is ONE row per (batch, speaker) instead: the terms are element-wise and every
    pair loss is a batch mean, so the grouping changes no value, only which shapes are taken."""
    b, s = int(shape[0]), int(shape[1])
    n = int(shape[-1]) if len(shape) >= 3 else 1
    c = 1
    for d in shape[2:-1]:
        c *= int(d)
    if b * c > PIT_POINTWISE_MAX_ROWS:
        c, n = 1, c * n
    return b, s, c, n


class _PitPointwiseLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, est, ref, mode, partials):
        b, s, c, n = _pit_pointwise_view(est.shape)
        e4 = est.reshape(b, s, c, n).contiguous().float()
        r4 = ref.reshape(b, s, c, n).contiguous().float()
        loss, pairloss, perm = ops.pit_pointwise_fwd(e4, r4, mode, partials)
        ctx.save_for_backward(e4, r4, perm)
        ctx.mode, ctx.shape = mode, est.shape
        ctx.mark_non_differentiable(perm, pairloss)
        return loss.reshape(()), perm, pairloss

    @staticmethod
    def backward(ctx, g, _gp, _gl):
        e4, r4, perm = ctx.saved_tensors
        d = ops.pit_pointwise_bwd(e4, r4, perm, ctx.mode, g.reshape(1).contiguous().float())
        return d.view(ctx.shape), None, None, None


PIT_MAX_SPEAKERS = 6      # PIT_MAXS of csrc/loss.hip
_pit_workspaces = {}      # (device, B, S, C, n) -> partials [blocks, S*S]: scratch of the pair-matrix kernel, consumed by the select kernel
                          # of the same call on the same stream, so one buffer per shape serves every call (and exists before a capture)


def pit_pointwise_workspace(shape, device):
    """The cached pair-matrix workspace for enhance / target of `shape` [B, S, ..., n] on `device`.  pit_loss_pointwise fetches it
    itself; a caller that records the loss into a hipGraph calls this BEFORE the capture begins, so the recording allocates nothing
    but the call's own outputs."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    b, s, c, n = _pit_pointwise_view(shape)
    key = (device, b, s, c, n)
    ws = _pit_workspaces.get(key)
    if ws is None:
        ws = torch.empty(ops.pit_pointwise_blocks(b, s, c, n), s * s, device=device, dtype=torch.float32)
        if not (device.type == "cuda" and torch.cuda.is_current_stream_capturing()):
            _pit_workspaces[key] = ws      # (a buffer born inside a capture lives in that graph's pool: it serves that recording only)
    return ws


def pit_loss_pointwise(enhance, target, mode, return_comb=False):
    """UtterenceBaasedPermutationInvariantTraining(enhance, target, loss_function=l1_loss | mse_loss) of src/loss.py:58-100 on the
    device (mode 'l1' / 0 or 'mse' / 1): enhance / target [B, S, ...], speakers on axis 1, S <= 6.  One pass over the data fills
    the S x S matrix of batch-mean pair losses, a single wave picks the permutation (first minimum in itertools order, no gradient
    through the choice) and the backward pass reads it from device memory: no host round trip, so the call can be recorded into a
    hipGraph, and no atomics, so the bits do not depend on utils.set_deterministic.  With return_comb the device tensor perm [S]
    int32 (perm[j] = estimated speaker matched with target j) is returned as well, as by pit_loss_sisdr."""
    mode = {"l1": 0, "mse": 1}.get(mode, mode)
    if mode not in (0, 1):
        raise SehipError(f"pit_loss_pointwise: mode {mode!r} (expected 'l1' / 0 or 'mse' / 1)")
    if enhance.shape != target.shape:
        raise SehipError(f"enhance and target shape did not match...{tuple(enhance.shape)}, {tuple(target.shape)}")
    if enhance.dim() < 2 or not 1 <= enhance.shape[1] <= PIT_MAX_SPEAKERS:
        raise SehipError(f"pit_loss_pointwise: expected [batch, speakers <= {PIT_MAX_SPEAKERS}, ...], got {tuple(enhance.shape)}")
    from ._lib import require_gpu
    require_gpu(enhance, "pit_loss_pointwise")
    loss, perm, _ = _PitPointwiseLoss.apply(enhance, target, mode, pit_pointwise_workspace(enhance.shape, enhance.device))
    return (loss, perm) if return_comb else loss


def pit_loss(enhance, target, loss_function, return_comb=False):
    """The same for any loss function of this module.  si-sdr, l1 and mse run fused on the device without a host round trip (l1 / mse
    for up to 6 speakers on the GPU: pit_loss_pointwise; return_comb then gives the reference's list of (ienhance, itarget) pairs,
    built from the device permutation with one readback on that opt-in path only).  Any other loss function, or more than 6
    speakers, evaluates the S x S pair matrix with S*S small launches and reads it back once to pick the permutation
    (src/loss.py:67-86).  `psa` is not a PIT loss: the reference's own PIT raises for it (src/loss.py:95 calls the three-argument loss
    with two arguments), so there is no behaviour to match."""
    if loss_function is loss_sisdr:
        return pit_loss_sisdr(enhance, target, return_comb)
    if (loss_function is l1_loss or loss_function is mse_loss) and enhance.shape == target.shape and enhance.dim() >= 2 and \
            1 <= enhance.shape[1] <= PIT_MAX_SPEAKERS and enhance.is_cuda and enhance.numel() > 0:
        res = pit_loss_pointwise(enhance, target, 0 if loss_function is l1_loss else 1, return_comb)
        if not return_comb:
            return res
        return res[0], [(i, j) for j, i in enumerate(res[1].cpu().tolist())]
    if enhance.shape != target.shape:
        raise SehipError(f"enhance and target shape did not match...{tuple(enhance.shape)}, {tuple(target.shape)}")
    from itertools import permutations
    s = enhance.shape[1]
    with torch.no_grad():
        m = torch.stack([torch.stack([loss_function(enhance[:, i].contiguous(), target[:, j].contiguous()) for j in range(s)])
                         for i in range(s)]).cpu()
    best, lmin = None, 1e9
    for pe in permutations(range(s)):
        l = sum(float(m[pe[j], j]) for j in range(s))
        if lmin > l:
            best, lmin = [(pe[j], j) for j in range(s)], l
    loss = sum(loss_function(enhance[:, i].contiguous(), target[:, j].contiguous()) for i, j in best) / s
    return (loss, best) if return_comb else loss


class _PointwiseLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, mode):
        from ._lib import call, ptr, stream, require_gpu
        require_gpu(x, "l1/mse loss")
        xf, yf = x.contiguous().float(), y.contiguous().float()
        acc = torch.zeros(1, dtype=torch.float64, device=x.device)
        loss = torch.empty(1, device=x.device)
        call("sehip_pointwise_loss_fwd", ptr(xf), ptr(yf), xf.numel(), mode, ptr(acc), ptr(loss), stream())
        ctx.save_for_backward(xf, yf)
        ctx.mode, ctx.shape = mode, x.shape
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        from ._lib import call, ptr, stream
        xf, yf = ctx.saved_tensors
        dx = torch.empty_like(xf)
        call("sehip_pointwise_loss_bwd", ptr(xf), ptr(yf), xf.numel(), ctx.mode, ptr(g.reshape(1).contiguous().float()), ptr(dx),
             stream())
        return dx.view(ctx.shape), None, None


def l1_loss(inputs, targets):
    """torch.nn.functional.l1_loss(reduction='mean') as used by src/distrib.py:264-265."""
    if inputs.shape != targets.shape:
        raise SehipError(f"l1_loss: shape mismatch {tuple(inputs.shape)} vs {tuple(targets.shape)}")
    return _PointwiseLoss.apply(inputs, targets, 0)


def mse_loss(inputs, targets):
    """torch.nn.functional.mse_loss(reduction='mean') as used by src/distrib.py:266-267."""
    if inputs.shape != targets.shape:
        raise SehipError(f"mse_loss: shape mismatch {tuple(inputs.shape)} vs {tuple(targets.shape)}")
    return _PointwiseLoss.apply(inputs, targets, 1)


class _PsaLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, enh, tgt, mix):
        from ._lib import call, ptr, stream, require_gpu
        require_gpu(enh, "psa loss")
        e, t, m = enh.contiguous().float(), tgt.contiguous().float(), mix.contiguous().float()
        acc = torch.zeros(1, dtype=torch.float64, device=enh.device)
        loss = torch.empty(1, device=enh.device)
        call("sehip_psa_loss_fwd", ptr(e), ptr(t), ptr(m), e.numel() // 2, ptr(acc), ptr(loss), stream())
        ctx.save_for_backward(e, t, m)
        ctx.shape = enh.shape
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        from ._lib import call, ptr, stream
        e, t, m = ctx.saved_tensors
        de = torch.empty_like(e)
        call("sehip_psa_loss_bwd", ptr(e), ptr(t), ptr(m), e.numel() // 2, ptr(g.reshape(1).contiguous().float()), ptr(de), stream())
        return de.view(ctx.shape), None, None


def loss_phase_sensitive_spectral_approximation(enhance, target, mixture):
    """src/loss.py:32-56 (`optim.loss: psa`): mean (|E| - |T| cos(tanh(Ti / (Tr + eps)) - tanh(Mi / (Mr + eps))))^2 over [..., 2] spectra;
    the gradient flows into `enhance` only (target and mixture are data in the Solver, src/solver.py:480)."""
    if not (enhance.shape == target.shape == mixture.shape) or enhance.shape[-1] != 2:
        raise SehipError(f"psa loss: three [..., 2] tensors of one shape expected, got {tuple(enhance.shape)}, {tuple(target.shape)}, "
                         f"{tuple(mixture.shape)}")
    return _PsaLoss.apply(enhance, target, mixture)
