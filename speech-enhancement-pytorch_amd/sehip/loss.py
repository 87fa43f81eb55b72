"""Loss functions of the train step (reference: src/loss.py:14-29 si_snr / loss_sisdr; l1 / mse are
torch.nn.functional in the reference, src/distrib.py:263-275)."""
import torch

from . import _lib, ops
from ._cache import CaptureAwareCache, canonical_device
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


def _pit_pointwise_view(shape, fold_above=PIT_POINTWISE_MAX_ROWS):
    """(B, S, C, n) the pair-matrix kernel sees for enhance / target [B, S, ..., n]: the last axis is a row's samples and the axes
    between are its rows.  A tensor with more rows than the kernel's grid takes (an STFT-domain estimate [B, S, C, F, T, 2] at the
    shipped size has B C F T rows of 2 samples) is ONE row per (batch, speaker) instead: the terms are element-wise and every
    pair loss is a batch mean, so the grouping changes no value, only which shapes are taken.  fold_above=None keeps the rows as
    they are (pit_mrstft_loss: a row is a signal with transforms of its own)."""
    b, s = int(shape[0]), int(shape[1])
    n = int(shape[-1]) if len(shape) >= 3 else 1
    c = 1
    for d in shape[2:-1]:
        c *= int(d)
    if fold_above is not None and b * c > fold_above:
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
_pit_workspaces = CaptureAwareCache()     # (device, B, S, C, n) -> partials [blocks, S*S]: scratch of the pair-matrix kernel, consumed by
                                          # the select kernel of the same call on the same stream, so one buffer per shape serves every call


def _pit_pointwise_partials(device, b, s, c, n):
    return torch.empty(ops.pit_pointwise_blocks(b, s, c, n), s * s, device=device, dtype=torch.float32)


def pit_pointwise_workspace(shape, device):
    """The cached pair-matrix workspace for enhance / target of `shape` [B, S, ..., n] on `device`.  pit_loss_pointwise fetches it
    itself; a caller that records the loss into a hipGraph calls this BEFORE the capture begins, so the recording allocates nothing
    but the call's own outputs."""
    device = canonical_device(device)
    view = _pit_pointwise_view(shape)
    return _pit_workspaces.get((device,) + view, _pit_pointwise_partials, device, *view)


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
    _lib.require_gpu(enhance, "pit_loss_pointwise")
    loss, perm, _ = _PitPointwiseLoss.apply(enhance, target, mode, pit_pointwise_workspace(enhance.shape, enhance.device))
    return (loss, perm) if return_comb else loss


def pit_loss(enhance, target, loss_function, return_comb=False):
    """The same for any loss function of this module.  si-sdr, l1, mse and the multi-resolution STFT loss run fused on the device
    without a host round trip (l1 / mse and mrstft_loss / an MRSTFTLoss module for up to 6 speakers on the GPU: pit_loss_pointwise,
    pit_mrstft_loss; return_comb then gives the reference's list of (ienhance, itarget) pairs,
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
    if loss_function is mrstft_loss or isinstance(loss_function, MRSTFTLoss):
        # every signal transformed once, the permutation picked on the device (pit_mrstft_loss); an MRSTFTLoss module brings its
        # resolutions, weights and wave_l1 and keeps the permutation-invariant form's workspaces with it
        if loss_function is mrstft_loss:
            res = pit_mrstft_loss(enhance, target, return_comb=return_comb)
        else:
            res = loss_function.pit()(enhance, target, return_comb)
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


# ---- what the losses with a workspace share: stoi_loss, mrstft_loss, pit_mrstft_loss and their modules ---------------------------------
def _rows_of(shape):
    """the rows of [..., n]: the product of every axis but the last"""
    rows = 1
    for s in shape[:-1]:
        rows *= int(s)
    return rows


def _as_rows(x, view):
    """x as the contiguous fp32 rows the kernels read, cut from the autograd graph (the loss's own backward pass carries the gradient)"""
    return x.detach().reshape(view).contiguous().float()


def _check_pair(enhanced, sources, what, shape_check=None):
    """every refusal that needs no workspace, before anything is allocated or launched; shape_check(shape, what) stands in for the
    refusal of an empty input where a loss asks more of the shape"""
    if not torch.is_tensor(enhanced) or not torch.is_tensor(sources):
        raise SehipError(f"{what}: needs device tensors")
    _lib.require_gpu(enhanced, what)
    _lib.require_gpu(sources, what)
    if enhanced.shape != sources.shape:
        raise ValueError(f"{what}: shapes differ: {tuple(enhanced.shape)} vs {tuple(sources.shape)}")
    if shape_check is not None:
        shape_check(enhanced.shape, what)
    elif enhanced.dim() < 1 or enhanced.numel() == 0:
        raise SehipError(f"{what}: empty input of shape {tuple(enhanced.shape)}")


class _LossWorkspace:
    """The base of the three workspaces.  `generation` counts the forward passes on these buffers: a backward pass whose forward is no
    longer the latest one is refused instead of differentiating the wrong call.  A subclass lists its buffers in tensors()."""
    generation = 0

    def forward_ran(self):
        self.generation += 1
        return self.generation

    def refuse_stale(self, generation, loss, module):
        """`generation` is what forward_ran() gave the forward pass that is about to be differentiated; `module` is the module to
        recommend, with its article ('an MRSTFTLoss')"""
        if self.generation != generation:
            raise SehipError(f"{loss}: another forward pass ran on this workspace before this one's backward pass; give each loss that "
                             f"is live at the same time {module} module of its own")

    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in self.tensors())


class _WorkspaceLoss(torch.nn.Module):
    """The base of the three modules that own their buffers: one workspace per input shape, kept for the life of the module (a captured
    graph refers to them).  A subclass gives WHAT (the name in its refusals), SHAPE_CHECK, _key(shape, device), _make(shape, device) and
    _loss(enhanced, sources, ws, *extra); its forward() is _run() under the subclass's own signature."""
    SHAPE_CHECK = None

    def __init__(self):
        super().__init__()
        self._workspaces = CaptureAwareCache()

    def workspace(self, shape, device):
        """this module's buffers for inputs of `shape` on `device`; call it before a capture that records the loss"""
        return self._workspaces.get(self._key(shape, device), self._make, shape, device)

    def _run(self, enhanced, sources, *extra):
        _check_pair(enhanced, sources, self.WHAT, self.SHAPE_CHECK)      # (before the workspace: a refusal allocates nothing)
        return self._loss(enhanced, sources, self.workspace(enhanced.shape, enhanced.device), *extra)


# ---- STOI / ESTOI as a loss (csrc/stoi_loss.hip behind the forward launches of csrc/stoi.hip) ------------------------------------------
_stoi_loss_workspaces = CaptureAwareCache()    # (rows, n, sr, extended, device) -> StoiLossWorkspace of the functional form


class StoiLossWorkspace(_LossWorkspace):
    """Every buffer of one stoi_loss call on `rows` pairs of n samples at sr, forward and backward: the forward's (as
    sehip.metric.stoi_workspace, but never shared with the metric, so a STOI() call between a forward and its backward changes nothing)
    plus the value pair and the backward's scratch."""

    def __init__(self, rows, n, sr, device):
        from . import metric
        from ._lib import lib
        self.fwd = metric.stoi_buffers(rows, n, sr, device, "stoi_loss")     # the forward's own: p, q, n10, frames, table, sig, kept, src, tob
        for k, v in self.fwd.items():
            setattr(self, k, v)
        f32 = dict(device=self.kept.device, dtype=torch.float32)
        spectra = max(self.frames - 1, 1)
        self.rows, self.n, self.sr = rows, n, int(sr)
        self.d = torch.empty(rows, **f32)
        self.mean = torch.empty((), **f32)
        self.seg = torch.empty(lib().sehip_stoil_segment_floats(rows, self.frames), **f32)
        self.dtob = torch.empty(rows, metric.STOI_BANDS, spectra, **f32)
        self.fgrad = torch.empty(rows, spectra, metric.STOI_FRAME, **f32)
        self.inv = torch.empty(rows, self.frames, device=self.kept.device, dtype=torch.int32)
        self.g10 = None if self.sig is None else torch.empty(rows, self.n10, **f32)

    def tensors(self):
        own = [self.d, self.mean, self.seg, self.dtob, self.fgrad, self.inv, self.level, self.kept, self.src, self.tob] + self.partial
        return own + ([] if self.sig is None else [self.sig, self.g10])       # (the resampling table is metric.stoi_resample_table's)


def stoi_loss_workspace(shape, sr=16000, extended=False, device="cuda"):
    """The cached workspace of the functional stoi_loss / stoi_loss_rows for inputs of `shape` [..., T].  The loss fetches it itself; a
    caller that records the loss into a hipGraph calls this BEFORE the capture begins, so that the recording allocates nothing but
    the call's results."""
    rows, n = _rows_of(shape), int(shape[-1])
    return _stoi_loss_workspaces.get((rows, n, int(sr), bool(extended), canonical_device(device)), StoiLossWorkspace, rows, n, sr, device)


class _StoiLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, est, ref, ws, extended, per_row):
        from . import metric
        e, r = _as_rows(est, (ws.rows, ws.n)), _as_rows(ref, (ws.rows, ws.n))
        ext = int(bool(extended))
        metric.stoi_forward(r, e, ws.fwd, ext, ws.d, ws.mean)
        ctx.ws, ctx.ext, ctx.per_row, ctx.generation, ctx.shape = ws, ext, per_row, ws.forward_ran(), est.shape
        ctx.save_for_backward(*([e] if ws.sig is None else []))   # off 10 kHz the backward pass reads the resampled estimate the forward left
        return torch.neg(ws.d if per_row else ws.mean)

    @staticmethod
    def backward(ctx, g):
        from ._lib import call, ptr, stream
        ws = ctx.ws
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        ws.refuse_stale(ctx.generation, "stoi_loss", "a StoiLoss")
        rows, n, n10, frames = ws.rows, ws.n, ws.n10, ws.frames
        g = g.reshape(rows if ctx.per_row else 1).contiguous().float()
        st = stream()
        est10 = ptr(ctx.saved_tensors[0]) if ws.sig is None else ptr(ws.sig[rows:])
        grad = torch.empty(rows, n, device=g.device, dtype=torch.float32)
        g10 = grad if ws.sig is None else ws.g10
        call("sehip_stoil_segments", ptr(ws.tob), ptr(ws.kept), rows, frames, ctx.ext, ptr(g), int(ctx.per_row),
             1.0 if ctx.per_row else 1.0 / rows, ptr(ws.seg), ptr(ws.dtob), st)
        call("sehip_stoil_bands", est10, rows, n10, ptr(ws.kept), ptr(ws.src), ptr(ws.tob), ptr(ws.dtob), ptr(ws.fgrad), st)
        call("sehip_stoil_compact", ptr(ws.fgrad), ptr(ws.kept), ptr(ws.src), rows, n10, ptr(ws.inv), ptr(g10), st)
        if ws.sig is not None:
            table, p, q, L = ws.table
            call("sehip_stoil_resample_adj", ptr(g10), rows, n, ptr(table), p, q, L, ptr(grad), st)
        return grad.view(ctx.shape), None, None, None, None


def _stoi_loss(enhanced, sources, sr, extended, per_row):
    _check_pair(enhanced, sources, "stoi_loss")
    return _StoiLoss.apply(enhanced, sources, stoi_loss_workspace(enhanced.shape, sr, extended, enhanced.device), bool(extended), per_row)


def stoi_loss(enhanced, sources, sr=16000, extended=False):
    """-mean over all rows of stoi(sources, enhanced, sr, extended) for device tensors [..., T] of equal shape (rows = every axis but the
    last) -> 0-dim float32 device tensor: bit for bit the negation of sehip.metric.STOI(sources, enhanced, sr, extended), computed with
    the same forward launches, and differentiable with respect to `enhanced` (csrc/stoi_loss.hip).  `sources` is the clean signal:
    the frame selection follows it and it receives no gradient.

    The gradient's conventions: the kept-frame set is a constant; sqrt at exactly 0 has derivative 0; the clip min(c y, 6.62 x) passes the
    gradient to the branch the forward took (c y on a tie); a row with fewer than 30 spectra (value 1e-5) has gradient exactly zero.
    No readbacks and no atomics, every sum in a fixed order: two runs give the same bits, and forward + backward can be captured into
    one graph (stoi_loss_workspace(...) before the capture).  After the first call at a shape nothing but the results is allocated.

    Limit of this functional form: all calls at one (rows, T, sr, extended, device) share one workspace, so only the LATEST forward pass
    at a shape can be differentiated; the backward pass of an earlier one (two estimates against one target, say) raises SehipError.
    Give each loss that is live at the same time a StoiLoss module of its own.  Workspaces stay allocated (a captured graph refers to
    their buffers): one per shape, each with the backward's scratch of 450 floats per segment and 256 per spectrum and row."""
    return _stoi_loss(enhanced, sources, sr, extended, False)


def stoi_loss_rows(enhanced, sources, sr=16000, extended=False):
    """The negated value per row, [rows] float32 on the device, differentiable as stoi_loss."""
    return _stoi_loss(enhanced, sources, sr, extended, True)


class StoiLoss(_WorkspaceLoss):
    """stoi_loss(enhanced, sources, sr, extended) as a module that owns its buffers: one workspace per input shape, kept for the life of
    the module (a captured graph refers to them), so feed it a bounded set of shapes -- training segments, not clips of every length."""
    WHAT = "stoi_loss"

    def __init__(self, sr=16000, extended=False):
        super().__init__()
        self.sr, self.extended = int(sr), bool(extended)

    def _key(self, shape, device):
        return (tuple(shape), self.sr, canonical_device(device))

    def _make(self, shape, device):
        return StoiLossWorkspace(_rows_of(shape), int(shape[-1]), self.sr, device)

    def _loss(self, enhanced, sources, ws):
        return _StoiLoss.apply(enhanced, sources, ws, self.extended, False)

    def forward(self, enhanced, sources):
        return self._run(enhanced, sources)

    def extra_repr(self):
        return f"sr={self.sr}, extended={self.extended}"


# ---- the multi-resolution STFT loss (csrc/mrstft_loss.hip) -----------------------------------------------------------------------------
MRSTFT_RESOLUTIONS = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))     # (n_fft, hop, win_length)
_mrstft_workspaces = CaptureAwareCache()       # (rows, n, resolutions, device) -> MRSTFTWorkspace of the functional form


class MRSTFTWorkspace(_LossWorkspace):
    """Every buffer of one mrstft_loss call on `rows` pairs of n samples: the windows, the per-workgroup partial sums of all resolutions,
    the (sc, mag) terms, the loss, the two backward factors per resolution and the frame-gradient scratch (sized for the largest
    resolution; the resolutions run one after another on one stream)."""

    def __init__(self, rows, n, resolutions, device):
        from ._lib import lib
        rows, n = int(rows), int(n)
        self.res_host = ops.mrl_check(resolutions, rows, n, "mrstft_loss")          # refusals first: nothing is allocated for a bad shape
        self.resolutions = tuple(tuple(r) for r in self.res_host.tolist())
        self.rows, self.n = rows, n
        f32 = dict(device=device, dtype=torch.float32)
        self.windows = [ops.mrl_window(nf, w, device) for nf, _, w in self.resolutions]
        self.blocks = [rows * lib().sehip_mrl_blocks(n, h) for _, h, _ in self.resolutions]
        self.offsets = [sum(self.blocks[:r]) for r in range(len(self.blocks))]
        self.partials = torch.empty(sum(self.blocks), 3, **f32)
        self.terms = torch.empty(len(self.resolutions), 2, **f32)
        self.stats = torch.empty(len(self.resolutions), 2, **f32)
        self.loss = torch.empty((), **f32)
        self.fgrad = torch.empty(max(rows * lib().sehip_mrl_frames(n, h) * w for _, h, w in self.resolutions), **f32)

    def tensors(self):
        return [self.partials, self.terms, self.stats, self.loss, self.fgrad] + self.windows


def _mrstft_key(shape, resolutions, device):
    return (_rows_of(shape), int(shape[-1]), tuple(tuple(int(v) for v in r) for r in resolutions), canonical_device(device))


def mrstft_loss_workspace(shape, resolutions=MRSTFT_RESOLUTIONS, device="cuda"):
    """The cached workspace of the functional mrstft_loss / mrstft_terms for inputs of `shape` [..., T].  The loss fetches it itself; a
    caller that records the loss into a hipGraph calls this BEFORE the capture begins, so that the recording allocates nothing but
    the call's results."""
    key = _mrstft_key(shape, resolutions, device)
    return _mrstft_workspaces.get(key, MRSTFTWorkspace, key[0], key[1], resolutions, device)


def _mrstft_forward(enhanced, sources, ws, sc_weight, mag_weight):
    """the forward launches on the rows [rows, n] fp32 of both signals (returned): one per resolution and the finalize; results stay in
    ws.loss / ws.terms / ws.stats"""
    from ._lib import call, ptr, stream
    e, r = _as_rows(enhanced, (ws.rows, ws.n)), _as_rows(sources, (ws.rows, ws.n))
    st = stream()
    for (nf, hop, win), window, off in zip(ws.resolutions, ws.windows, ws.offsets):
        call("sehip_mrl_forward", ptr(e), ptr(r), ws.rows, ws.n, nf, hop, win, ptr(window), ptr(ws.partials[off:]), st)
    call("sehip_mrl_finalize", ptr(ws.partials), len(ws.resolutions), ptr(ws.res_host), ws.rows, ws.n, float(sc_weight), float(mag_weight),
         ptr(ws.stats), ptr(ws.terms), ptr(ws.loss), st)
    return e, r, ws.forward_ran()


class _MRSTFTLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, est, ref, ws, sc_weight, mag_weight):
        e, r, ctx.generation = _mrstft_forward(est, ref, ws, sc_weight, mag_weight)
        ctx.ws, ctx.weights, ctx.shape = ws, (float(sc_weight), float(mag_weight)), est.shape
        ctx.save_for_backward(e, r)
        return ws.loss.clone()

    @staticmethod
    def backward(ctx, g):
        from ._lib import call, ptr, stream
        ws = ctx.ws
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        ws.refuse_stale(ctx.generation, "mrstft_loss", "an MRSTFTLoss")
        e, r = ctx.saved_tensors
        g = g.reshape(1).contiguous().float()
        st = stream()
        R = len(ws.resolutions)
        grad = torch.empty(ws.rows, ws.n, device=g.device, dtype=torch.float32)
        for i, ((nf, hop, win), window) in enumerate(zip(ws.resolutions, ws.windows)):
            call("sehip_mrl_backward", ptr(e), ptr(r), ws.rows, ws.n, nf, hop, win, ptr(window), ptr(ws.stats[i]), ptr(g),
                 ctx.weights[0] / R, ctx.weights[1] / R, ptr(ws.fgrad), st)
            call("sehip_mrl_gather", ptr(ws.fgrad), ws.rows, ws.n, nf, hop, win, int(i > 0), ptr(grad), st)
        return grad.view(ctx.shape), None, None, None, None


def mrstft_loss(enhanced, sources, resolutions=MRSTFT_RESOLUTIONS, sc_weight=1.0, mag_weight=1.0, ws=None):
    """The multi-resolution STFT loss (Yamamoto et al. 2020) of device tensors [..., T] of equal shape (rows = every axis but the last)
    -> 0-dim float32 device tensor, differentiable with respect to `enhanced` (csrc/mrstft_loss.hip).  Per resolution
    (n_fft, hop, win_length): S = torch.stft(row, n_fft, hop, win_length, hann_window(win_length), center=True, pad_mode='reflect'),
    M = sqrt(max(re^2 + im^2, 1e-7)) [rows, n_fft / 2 + 1, 1 + T // hop] (torch's scaling: no division by win_length), X = M(enhanced),
    Y = M(sources), sc = ||Y - X||_F / ||Y||_F and mag = mean |log Y - log X|, norms and mean over the whole batch;
    loss = (1 / R) sum over the resolutions of sc_weight sc + mag_weight mag.  n_fft is a power of two in [64, 2048],
    1 <= hop <= win_length <= n_fft, T > n_fft / 2, 1 to 8 resolutions; anything else raises SehipError before a launch.

    The gradient's conventions: `sources` gets no gradient; a cell the forward clamped (re^2 + im^2 < 1e-7) passes nothing; |.| at
    exactly 0 has derivative 0; ||Y - X|| = 0 gives an exactly zero gradient of the sc term, not a NaN.  No spectrum is stored (the
    backward pass transforms both signals again), no readbacks and no atomics, every sum in a fixed order: two runs give the same bits,
    and forward + backward can be captured into one graph (mrstft_loss_workspace(...) before the capture).  After the first call at a
    shape nothing but the results is allocated.

    Limit of this functional form: all calls at one (rows, T, resolutions, device) share one workspace, so only the LATEST forward pass
    at a shape can be differentiated; the backward pass of an earlier one raises SehipError.  Give each loss that is live at the same
    time an MRSTFTLoss module of its own (or pass `ws`, an MRSTFTWorkspace of the caller's own).  Workspaces stay allocated (a captured graph refers to their buffers): one per shape, each
    with the frame-gradient scratch of win_length floats per frame and row of the largest resolution."""
    _check_pair(enhanced, sources, "mrstft_loss")
    if ws is None:
        ws = mrstft_loss_workspace(enhanced.shape, resolutions, enhanced.device)
    return _MRSTFTLoss.apply(enhanced, sources, ws, float(sc_weight), float(mag_weight))


def mrstft_terms(enhanced, sources, resolutions=MRSTFT_RESOLUTIONS, ws=None):
    """[R, 2] float32 on the device: (sc, mag) of each resolution, from the forward launches of mrstft_loss.  Not differentiable."""
    _check_pair(enhanced, sources, "mrstft_terms")
    if ws is None:
        ws = mrstft_loss_workspace(enhanced.shape, resolutions, enhanced.device)
    _mrstft_forward(enhanced, sources, ws, 1.0, 1.0)
    return ws.terms.clone()


class _MRSTFTModule(_WorkspaceLoss):
    """what MRSTFTLoss and PitMRSTFTLoss share: the settings and how they print"""

    def __init__(self, resolutions=MRSTFT_RESOLUTIONS, sc_weight=1.0, mag_weight=1.0, wave_l1=0.0):
        super().__init__()
        self.resolutions = tuple(tuple(int(v) for v in r) for r in resolutions)
        self.sc_weight, self.mag_weight, self.wave_l1 = float(sc_weight), float(mag_weight), float(wave_l1)

    def extra_repr(self):
        return f"resolutions={self.resolutions}, sc_weight={self.sc_weight}, mag_weight={self.mag_weight}, wave_l1={self.wave_l1}"


class MRSTFTLoss(_MRSTFTModule):
    """mrstft_loss(enhanced, sources, resolutions, sc_weight, mag_weight) as a module that owns its buffers: one workspace per input
    shape, kept for the life of the module (a captured graph refers to them), so feed it a bounded set of shapes.  wave_l1 > 0 adds
    wave_l1 * l1_loss(enhanced, sources), the waveform term of the Demucs denoiser recipe."""
    WHAT = "mrstft_loss"

    def _key(self, shape, device):
        return _mrstft_key(shape, self.resolutions, device)

    def _make(self, shape, device):
        return MRSTFTWorkspace(_rows_of(shape), int(shape[-1]), self.resolutions, device)

    def _loss(self, enhanced, sources, ws):
        loss = _MRSTFTLoss.apply(enhanced, sources, ws, self.sc_weight, self.mag_weight)
        if self.wave_l1 > 0.0:
            loss = loss + self.wave_l1 * l1_loss(enhanced, sources)
        return loss

    def forward(self, enhanced, sources):
        return self._run(enhanced, sources)

    def pit(self):
        """this loss under permutation-invariant training, with its settings and workspaces of its own: pit_loss's helper, built on first
        use and kept through __dict__, so it is no registered submodule and state_dict() is unchanged"""
        pit = self.__dict__.get("_pit")
        if pit is None:
            pit = self.__dict__["_pit"] = PitMRSTFTLoss(self.resolutions, self.sc_weight, self.mag_weight, self.wave_l1)
        return pit


# ---- the permutation-invariant multi-resolution STFT loss (the sehip_mrl_pair_* kernels of csrc/mrstft_loss.hip) ------------------------
_pit_mrstft_workspaces = CaptureAwareCache()   # (B, S, C, n, resolutions, device) -> PitMRSTFTWorkspace of the functional form


def _pit_mrstft_shape_check(shape, what):
    if len(shape) < 3:
        raise SehipError(f"{what}: expected [batch, speakers, ..., samples], got {tuple(shape)}")
    if not 1 <= int(shape[1]) <= PIT_MAX_SPEAKERS:
        raise SehipError(f"{what}: S={int(shape[1])} speakers outside [1, {PIT_MAX_SPEAKERS}] in {tuple(shape)}")
    if any(int(d) == 0 for d in shape):
        raise SehipError(f"{what}: empty input of shape {tuple(shape)}")


class PitMRSTFTWorkspace(_LossWorkspace):
    """Every buffer of one pit_mrstft_loss call on enhance / target of `shape` [B, S, ..., n]: the windows, the per-workgroup sums of all
    resolutions ((2 S S + S) floats per workgroup), the pair terms, the pair matrix, the permutation, the loss, the backward factors per
    (resolution, target), the frame-gradient scratch of the B S C estimated rows at the largest resolution and the small buffers of the
    waveform-L1 pair matrix."""

    def __init__(self, shape, resolutions, device):
        from ._lib import lib
        _pit_mrstft_shape_check(shape, "pit_mrstft_loss")
        b, s, c, n = self.view = _pit_pointwise_view(shape, None)
        self.res_host = ops.mrl_check(resolutions, b * c, n, "pit_mrstft_loss")    # refusals first: nothing is allocated for a bad shape
        self.resolutions = tuple(tuple(r) for r in self.res_host.tolist())
        f32 = dict(device=device, dtype=torch.float32)
        i32 = dict(device=device, dtype=torch.int32)
        R = len(self.resolutions)
        self.windows = [ops.mrl_window(nf, w, device) for nf, _, w in self.resolutions]
        self.floats = [lib().sehip_mrl_pair_blocks(b, s, c, n, h) for _, h, _ in self.resolutions]
        self.offsets = [sum(self.floats[:r]) for r in range(R)]
        self.partials = torch.empty(sum(self.floats), **f32)
        self.terms = torch.empty(R, s, s, 2, **f32)
        self.matrix = torch.empty(s, s, **f32)
        self.perm = torch.empty(s, **i32)
        self.loss = torch.empty((), **f32)
        self.stats = torch.empty(R, s, 2, **f32)
        self.fgrad = torch.empty(max(b * s * c * lib().sehip_mrl_frames(n, h) * w for _, h, w in self.resolutions), **f32)
        self.l1_partials = torch.empty(ops.pit_pointwise_blocks(b, s, c, n), s * s, **f32)
        self.l1_pairs = torch.empty(s, s, **f32)
        self.l1_perm = torch.empty(s, **i32)
        self.l1_loss = torch.empty(1, **f32)

    def tensors(self):
        return [self.partials, self.terms, self.matrix, self.perm, self.loss, self.stats, self.fgrad, self.l1_partials, self.l1_pairs,
                self.l1_perm, self.l1_loss] + self.windows


def _pit_mrstft_check(enhance, target, what="pit_mrstft_loss"):
    _check_pair(enhance, target, what, _pit_mrstft_shape_check)


def _pit_mrstft_key(shape, resolutions, device):
    _pit_mrstft_shape_check(shape, "pit_mrstft_loss")      # (workspace(...) is public: the view below needs [batch, speakers, ..., samples])
    return _pit_pointwise_view(shape, None) + (tuple(tuple(int(v) for v in r) for r in resolutions), canonical_device(device))


def pit_mrstft_workspace(shape, resolutions=MRSTFT_RESOLUTIONS, device="cuda"):
    """The cached workspace of the functional pit_mrstft_loss / pit_mrstft_terms for inputs of `shape` [B, S, ..., n].  The loss fetches it
    itself; a caller that records the loss into a hipGraph calls this BEFORE the capture begins, so that the recording allocates nothing
    but the call's results."""
    return _pit_mrstft_workspaces.get(_pit_mrstft_key(shape, resolutions, device), PitMRSTFTWorkspace, shape, resolutions, device)


def _pit_mrstft_forward(enhance, target, ws, sc_weight, mag_weight, wave_l1):
    """the forward launches on both signals as [B, S, C, n] fp32 (returned): the waveform-L1 pair matrix if it is asked for, one launch
    per resolution and the select; results stay in ws.loss / ws.perm / ws.matrix / ws.terms / ws.stats"""
    from ._lib import call, ptr, stream
    e, r = _as_rows(enhance, ws.view), _as_rows(target, ws.view)
    st = stream()
    b, s, c, n = ws.view
    extra = None
    if wave_l1 > 0.0:
        call("sehip_pit_pointwise_fwd", ptr(e), ptr(r), b, s, c, n, 0, ptr(ws.l1_partials), ptr(ws.l1_pairs), ptr(ws.l1_perm),
             ptr(ws.l1_loss), st)
        extra = ws.l1_pairs
    for (nf, hop, win), window, off in zip(ws.resolutions, ws.windows, ws.offsets):
        call("sehip_mrl_pair_forward", ptr(e), ptr(r), b, s, c, n, nf, hop, win, ptr(window), ptr(ws.partials[off:]), st)
    call("sehip_mrl_pair_select", ptr(ws.partials), len(ws.resolutions), ptr(ws.res_host), b, s, c, n, float(sc_weight), float(mag_weight),
         ptr(extra), float(wave_l1), ptr(ws.terms), ptr(ws.matrix), ptr(ws.perm), ptr(ws.loss), ptr(ws.stats), st)
    return e, r, ws.forward_ran()


MRSTFT_GATHER_ROWS = 65535    # MRL_MAX_ROWS of csrc/mrstft_loss.hip: the rows one sehip_mrl_gather launch takes


class _PitMRSTFTLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, est, ref, ws, sc_weight, mag_weight, wave_l1):
        e, r, ctx.generation = _pit_mrstft_forward(est, ref, ws, sc_weight, mag_weight, wave_l1)
        ctx.ws, ctx.weights, ctx.shape = ws, (float(sc_weight), float(mag_weight), float(wave_l1)), est.shape
        ctx.save_for_backward(e, r)
        perm = ws.perm.clone()
        ctx.mark_non_differentiable(perm)
        return ws.loss.clone(), perm

    @staticmethod
    def backward(ctx, g, _gp):
        from ._lib import call, lib, ptr, stream
        ws = ctx.ws
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None, None
        ws.refuse_stale(ctx.generation, "pit_mrstft_loss", "a PitMRSTFTLoss")
        e, r = ctx.saved_tensors
        g = g.reshape(1).contiguous().float()
        st = stream()
        b, s, c, n = ws.view
        scw, magw, wave_l1 = ctx.weights
        R = len(ws.resolutions)
        rows = b * s * c
        grad = torch.empty(rows, n, device=g.device, dtype=torch.float32)
        if wave_l1 > 0.0:      # d (wave_l1 / S) sum_j mean |enhance[:, perm[j]] - target[:, j]|, written; the resolutions add to it
            gl = g * wave_l1
            call("sehip_pit_pointwise_bwd", ptr(e), ptr(r), ptr(ws.perm), ptr(gl), b, s, c, n, 0, ptr(grad), st)
        for i, ((nf, hop, win), window) in enumerate(zip(ws.resolutions, ws.windows)):
            call("sehip_mrl_pair_backward", ptr(e), ptr(r), b, s, c, n, nf, hop, win, ptr(window), ptr(ws.stats[i]), ptr(ws.perm), ptr(g),
                 scw / R / s, magw / R / s, ptr(ws.fgrad), st)
            per_row = lib().sehip_mrl_frames(n, hop) * win
            for r0 in range(0, rows, MRSTFT_GATHER_ROWS):
                call("sehip_mrl_gather", ptr(ws.fgrad[r0 * per_row:]), min(MRSTFT_GATHER_ROWS, rows - r0), n, nf, hop, win,
                     int(i > 0 or wave_l1 > 0.0), ptr(grad[r0:]), st)
        return grad.view(ctx.shape), None, None, None, None, None


def pit_mrstft_loss(enhance, target, resolutions=MRSTFT_RESOLUTIONS, sc_weight=1.0, mag_weight=1.0, wave_l1=0.0, return_comb=False, ws=None):
    """The multi-resolution STFT loss under batch-level permutation-invariant training (src/loss.py:58-100, as pit_loss_pointwise and
    pit_loss_sisdr have it) of device tensors enhance / target [B, S, ..., n], speakers on axis 1, 1 <= S <= 6 -> 0-dim float32 device
    tensor, differentiable with respect to `enhance` (csrc/mrstft_loss.hip).  For estimated speaker i and target speaker j

        M[i, j] = (1 / R) sum_r (sc_weight sc + mag_weight mag)(enhance[:, i], target[:, j]) + wave_l1 mean |enhance[:, i] - target[:, j]|

    with (sc, mag) the terms of mrstft_loss, norms and mean over the B C rows of the pair; perm is the first minimum of
    sum_j M[perm[j], j] over itertools.permutations(range(S)) (strict '<' from 1e9, the sum in fp32 over j ascending) and the loss is
    (1 / S) sum_j M[perm[j], j].  With return_comb the device tensor perm [S] int32 (perm[j] = the estimate matched with target j) is
    returned as well.  No gradient flows through the choice, `target` gets none, and the conventions of mrstft_loss carry over.

    Every signal is transformed once per resolution -- 2 S transforms per row group fill the S x S matrix -- and the permutation is
    picked and read on the device: no readback and no atomics, every sum in a fixed order, so two runs give the same bits and forward +
    backward can be captured into one graph (pit_mrstft_workspace(...) before the capture).  After the first call at a shape nothing but
    the results is allocated.  The pair terms carry the bits of mrstft_terms(enhance[:, i], target[:, j]).

    Refused before any allocation or launch: shapes that differ (ValueError), fewer than 3 axes, more than 6 speakers, and whatever
    mrstft_loss refuses for B C rows of n samples (SehipError).  As with mrstft_loss all calls at one shape share one workspace, so only
    the LATEST forward pass at a shape can be differentiated; give each loss that is live at the same time a PitMRSTFTLoss of its own
    (or pass `ws`, a PitMRSTFTWorkspace of the caller's own)."""
    _pit_mrstft_check(enhance, target)
    if ws is None:
        ws = pit_mrstft_workspace(enhance.shape, resolutions, enhance.device)
    loss, perm = _PitMRSTFTLoss.apply(enhance, target, ws, float(sc_weight), float(mag_weight), float(wave_l1))
    return (loss, perm) if return_comb else loss


def pit_mrstft_terms(enhance, target, resolutions=MRSTFT_RESOLUTIONS, sc_weight=1.0, mag_weight=1.0, wave_l1=0.0, ws=None):
    """(terms [R, S, S, 2], the pair matrix M [S, S], perm [S] int32) on the device, from the forward launches of pit_mrstft_loss:
    terms[r, i, j] = (sc, mag) of resolution r for (enhance[:, i], target[:, j]).  Not differentiable."""
    _pit_mrstft_check(enhance, target, "pit_mrstft_terms")
    if ws is None:
        ws = pit_mrstft_workspace(enhance.shape, resolutions, enhance.device)
    _pit_mrstft_forward(enhance, target, ws, float(sc_weight), float(mag_weight), float(wave_l1))
    return ws.terms.clone(), ws.matrix.clone(), ws.perm.clone()


class PitMRSTFTLoss(_MRSTFTModule):
    """pit_mrstft_loss(enhance, target, resolutions, sc_weight, mag_weight, wave_l1) as a module that owns its buffers: one workspace per
    input shape, kept for the life of the module (a captured graph refers to them), so feed it a bounded set of shapes.  wave_l1 > 0
    adds wave_l1 * mean |enhance[:, i] - target[:, j]| to every pair before the permutation is picked ('pit-l1+mrstft': the Demucs
    denoiser recipe for separation networks)."""
    WHAT, SHAPE_CHECK = "pit_mrstft_loss", staticmethod(_pit_mrstft_shape_check)

    def _key(self, shape, device):
        return _pit_mrstft_key(shape, self.resolutions, device)

    def _make(self, shape, device):
        return PitMRSTFTWorkspace(shape, self.resolutions, device)

    def _loss(self, enhance, target, ws, return_comb):
        loss, perm = _PitMRSTFTLoss.apply(enhance, target, ws, self.sc_weight, self.mag_weight, self.wave_l1)
        return (loss, perm) if return_comb else loss

    def forward(self, enhance, target, return_comb=False):
        return self._run(enhance, target, return_comb)
