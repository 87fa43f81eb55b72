"""The multi-resolution STFT loss (sehip.loss.mrstft_loss) restated in torch, in the dtype of its inputs: torch.stft and autograd.  In
float64 it is the oracle of the kernels of csrc/mrstft_loss.hip, in float32 the yardstick their deviation is measured with.

Per resolution (n_fft, hop, win_length): S = torch.stft(x, n_fft, hop, win_length, hann_window(win_length) (periodic), center=True,
pad_mode='reflect'), P = re^2 + im^2, M = sqrt(max(P, 1e-7)) [rows, n_fft / 2 + 1, 1 + n // hop]; X = M(enhanced), Y = M(sources);
sc = ||Y - X||_F / ||Y||_F, mag = mean |log Y - log X|, norms and mean over the whole batch;
loss = (1 / R) sum (sc_weight sc + mag_weight mag).

Conventions of the gradient, applied explicitly where autograd would give NaN or leaves a choice:
  * `gsqrt`: sqrt with derivative 0 at exactly 0, so ||Y - X|| = 0 gives a zero gradient of sc;
  * `gabs`: |.| with derivative 0 at exactly 0;
  * `gclamp`: max(P, 1e-7) passes the gradient where P >= 1e-7 and nothing where the forward clamped;
  * the clean signal receives no gradient."""
import torch

RESOLUTIONS = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))
CLAMP = 1e-7


class _GuardedSqrt(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a):
        s = torch.sqrt(a)
        ctx.save_for_backward(s)
        return s

    @staticmethod
    def backward(ctx, g):
        s, = ctx.saved_tensors
        return torch.where(s > 0, g / (2 * torch.where(s > 0, s, torch.ones_like(s))), torch.zeros_like(g))


def gsqrt(a):
    return _GuardedSqrt.apply(a)


def gabs(a):
    return torch.where(a > 0, a, torch.where(a < 0, -a, torch.zeros_like(a)))


def gclamp(p):
    return torch.where(p >= CLAMP, p, torch.full_like(p, CLAMP))


def magnitudes(x, n_fft, hop, win_length):
    """x [rows, n] -> M [rows, n_fft / 2 + 1, 1 + n // hop] in x's dtype"""
    window = torch.hann_window(win_length, periodic=True, dtype=x.dtype, device=x.device)
    s = torch.stft(x, n_fft, hop, win_length, window, center=True, pad_mode="reflect", return_complex=True)
    return torch.sqrt(gclamp(s.real ** 2 + s.imag ** 2))


def terms(enhanced, sources, resolutions=RESOLUTIONS):
    """[R, 2]: (sc, mag) of each resolution; enhanced / sources [rows, n]"""
    out = []
    for n_fft, hop, win in resolutions:
        x, y = magnitudes(enhanced, n_fft, hop, win), magnitudes(sources.detach(), n_fft, hop, win)
        sc = gsqrt(((y - x) ** 2).sum()) / torch.sqrt((y * y).sum())
        mag = gabs(torch.log(y) - torch.log(x)).mean()
        out.append(torch.stack([sc, mag]))
    return torch.stack(out)


def loss(enhanced, sources, resolutions=RESOLUTIONS, sc_weight=1.0, mag_weight=1.0):
    t = terms(enhanced, sources, resolutions)
    return (sc_weight * t[:, 0] + mag_weight * t[:, 1]).sum() / len(resolutions)


def loss_and_grad(enhanced, sources, resolutions=RESOLUTIONS, sc_weight=1.0, mag_weight=1.0, dtype=torch.float64):
    """-> (loss, terms [R, 2], gradient [rows, n]) as tensors of `dtype`, from inputs of any dtype"""
    e = enhanced.detach().to(dtype).clone().requires_grad_(True)
    s = sources.detach().to(dtype)
    t = terms(e, s, resolutions)
    value = (sc_weight * t[:, 0] + mag_weight * t[:, 1]).sum() / len(resolutions)
    g, = torch.autograd.grad(value, e)
    return value.detach(), t.detach(), g


def all_grads(enhanced, sources, resolutions=RESOLUTIONS, dtype=torch.float64):
    """one forward in `dtype` -> dict: terms [R, 2], loss (both weights 1) and the gradients of the loss with weights (1, 0), (0, 1), (1, 1)"""
    e = enhanced.detach().to(dtype).clone().requires_grad_(True)
    t = terms(e, sources.detach().to(dtype), resolutions)
    sc, mag = t[:, 0].sum() / len(resolutions), t[:, 1].sum() / len(resolutions)
    out = {"terms": t.detach(), "loss": (sc + mag).detach()}
    out["g_sc"], = torch.autograd.grad(sc, e, retain_graph=True)
    out["g_mag"], = torch.autograd.grad(mag, e, retain_graph=True)
    out["g_full"], = torch.autograd.grad(sc + mag, e)
    return out
