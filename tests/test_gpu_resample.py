"""julius.resample_frac on the device (csrc/resample.hip) and DeviceBatcher's `rates` argument.

Op-local: six ratios (and 640 -> 441 for the direct kernel), rows of 1 .. 40 * old + 13 samples and one that spans several workgroup
tiles in ONE ragged flat buffer, a call in which one workgroup strides over the tiles of its row, every output sample against the float64
evaluation of the formula in include/sehip.h with the same fp32 table, within the bound of a K-term fp32 dot product in any
summation order, (K + 2) * 2^-24 * sum_k |kernels[p][k]| * |x_k|; lengths, guard words behind the buffer, run-to-run bits.
Plumbing: a batch that mixes 48 kHz, 44.1 kHz and 16 kHz utterances through `rates` is bit-identical to the batch built from the
same utterances resampled by ops.resample_frac first.
Reference semantics: against oracle.demucs_oracle.resample_frac in float64 followed by the reference's z-score, crop and collate
(oracle/data_oracle.py).  The op-local errors measured on an MI355X are in DESIGN.md section 4.2; the batch figures, which the gate
of test_batch_matches_the_reference_semantics is built from, are in that test's docstring."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RATIOS = ((48000, 16000), (44100, 16000), (16000, 44100), (22050, 16000), (1, 2), (2, 1))
DIRECT = (16000, 11025)      # 640 -> 441: a 64-frame window of 170 KB does not fit the LDS, so this ratio lands on resample_direct_kernel
GUARD = 64
_cache = {}


def _formula64(x, table, old, new, width):
    """y[m] = sum_k h[p][k] x[clamp(q * old + k - width)] and the bound's sum_k |h_k| |x_k|, in float64; x [n], table [new][K] float64.
    (The K-sample windows of all frames are one strided view of the clamped signal; the sums are a float64 matrix product.)"""
    n, K = x.shape[0], table.shape[1]
    m = n * new // old
    if m == 0:
        return np.zeros(0), np.zeros(0)
    frames = (m + new - 1) // new
    xpad = x[np.clip(np.arange((frames - 1) * old + K) - width, 0, n - 1)]
    win = np.lib.stride_tricks.sliding_window_view(xpad, K)[::old]
    assert win.shape == (frames, K)
    return (win @ table.T).reshape(-1)[:m], (np.abs(win) @ np.abs(table).T).reshape(-1)[:m]


def _long_row(old):
    """samples of the row that spans several tiles of whichever kernel takes the ratio: 200 frames against the phase kernel's 64-frame
    tile of the large ratios; more than three decimator tiles (2048 outputs) / phase tiles (up to 1024 frames) for the small ones"""
    return 200 * old + 13 if old >= 100 else 3 * 2048 * old + 5 * old + 1


def _case(old_sr, new_sr):
    """rows, their float64 reference and bound: computed once per ratio and shared"""
    key = (old_sr, new_sr)
    if key not in _cache:
        from sehip import ops
        table, width, old, new = ops.resample_kernels(old_sr, new_sr)
        lens = [1, 5] + ([old - 1] if old - 1 >= 1 else []) + [old, old + 1, 3 * old + 7, 40 * old + 13, _long_row(old)]
        g = torch.Generator().manual_seed(1000 * old + new)
        rows = [0.3 * torch.randn(n, generator=g) + 0.05 for n in lens]
        t64 = table.double().numpy()
        ref = [_formula64(r.double().numpy(), t64, old, new, width) for r in rows]
        _cache[key] = (table, width, old, new, lens, rows, ref)
    return _cache[key]


def _tile_frames(kernel):
    """frames (of `new` output samples) per workgroup tile, from what sehip_last_kernel reports; None for the untiled direct kernel"""
    if kernel.startswith("resample_decim"):
        return 2048
    if kernel.startswith("resample_phase"):
        return 64 * int(kernel.split("wf=")[1].split()[0])
    assert kernel.startswith("resample_direct"), kernel
    return None


def _check_rows(out, oof, ref, K, lens):
    """every row of `out` within the fp32 dot-product bound of its float64 reference; -> worst error / bound"""
    worst = 0.0
    for i, (y64, mag) in enumerate(ref):
        y = out[int(oof[i]):int(oof[i + 1])].double().numpy()
        assert y.shape == y64.shape
        bound = (K + 2) * 2.0 ** -24 * mag
        err = np.abs(y - y64)
        if len(err):
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert bool((err <= bound).all()), (i, lens[i], int(err.argmax()), float(err.max()), float(bound[err.argmax()]))
    return worst


def _run_flat(rows, old_sr, new_sr):
    from sehip import ops
    from sehip._lib import call, ptr, stream
    dev = torch.device("cuda")
    table, width, old, new = ops.resample_kernels(old_sr, new_sr, dev)
    lens = [int(r.shape[0]) for r in rows]
    off = np.zeros(len(rows) + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    oof = np.zeros(len(rows) + 1, dtype=np.int64)
    oof[1:] = np.cumsum([n * new // old for n in lens])
    raw, d_off, d_oof = torch.cat(rows).to(dev), torch.from_numpy(off).to(dev), torch.from_numpy(oof).to(dev)   # (named: alive until the launch)
    out = torch.full((int(oof[-1]) + GUARD,), 12345.0, device=dev)
    call("sehip_resample_frac", ptr(raw), ptr(d_off), len(rows), ptr(table), old, new, width, ptr(out), ptr(d_oof), stream())
    torch.cuda.synchronize()
    return out.cpu(), oof


@pytest.mark.parametrize("old_sr,new_sr", RATIOS + (DIRECT,))
def test_resample_rows_against_float64(old_sr, new_sr):
    from sehip import _lib
    table, width, old, new, lens, rows, ref = _case(old_sr, new_sr)
    K = 2 * width + old
    out, oof = _run_flat(rows, old_sr, new_sr)
    kernel = _lib.lib().sehip_last_kernel().decode()
    print(f"[resample {old}->{new}] K={K} rows={lens} kernel: {kernel}")
    assert [int(oof[i + 1] - oof[i]) for i in range(len(lens))] == [int(new * n / old) for n in lens]
    assert [_lib.lib().sehip_resample_out_len(n, old_sr, new_sr) for n in lens] == [int(new * n / old) for n in lens]
    if old == 3:
        assert oof[3] == oof[2]                                  # the row of old - 1 samples yields nothing
    if (old_sr, new_sr) == DIRECT:
        assert kernel.startswith("resample_direct")
    elif new == 1:
        assert kernel.startswith("resample_decim")
    else:
        assert kernel.startswith("resample_phase")
    tile = _tile_frames(kernel)
    if tile is not None:                                         # the long row really spans several workgroup tiles
        assert -(-int(oof[-1] - oof[-2]) // new) > 3 * tile, (kernel, lens[-1])
    assert bool((out[int(oof[-1]):] == 12345.0).all()), "wrote past out_off[rows]"
    worst = _check_rows(out, oof, ref, K, lens)
    print(f"[resample {old}->{new}] worst error / bound = {worst:.4f}")
    again, _ = _run_flat(rows, old_sr, new_sr)
    assert torch.equal(out.view(torch.int32), again.view(torch.int32)), "two runs differ in their bits"


@pytest.mark.parametrize("old_sr,new_sr", ((44100, 16000), (48000, 16000), DIRECT))
def test_one_block_strides_over_the_tiles_of_its_row(old_sr, new_sr):
    """2048 rows of 5 samples around the long row: with more than 2048 rows a row gets ONE workgroup, which then walks all the
    tiles of the long row (phase: 200 frames in tiles of 64; decimator: 6149 outputs in tiles of 2048; direct: 256 outputs per
    step).  Same float64 bound."""
    from sehip import _lib
    table, width, old, new, lens, rows, ref = _case(old_sr, new_sr)
    K, t64 = 2 * width + old, table.double().numpy()
    g = torch.Generator().manual_seed(77)
    short = 0.3 * torch.randn(2048, 5, generator=g) - 0.1
    all_rows = list(short[:1000]) + [rows[-1]] + list(short[1000:])
    short_ref = [_formula64(r.double().numpy(), t64, old, new, width) for r in short]
    all_ref = short_ref[:1000] + [ref[-1]] + short_ref[1000:]
    out, oof = _run_flat(all_rows, old_sr, new_sr)
    kernel = _lib.lib().sehip_last_kernel().decode()
    tile = _tile_frames(kernel)
    n_out = int(oof[1001] - oof[1000])
    assert (-(-n_out // new) > 3 * tile) if tile is not None else (n_out > 3 * 256), (kernel, n_out)
    assert bool((out[int(oof[-1]):] == 12345.0).all()), "wrote past out_off[rows]"
    worst = _check_rows(out, oof, all_ref, K, [int(r.shape[0]) for r in all_rows])
    print(f"[resample {old}->{new}, 2049 rows] kernel: {kernel}; worst error / bound = {worst:.4f}")


def test_resample_frac_tensor_interface():
    from oracle import demucs_oracle as O
    from sehip import ops
    from sehip._lib import SehipError
    g = torch.Generator().manual_seed(5)
    x = 0.2 * torch.randn(2, 3, 1000, generator=g)
    for old_sr, new_sr in ((44100, 16000), (48000, 16000), (16000, 44100)):
        y = ops.resample_frac(x.cuda(), old_sr, new_sr)
        ref = O.resample_frac(x, old_sr, new_sr)
        assert tuple(y.shape) == tuple(ref.shape) and y.dtype == torch.float32 and y.is_cuda
        flat, oof = _run_flat(list(x.reshape(6, 1000)), old_sr, new_sr)
        assert torch.equal(y.cpu().reshape(-1).view(torch.int32), flat[:int(oof[-1])].view(torch.int32))
        assert float((y.cpu() - ref).abs().max()) < 1e-5        # (sanity against the fp32 oracle; the float64 gate is above)
    xc = x.cuda()
    assert ops.resample_frac(xc, 16000, 16000) is xc
    assert tuple(ops.resample_frac(xc[..., :2], 48000, 16000).shape) == (2, 3, 0)
    assert ops.resample_frac(xc.transpose(0, 1), 48000, 16000).shape == (3, 2, 333)     # non-contiguous input
    for bad in (xc.double(), xc[..., :0]):
        with pytest.raises(SehipError):
            ops.resample_frac(bad, 48000, 16000)


# ---- the batch: 48 kHz, 44.1 kHz and 16 kHz utterances mixed, C = 2, S = 2, segments of 1000 samples at 16 kHz -------------------
SEG = 1000
CFG = types.SimpleNamespace(segment=SEG / 16000, sample_rate=16000)
#        raw length, rate   -> resampled length (segments without a crop, drop_last)
UTTS = ((2400, 48000),      # 800  (0: padded to one segment by collate_fn_pad)
        (9800, 44100),      # 3555 (3)
        (1700, 16000),      # 1700 (1)
        (4000, 48000),      # 1333 (1)
        (2000, 44100))      # 725  (0)


def _items():
    if "items" not in _cache:
        g = torch.Generator().manual_seed(21)
        _cache["items"] = [(0.1 * torch.randn(2, n, generator=g) + 0.01, 0.1 * torch.randn(2, 2, n, generator=g) - 0.02, f"utt{i}")
                           for i, (n, _) in enumerate(UTTS)]
    return _cache["items"]


def _same_bits(a, b):
    if not torch.is_tensor(a):
        return a == b
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("sample_length", (0, 1500))
@pytest.mark.parametrize("normalize", ("", "z-score", "linear-scale"))
def test_rates_plumbing_is_exact(normalize, sample_length):
    from sehip import ops
    from sehip.data import DeviceBatcher
    items, rates = _items(), [r for _, r in UTTS]
    items_rs = [(ops.resample_frac(m.cuda(), r, 16000).cpu(), ops.resample_frac(s.cuda(), r, 16000).cpu(), name)
                for (m, s, name), r in zip(items, rates)]
    assert [int(m.shape[-1]) for m, _, _ in items_rs] == [800, 3555, 1700, 1333, 725]
    starts = [0, 1200, 100, 0, 0] if sample_length else None
    b = DeviceBatcher(CFG, normalize=normalize, sample_length=sample_length, drop_last=True)
    got = b(items, starts=starts, rates=rates)
    want = b(items_rs, starts=starts)
    assert want[5] == ([1, 1, 1, 1, 1] if sample_length else [1, 3, 1, 1, 1]) and got[5] == want[5]
    assert got[4] == want[4] == [f"utt{i}" for i in range(len(items))]
    assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1])
    for gm, wm in zip(got[2] + got[3], want[2] + want[3]):
        assert gm.keys() == wm.keys() and all(_same_bits(gm[k], wm[k]) for k in gm)
    same = b([items[2]], starts=[100] if sample_length else None, rates=16000)        # every rate at the target: today's path
    plain = b([items[2]], starts=[100] if sample_length else None)
    assert _same_bits(same[0], plain[0]) and _same_bits(same[1], plain[1])


def test_batch_matches_the_reference_semantics():
    """z-score batch against oracle.demucs_oracle.resample_frac in float64 + the reference's normalise / crop / collate
    (oracle/data_oracle.py).  Gate per utterance: 2 x the deviation of the fp32 CPU oracle pipeline from the float64 one on these
    inputs (measured inside the test) + the op-local bound (K + 2) * 2^-24 * sum|h||x| of the resampler divided by the row's std.
    Measured on an MI355X (this batch, crop at [0, 1200, 100, 0, 0]), worst over rows, fp32 oracle vs float64 / device vs float64 /
    op-local term: 44.1 kHz rows 2.129e-06 / 1.356e-06 / 2.009e-04; 48 kHz rows 2.268e-06 / 2.356e-06 / 5.499e-05; the 16 kHz rows
    (copied through, no op-local term) 3.340e-07 / 4.289e-07 / 0."""
    from oracle import data_oracle as DO
    from oracle import demucs_oracle as O
    from sehip import ops
    from sehip.data import DeviceBatcher
    items, rates = _items(), [r for _, r in UTTS]
    sl, starts = 1500, [0, 1200, 100, 0, 0]

    def pipeline(dtype):
        proc = []
        for (m, s, _), r, st in zip(items, rates, starts):
            m, s = O.resample_frac(m.to(dtype), r, 16000), O.resample_frac(s.to(dtype), r, 16000)
            m, s = DO.normalise(m, s, "z-score")
            proc.append(tuple(DO.crop([m, s], sl, st)))
        return DO.collate(proc, SEG, True)

    bm64, bs64, idx = pipeline(torch.float64)
    bm32, bs32, _ = pipeline(torch.float32)
    got = DeviceBatcher(CFG, normalize="z-score", sample_length=sl, drop_last=True)(items, starts=starts, rates=rates)
    assert got[5] == idx == [1, 1, 1, 1, 1]
    assert tuple(got[0].shape) == tuple(bm64.shape) and tuple(got[1].shape) == tuple(bs64.shape)
    # per raw row (mixture channel c, source s channel c of utterance g; segment g of this batch IS utterance g): the resampler's
    # op-local bound relative to the row's std, the deviation of the fp32 oracle pipeline, and the device's
    worst = {}
    for g_, ((m, s, _), r) in enumerate(zip(items, rates)):
        table, width, old, new = ops.resample_kernels(r, 16000) if r != 16000 else (None, 0, 1, 1)
        rows = [("mixture", (g_, c), m[c]) for c in range(2)] + [("sources", (g_, k, c), s[k, c]) for k in range(2) for c in range(2)]
        for name, at, row in rows:
            op_term = 0.0
            if table is not None:
                y64, mag = _formula64(row.double().numpy(), table.double().numpy(), old, new, width)
                op_term = float(((2 * width + old + 2) * 2.0 ** -24 * mag).max() / y64.std(ddof=1))
            t64, t32, dev_t = ((bm64, bm32, got[0]) if name == "mixture" else (bs64, bs32, got[1]))
            oracle_dev = float((t32[at].double() - t64[at]).abs().max())
            device_dev = float((dev_t[at].cpu().double() - t64[at]).abs().max())
            gate = 2.0 * oracle_dev + op_term
            w = worst.setdefault(r, [0.0, 0.0, 0.0])
            worst[r] = [max(w[0], oracle_dev), max(w[1], device_dev), max(w[2], op_term)]
            assert device_dev <= gate, (name, at, r, device_dev, oracle_dev, op_term)
    for r, (o_, d_, t_) in sorted(worst.items()):
        print(f"[resample batch] rate {r}: worst over rows: fp32 oracle vs float64 {o_:.3e}, device vs float64 {d_:.3e}, op-local term {t_:.3e}")
    m0 = O.resample_frac(items[1][0].double(), 44100, 16000)
    assert float((got[2][1]["mean"].cpu().double() - m0.mean(-1, keepdim=True)).abs().max()) < 1e-6
    assert float((got[2][1]["std"].cpu().double() - m0.std(-1, keepdim=True)).abs().max()) < 1e-6
