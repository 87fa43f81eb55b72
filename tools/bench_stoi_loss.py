#!/usr/bin/env python3
"""Times sehip.loss.StoiLoss forward + backward on one GPU and writes profiles/stoi_loss.json.

  [32, 1, 32000] at 16 kHz (a training batch of 2-second segments) and [4, 2, 264600] at 44.1 kHz (6-second clips, two speakers), STOI and
  ESTOI: milliseconds per forward + backward with the calls queued back to back between two device events (after warm-up calls), eager
  and as the replay of one captured graph.  In the same run, beside them: the metric's forward alone (sehip.metric.STOI) on the same
  input, and loss_sisdr forward + backward on the first shape.  The launches per call are counted from the code, not measured; per-kernel
  times are not measured.

Nothing is promised about these times: the file records what was measured.
Run:  python tools/bench_stoi_loss.py [--calls 2000] [--out profiles/stoi_loss.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "speech-enhancement-pytorch_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import stoi_ref as R  # noqa: E402
from sehip import _lib  # noqa: E402
from sehip.loss import StoiLoss, loss_sisdr  # noqa: E402
from sehip.metric import STOI  # noqa: E402

CASES = (("batch_32x32000_16k", (32, 1, 32000), 16000), ("clips_4x2x264600_44k1", (4, 2, 264600), 44100))
# library launches of one call off 10 kHz: resample, levels, select, bands, segments, finalize (+ one torch negation) forward;
# segments, gather, bands, inverse, compact, resampler adjoint backward.  At 10 kHz both resampler launches drop out.
LAUNCHES = {"forward_library": 6, "forward_torch": 1, "backward_library": 6}


def timed(fn, calls):
    """mean milliseconds of fn() over `calls` calls queued back to back (after 5 warm-up calls)"""
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def eager_and_graph(loss_fn, x, y_host, calls):
    """(eager ms, graph-replay ms, value) of loss_fn(y, x) forward + backward with respect to y"""
    unit = torch.ones((), device=x.device)
    y = y_host.cuda().requires_grad_(True)

    def step():
        return torch.autograd.grad(loss_fn(y, x), y, unit)[0]
    eager = timed(step, calls)
    del y
    torch.cuda.synchronize()
    y_s = y_host.cuda().requires_grad_(True)                 # first used inside the capture
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        loss = loss_fn(y_s, x)
        torch.autograd.grad(loss, y_s, unit)
    return eager, timed(g.replay, calls), float(loss.detach())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stoi_loss.json"))
    args = ap.parse_args()
    _lib.call("sehip_check_device", 0)
    res = {"calls": args.calls, "device": torch.cuda.get_device_name(0), "launches_per_call": LAUNCHES,
           "not_measured": "per-kernel times", "cases": {}}
    for i, (name, shape, sr) in enumerate(CASES):
        rows, n = int(np.prod(shape[:-1])), shape[-1]
        clean = np.stack([R.am_signal(n, sr, seed=100 + r) for r in range(rows)]).astype(np.float32)
        noisy = clean + 0.03 * np.random.RandomState(7).randn(rows, n).astype(np.float32)
        x, y_host = torch.from_numpy(clean).cuda().reshape(shape), torch.from_numpy(noisy).reshape(shape)
        case = {"shape": list(shape), "sr": sr}
        for ext in (False, True):
            tag = "estoi" if ext else "stoi"
            e, g, v = eager_and_graph(StoiLoss(sr=sr, extended=ext), x, y_host, args.calls)
            case[f"{tag}_loss_fwd_bwd_eager_ms"], case[f"{tag}_loss_fwd_bwd_graph_ms"], case[f"{tag}_loss_value"] = e, g, v
            y = y_host.cuda()
            case[f"{tag}_metric_fwd_eager_ms"] = timed(lambda: STOI(x, y, sr=sr, extended=ext), args.calls)
        if i == 0:
            e, g, v = eager_and_graph(loss_sisdr, x, y_host, args.calls)
            case["sisdr_loss_fwd_bwd_eager_ms"], case["sisdr_loss_fwd_bwd_graph_ms"], case["sisdr_loss_value"] = e, g, v
        res["cases"][name] = case
        print(name, json.dumps(case))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
