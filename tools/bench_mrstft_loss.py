#!/usr/bin/env python3
"""Times sehip.loss.MRSTFTLoss on one GPU and writes profiles/mrstft_loss.json.

  [32, 1, 32000] (a training batch of 2-second segments at 16 kHz) and [16, 2, 96000] (6-second clips, two speakers), the default
  resolutions: milliseconds per forward alone and per forward + backward, the calls queued back to back between two device events (after
  warm-up calls at that shape), eager and as the replay of one captured graph.  In the same run, alternating with it in rounds: the
  restatement tests/mrstft_ref.py in float32 on the GPU (stock torch.stft + autograd), and loss_sisdr and l1_loss forward + backward at
  the same shape.  The workspace bytes per shape are recorded; the launches per call are counted from the code, not measured; per-kernel
  times are not measured.

The hand-written path has no reason to exist if it is slower than the stock one: the run FAILS (exit status 1, after the file is written)
if its eager forward + backward is slower than the stock one timed in this run.
Run:  python tools/bench_mrstft_loss.py [--calls 300] [--rounds 3] [--out profiles/mrstft_loss.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "speech-enhancement-pytorch_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mrstft_ref as MR  # noqa: E402
from sehip import _lib  # noqa: E402
from sehip.loss import MRSTFTLoss, l1_loss, loss_sisdr  # noqa: E402

CASES = (("batch_32x1x32000", (32, 1, 32000)), ("clips_16x2x96000", (16, 2, 96000)))
# library launches of one call at R resolutions: R forward + 1 finalize (+ one torch copy of the result); R backward + R gather
LAUNCHES = {"forward_library": "R + 1", "forward_torch": 1, "backward_library": "2 R", "R": len(MR.RESOLUTIONS)}


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


def stock(y, x):
    return MR.loss(y.reshape(-1, y.shape[-1]), x.reshape(-1, x.shape[-1]))


def graphed(loss_fn, x, y_host, backward):
    """the replay of one captured forward (+ backward) of loss_fn(y, x)"""
    unit = torch.ones((), device=x.device)
    y_s = y_host.cuda().requires_grad_(True)                 # first used inside the capture
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        loss = loss_fn(y_s, x)
        if backward:
            torch.autograd.grad(loss, y_s, unit)
    return g, (y_s, loss)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mrstft_loss.json"))
    args = ap.parse_args()
    _lib.call("sehip_check_device", 0)
    res = {"calls": args.calls, "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "resolutions": [list(r) for r in MR.RESOLUTIONS],
           "launches_per_call": LAUNCHES, "times": "milliseconds per call, the median of the rounds; every round's value under *_rounds",
           "not_measured": "per-kernel times (a kernel trace is a run of its own: DESIGN.md section 21)", "cases": {}}
    slower = []
    for name, shape in CASES:
        g = torch.Generator().manual_seed(7)
        clean = 0.1 * torch.randn(shape, generator=g)
        y_host = clean + 0.05 * torch.randn(shape, generator=g)
        x = clean.cuda()
        unit = torch.ones((), device=x.device)
        mod = MRSTFTLoss()
        y = y_host.cuda().requires_grad_(True)
        fns = {
            "hip_fwd_eager_ms": lambda: mod(y.detach(), x),
            "hip_fwd_bwd_eager_ms": lambda: torch.autograd.grad(mod(y, x), y, unit),
            "stock_fwd_eager_ms": lambda: stock(y.detach(), x),
            "stock_fwd_bwd_eager_ms": lambda: torch.autograd.grad(stock(y, x), y, unit),
            "sisdr_fwd_bwd_eager_ms": lambda: torch.autograd.grad(loss_sisdr(y, x), y, unit),
            "l1_fwd_bwd_eager_ms": lambda: torch.autograd.grad(l1_loss(y, x), y, unit),
        }
        value, stock_value = float(mod(y, x).detach()), float(stock(y, x).detach())
        torch.cuda.synchronize()
        keep = []
        for tag, fn, bwd in (("hip_fwd_graph_ms", MRSTFTLoss(), False), ("hip_fwd_bwd_graph_ms", MRSTFTLoss(), True)):
            graph, held = graphed(fn, x, y_host, bwd)
            keep.append((fn, held))
            fns[tag] = graph.replay
        rounds = {k: [] for k in fns}
        for _ in range(args.rounds):                          # alternating: a drift of the machine falls on every path alike
            for k, fn in fns.items():
                rounds[k].append(timed(fn, args.calls))
        case = {"shape": list(shape), "loss_value": value, "stock_loss_value": stock_value,
                "workspace_bytes": mod.workspace(shape, x.device).nbytes()}
        for k, v in rounds.items():
            case[k] = sorted(v)[len(v) // 2]
            case[k + "_rounds"] = v
        case["stock_over_hip_fwd_bwd_eager"] = case["stock_fwd_bwd_eager_ms"] / case["hip_fwd_bwd_eager_ms"]
        if case["hip_fwd_bwd_eager_ms"] > case["stock_fwd_bwd_eager_ms"]:
            slower.append(name)
        res["cases"][name] = case
        print(name, json.dumps(case))
        del keep
    res["hip_not_slower_than_stock"] = not slower
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    if slower:
        print(f"FAIL: the hand-written forward + backward is slower than stock torch.stft + autograd at {slower}", file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
