#!/usr/bin/env python3
"""Times sehip.loss.PitMRSTFTLoss on one GPU and writes profiles/mrstft_pit.json.

  [32, 2, 1, 32000] (the Conv-TasNet training batch: 2-second segments at 16 kHz, two speakers) and [16, 4, 2, 96000] (6-second clips,
  four speakers, two channels), the default resolutions, wave_l1 = 1 ('pit-l1+mrstft'): milliseconds per forward alone and per forward +
  backward, the calls queued back to back between two device events (after warm-up calls at that shape), eager and as the replay of one
  captured graph.  In the same run, alternating with it in rounds:
    (a) `composed`: the permutation-invariant loss put together from the plain pieces -- S * S mrstft_terms calls (+ the waveform L1 of
        each pair), the pair matrix read back, the permutation picked on the host, then S MRSTFTLoss modules (one each: they are live
        together) forward (+ backward) on the matched slices;
    (b) `plain`: MRSTFTLoss on the same tensors with the speakers in the given order, no PIT: the floor, the same 2 S transforms per
        row group and resolution;
    (c) `pit_l1`: pit_loss_pointwise l1 forward + backward.
  The workspace bytes per shape are recorded; per-kernel times are not measured.

The pair kernels have no reason to exist if they are slower than the composition: the run FAILS (exit status 1, after the file is written)
if the eager forward is not faster than (a)'s timed in this run.  The distance from (b) is reported, not gated.
Run:  python tools/bench_mrstft_pit.py [--calls 200] [--rounds 3] [--out profiles/mrstft_pit.json]"""
import argparse
import json
import os
import sys
from itertools import permutations

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "speech-enhancement-pytorch_amd"))

from sehip import _lib  # noqa: E402
from sehip.loss import MRSTFT_RESOLUTIONS, MRSTFTLoss, PitMRSTFTLoss, l1_loss, mrstft_terms, pit_loss_pointwise  # noqa: E402

CASES = (("batch_32x2x1x32000", (32, 2, 1, 32000)), ("clips_16x4x2x96000", (16, 4, 2, 96000)))
# library launches of one call at R resolutions and wave_l1 > 0: 2 (L1 pair matrix) + R forward + 1 select (+ two torch copies of the
# results); 1 (L1 backward) + R backward + R gather (+ one torch multiply of the upstream gradient)
LAUNCHES = {"forward_library": "R + 3", "forward_torch": 2, "backward_library": "2 R + 1", "backward_torch": 1, "R": len(MRSTFT_RESOLUTIONS)}
WAVE_L1 = 1.0


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


class Composed:
    """(a): what the plain pieces give.  The slices are made contiguous once, outside the timed region, for the targets; the estimates'
    slices are part of the call (they are the network's output)."""

    def __init__(self, S):
        self.S = S
        self.mods = [MRSTFTLoss(wave_l1=WAVE_L1) for _ in range(S)]

    def __call__(self, y, x_slices, backward, unit):
        S = self.S
        ys = [y[:, i].contiguous() for i in range(S)]
        with torch.no_grad():
            m = torch.stack([torch.stack([mrstft_terms(ys[i], x_slices[j]).sum(1).mean() + WAVE_L1 * l1_loss(ys[i], x_slices[j])
                                          for j in range(S)]) for i in range(S)]).cpu()
        best, lmin = None, 1e9
        for pe in permutations(range(S)):
            l = sum(float(m[pe[j], j]) for j in range(S))
            if lmin > l:
                best, lmin = pe, l
        loss = sum(self.mods[j](ys[best[j]], x_slices[j]) for j in range(S)) / S
        if backward:
            torch.autograd.grad(loss, y, unit)
        return loss, list(best)


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
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mrstft_pit.json"))
    args = ap.parse_args()
    _lib.call("sehip_check_device", 0)
    res = {"calls": args.calls, "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "resolutions": [list(r) for r in MRSTFT_RESOLUTIONS],
           "wave_l1": WAVE_L1, "launches_per_call": LAUNCHES,
           "times": "milliseconds per call, the median of the rounds; every round's value under *_rounds",
           "not_measured": "per-kernel times (a kernel trace is a run of its own)", "cases": {}}
    slower = []
    for name, shape in CASES:
        S = shape[1]
        g = torch.Generator().manual_seed(7)
        clean = 0.1 * torch.randn(shape, generator=g) * (1 + torch.arange(S, dtype=torch.float32)).reshape(1, S, *([1] * (len(shape) - 2)))
        order = [(i + 1) % S for i in range(S)]
        y_host = clean[:, order] + 0.05 * torch.randn(shape, generator=g)
        x = clean.cuda()
        x_slices = [x[:, j].contiguous() for j in range(S)]
        unit = torch.ones((), device=x.device)
        mod, plain, composed = PitMRSTFTLoss(wave_l1=WAVE_L1), MRSTFTLoss(wave_l1=WAVE_L1), Composed(S)
        y = y_host.cuda().requires_grad_(True)
        fns = {
            "pit_fwd_eager_ms": lambda: mod(y.detach(), x),
            "pit_fwd_bwd_eager_ms": lambda: torch.autograd.grad(mod(y, x), y, unit),
            "composed_fwd_eager_ms": lambda: composed(y.detach(), x_slices, False, unit),
            "composed_fwd_bwd_eager_ms": lambda: composed(y, x_slices, True, unit),
            "plain_fwd_eager_ms": lambda: plain(y.detach(), x),
            "plain_fwd_bwd_eager_ms": lambda: torch.autograd.grad(plain(y, x), y, unit),
            "pit_l1_fwd_bwd_eager_ms": lambda: torch.autograd.grad(pit_loss_pointwise(y, x, "l1"), y, unit),
        }
        loss, perm = mod(y, x, return_comb=True)
        c_loss, c_perm = composed(y, x_slices, False, unit)
        value, perm, c_value = float(loss.detach()), perm.tolist(), float(c_loss.detach())
        torch.cuda.synchronize()
        keep = []
        for tag, fn, bwd in (("pit_fwd_graph_ms", PitMRSTFTLoss(wave_l1=WAVE_L1), False),
                             ("pit_fwd_bwd_graph_ms", PitMRSTFTLoss(wave_l1=WAVE_L1), True)):
            fn.workspace(shape, x.device)                     # the buffers exist before the capture
            graph, held = graphed(fn, x, y_host, bwd)
            keep.append((fn, held))
            fns[tag] = graph.replay
        rounds = {k: [] for k in fns}
        for _ in range(args.rounds):                          # alternating: a drift of the machine falls on every path alike
            for k, fn in fns.items():
                rounds[k].append(timed(fn, args.calls))
        case = {"shape": list(shape), "loss_value": value, "perm": perm, "composed_loss_value": c_value, "composed_perm": c_perm,
                "workspace_bytes": mod.workspace(shape, x.device).nbytes(),
                "plain_workspace_bytes": plain.workspace(shape, x.device).nbytes()}
        for k, v in rounds.items():
            case[k] = sorted(v)[len(v) // 2]
            case[k + "_rounds"] = v
        case["composed_over_pit_fwd_eager"] = case["composed_fwd_eager_ms"] / case["pit_fwd_eager_ms"]
        case["composed_over_pit_fwd_bwd_eager"] = case["composed_fwd_bwd_eager_ms"] / case["pit_fwd_bwd_eager_ms"]
        case["pit_over_plain_fwd_eager"] = case["pit_fwd_eager_ms"] / case["plain_fwd_eager_ms"]
        case["pit_over_plain_fwd_bwd_eager"] = case["pit_fwd_bwd_eager_ms"] / case["plain_fwd_bwd_eager_ms"]
        if not case["pit_fwd_eager_ms"] < case["composed_fwd_eager_ms"] or perm != c_perm:
            slower.append(name)
        res["cases"][name] = case
        print(name, json.dumps(case), flush=True)
        del keep
    res["pit_forward_faster_than_composed"] = not slower
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    if slower:
        print(f"FAIL: the pair kernels' forward is not faster than the composition of the plain pieces (or picks another permutation) at {slower}",
              file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
