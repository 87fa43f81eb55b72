#!/usr/bin/env python3
"""Solver step time of ConvTasNet at the C4 shape ([32, 1, 32000], N128 L40 B128 H256 P3 X7 R2, SI-SNR, Adam, clip 5) for the four
variants causal in (False, True) x norm_type in ('gLN', 'cLN'), in ONE process.

The variants are timed in alternating rounds (default, cLN, causal gLN, causal cLN, default again, ...), every round device-
synchronised at both ends, after a warm-up of every variant; the default variant appears twice per cycle, so the spread of its
own repeats is in the result next to the differences between variants.  Every step starts from the same seeded weights (as
bench.py does).  One JSON document on stdout and, with --out, in a file:

    python tools/bench_ctn_variants.py --rounds 6 --steps 50 --warmup 20 --out profiles/ctn_variants_step.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "speech-enhancement-pytorch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

ORDER = ["default", "cln", "causal_gln", "causal_cln", "default_again"]
OPTIONS = {"default": dict(causal=False, norm_type="gLN"), "cln": dict(causal=False, norm_type="cLN"),
           "causal_gln": dict(causal=True, norm_type="gLN"), "causal_cln": dict(causal=True, norm_type="cLN"),
           "default_again": dict(causal=False, norm_type="gLN")}


def build(options, batch, n):
    import bench
    from sehip import distrib
    from sehip.solver import Solver, ScalarLog
    cfg = bench.convtasnet_config()
    for k, v in options.items():
        setattr(cfg.model, k, v)
    torch.manual_seed(cfg.seed)
    model = distrib.get_model(cfg.model)
    opt = distrib.get_optimizer(cfg.optim, model)
    solver = Solver(cfg, model, opt, distrib.get_loss_function(cfg.optim), device="gpu", writer=ScalarLog())
    noisy, clean = bench.workload_batch("convtasnet", batch, 0, solver.device)
    mixture, sources = solver._prepare_batch(noisy, clean)
    params0 = model.flat_params.detach().clone()

    def step():
        model.flat_params.copy_(params0)
        return solver.train_step(mixture, sources)

    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=50, help="steps per variant and round")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    steps = {tag: build(OPTIONS[tag], args.batch, 32000) for tag in ORDER}
    for tag in ORDER:
        for _ in range(args.warmup):
            loss, _m = steps[tag]()
        torch.cuda.synchronize()
        assert float(loss) == float(loss), tag
    ms = {tag: [] for tag in ORDER}
    for _ in range(args.rounds):
        for tag in ORDER:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                steps[tag]()
            torch.cuda.synchronize()
            ms[tag].append((time.perf_counter() - t0) / args.steps * 1e3)
    out = {"what": "ConvTasNet Solver step at the C4 shape, ms per step; one entry per round, rounds of the variants alternated in one process",
           "device": torch.cuda.get_device_name(0), "batch": args.batch, "samples": 32000, "rounds": args.rounds, "steps_per_round": args.steps,
           "warmup_steps": args.warmup, "ms_per_step": {t: [round(v, 4) for v in ms[t]] for t in ORDER},
           "median_ms": {t: round(statistics.median(ms[t]), 4) for t in ORDER}}
    d = out["median_ms"]
    out["default_repeat_spread_ms"] = round(abs(d["default"] - d["default_again"]), 4)
    out["relative_to_default"] = {t: round(d[t] / d["default"], 4) for t in ORDER}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
