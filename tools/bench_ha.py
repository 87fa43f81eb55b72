#!/usr/bin/env python3
"""Times the hearing-aid stage on one GPU and writes profiles/ha.json.

  amplify_torch on [4, 1, 2, 264600] at 44.1 kHz (nfir 220, the compressor settings of the reference's src/ha/conf/config.yaml):
  time per call with the calls queued back to back, the per-kernel split (FIR, compressor, their backward entries, each queued
  back to back on its own), and the same 8 rows through the vectorised float64 CPU path of tests/ha_ref.py (prefix-sum level,
  blocked recurrence) on this machine's host.

The reference itself is not read here.  Its wall time for the same call on a CPU-only host is measured by
`tools/gen_golden_ha.py --time` and handed over with --reference-cpu-seconds; it is stored under `reference_on_cpu_only_host_s`.
Run:  python tools/bench_ha.py [--calls 20] [--reference-cpu-seconds S] [--out profiles/ha.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "speech-enhancement-pytorch_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ha_ref as R  # noqa: E402
from sehip import _lib  # noqa: E402
from sehip.audio import amplify_torch  # noqa: E402
from sehip.ha import CompressorTorch, NALRTorch, compress_rows, fir_adjoint, fir_apply  # noqa: E402

SHAPE, FS, NFIR = (4, 1, 2, 264600), 44100, 220


def timed(fn, calls):
    """mean milliseconds of fn() over `calls` calls queued back to back (after 3 warm-up calls)"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reference-cpu-seconds", type=float, default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ha.json"))
    args = ap.parse_args()
    _lib.call("sehip_check_device", 0)
    amp, comp = NALRTorch(NFIR, FS), CompressorTorch(fs=FS, **R.CHAIN["compressor"])
    rng = np.random.RandomState(3)
    t = np.arange(SHAPE[-1]) / FS
    x_host = (0.05 * rng.standard_normal(SHAPE) * (0.5 + 0.5 * np.sin(2 * np.pi * 3 * t)) ** 2).astype(np.float32)
    x = torch.from_numpy(x_host).cuda()
    rows, n = x.reshape(-1, SHAPE[-1]), SHAPE[-1]
    taps = amp.build_on(R.CHAIN["audiogram"]["audiogram_levels_l"], R.CHAIN["audiogram"]["audiogram_cfs"], x.device).reshape(1, -1).flip(-1).contiguous()
    res = {"shape": list(SHAPE), "fs": FS, "nfir": NFIR, "compressor": R.CHAIN["compressor"], "calls": args.calls,
           "device": torch.cuda.get_device_name(0)}
    res["amplify_torch_ms"] = timed(lambda: amplify_torch(x, amp, comp, R.CHAIN["audiogram"]), args.calls)
    y = fir_apply(rows, taps)
    res["fir_fwd_ms"] = timed(lambda: fir_apply(rows, taps), args.calls)
    res["fir_kernel"] = _lib.lib().sehip_last_kernel().decode()
    res["compressor_fwd_ms"] = timed(lambda: compress_rows(y, comp, soft_clip=True), args.calls)
    res["compressor_kernel"] = _lib.lib().sehip_last_kernel().decode()
    xg = x.clone().requires_grad_(True)
    G = torch.randn(SHAPE[:-1] + (n + NFIR,), device=x.device)

    def step():
        out = amplify_torch(xg, amp, comp, R.CHAIN["audiogram"])
        torch.autograd.grad(out, xg, G)

    res["amplify_torch_fwd_bwd_ms"] = timed(step, args.calls)
    res["fir_adj_ms"] = timed(lambda: fir_adjoint(G.reshape(-1, n + NFIR), taps, n), args.calls)
    # the CPU path of tests/ha_ref.py, vectorised, float64, same rows
    cfg = R.compressor_config(FS, **R.CHAIN["compressor"])
    t0 = time.perf_counter()
    st = R.chain(x_host.reshape(-1, n), taps.cpu().double().numpy().reshape(-1), cfg, soft_clip=True, loop=False, direct_level=False)
    res["ha_ref_vectorised_cpu_s"] = time.perf_counter() - t0
    res["ha_ref_vectorised_cpu_threads"] = torch.get_num_threads()
    out = amplify_torch(x, amp, comp, R.CHAIN["audiogram"]).reshape(-1, n + NFIR).double().cpu().numpy()
    res["max_abs_diff_to_ha_ref"] = float(np.abs(out - st["out"]).max())
    res["level_margin"] = R.margin(st["level"], cfg["threshold"])
    if args.reference_cpu_seconds is not None:
        res["reference_on_cpu_only_host_s"] = args.reference_cpu_seconds
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
