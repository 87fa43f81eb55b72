#!/usr/bin/env python3
"""Time of the device resampler (csrc/resample.hip through sehip.ops.resample_rows) on the data path's batch: 16 utterances x 6 rows
(a stereo mixture and two stereo sources) x 6 s, read at 44.1 kHz and at 48 kHz, resampled to 16 kHz.

The rows are on the device before the clock starts (the H2D copy of the raw batch exists with and without the resampler).  A
repetition is --inner calls enqueued back to back between ONE pair of device events, divided by --inner: the time per call with
the launches queued behind each other, so the host's share of a single call (table lookup, ctypes, launch latency) stays out as
long as the host enqueues faster than the device runs.  The two batches are visited in alternating rounds after a warm-up of
each; the report gives the median over all repetitions, the 10th / 90th percentile and the spread of the round medians.  Next
to it: the time oracle.demucs_oracle.resample_frac (the float32 CPU restatement of julius.resample_frac) takes for the same batch on this host with --threads threads; the bytes the kernel has to move (rows in, rows out, the table once) over
its time against the HBM roof; its multiply-adds over its time against the fp32 vector peak.  A run without a GPU fails.

    python tools/bench_resample.py --out profiles/resample.json
"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (HERE, os.path.join(HERE, "speech-enhancement-pytorch_amd")):
    sys.path.insert(0, p)

UTTERANCES, ROWS_PER_UTTERANCE, SECONDS, TARGET = 16, 6, 6, 16000
RATES = (44100, 48000)
HBM_PEAK_BYTES_PER_S = 8.0e12        # MI355X HBM3E, spec
FP32_PEAK_FLOP_PER_S = 157.3e12      # MI355X fp32 vector (= fp32 matrix) peak, spec


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(q * len(v)))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=40, help="timed repetitions per batch and round")
    ap.add_argument("--inner", type=int, default=10, help="calls between one pair of events")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--threads", type=int, default=16, help="CPU threads of the oracle's run")
    ap.add_argument("--cpu-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from oracle import demucs_oracle as O
    from sehip import _lib, ops
    if not torch.cuda.is_available():
        raise SystemExit("bench_resample: no GPU; a time measured anywhere else says nothing about this path")
    dev = torch.device("cuda:0")
    rows = UTTERANCES * ROWS_PER_UTTERANCE
    cases = {}
    for rate in RATES:
        n = rate * SECONDS
        g = torch.Generator().manual_seed(rate)
        host = 0.1 * torch.randn(rows, n, generator=g)
        raw = host.reshape(-1).to(dev)
        off = torch.arange(rows + 1, dtype=torch.int64) * n
        m = ops.resample_out_len(n, rate, TARGET)
        out = torch.empty(rows * m, dtype=torch.float32, device=dev)
        out_off = (torch.arange(rows + 1, dtype=torch.int64) * m).to(dev)
        cases[rate] = dict(host=host, raw=raw, off=off.to(dev), n=n, m=m, out=out, out_off=out_off)

    def run(rate):
        c = cases[rate]
        ops.resample_rows(c["raw"], c["off"], rows, rate, TARGET, c["out"], c["out_off"])

    kernel = {}
    for rate in RATES:
        for _ in range(args.warmup):
            run(rate)
        torch.cuda.synchronize()
        kernel[rate] = _lib.lib().sehip_last_kernel().decode()
    us = {rate: [[] for _ in range(args.rounds)] for rate in RATES}
    for r in range(args.rounds):
        for rate in RATES:
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.inner):
                    run(rate)
                e1.record()
                e1.synchronize()
                us[rate][r].append(e0.elapsed_time(e1) * 1e3 / args.inner)
    torch.set_num_threads(args.threads)
    results = {}
    for rate in RATES:
        c = cases[rate]
        table, width, old, new = ops.resample_kernels(rate, TARGET)
        taps = 2 * width + old
        ref = O.resample_frac(c["host"], rate, TARGET)           # (also the oracle's warm-up)
        cpu_s = []
        for _ in range(args.cpu_reps):
            t0 = time.perf_counter()
            O.resample_frac(c["host"], rate, TARGET)
            cpu_s.append(time.perf_counter() - t0)
        dev_y = c["out"].view(rows, c["m"]).cpu()
        flat = [v for rr in us[rate] for v in rr]
        rmed = [statistics.median(rr) for rr in us[rate]]
        med = statistics.median(flat)
        nbytes = 4 * (rows * c["n"] + rows * c["m"] + table.numel())
        macs = rows * c["m"] * taps
        results[f"{rate}_to_{TARGET}"] = {
            "rows": rows, "samples_in_per_row": c["n"], "samples_out_per_row": c["m"], "ratio": [old, new], "taps": taps,
            "table_bytes": 4 * table.numel(), "kernel": kernel[rate],
            "median_us": round(med, 2), "p10_us": round(pct(flat, 0.10), 2), "p90_us": round(pct(flat, 0.90), 2),
            "round_medians_us": [round(v, 2) for v in rmed], "spread_us": round(max(rmed) - min(rmed), 2),
            "bytes_moved": nbytes, "bytes_per_s": round(nbytes / (med * 1e-6), 0),
            "share_of_hbm_peak": round(nbytes / (med * 1e-6) / HBM_PEAK_BYTES_PER_S, 4),
            "macs": macs, "flop_per_s": round(2 * macs / (med * 1e-6), 0),
            "share_of_fp32_peak": round(2 * macs / (med * 1e-6) / FP32_PEAK_FLOP_PER_S, 4),
            "bound_by": "fp32 rate" if 2 * macs / FP32_PEAK_FLOP_PER_S > nbytes / HBM_PEAK_BYTES_PER_S else "HBM",
            "cpu_oracle_threads": args.threads, "cpu_oracle_median_s": round(statistics.median(cpu_s), 4),
            "cpu_oracle_over_device": round(statistics.median(cpu_s) / (med * 1e-6), 1),
            "max_abs_diff_to_cpu_oracle": float((dev_y - ref).abs().max()),
        }
    doc = {"what": "csrc/resample.hip, one call per batch of 16 utterances x 6 rows x 6 s; microseconds per call, `calls_per_event_pair` calls "
                   "enqueued back to back between two device events; batches alternated in rounds; CPU figure: oracle.demucs_oracle.resample_frac on the same batch, same host",
           "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "reps_per_round": args.reps, "warmup_calls": args.warmup,
           "calls_per_event_pair": args.inner, "hbm_peak_bytes_per_s": HBM_PEAK_BYTES_PER_S, "fp32_peak_flop_per_s": FP32_PEAK_FLOP_PER_S,
           "results": results}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
