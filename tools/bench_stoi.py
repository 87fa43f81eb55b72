#!/usr/bin/env python3
"""Times sehip.metric.STOI on one GPU and writes profiles/stoi.json.

  [32, 1, 32000] at 16 kHz (a validation batch of 2-second segments) and [1, 1, 6 s] at 48 kHz and 44.1 kHz: milliseconds per call with
  the calls queued back to back between two device events (after warm-up calls, enough calls for a window of a good fraction of a
  second), eager and as the replay of one captured graph; beside them the wall time of tests/stoi_ref.py (float64 numpy, this machine's
  host) on the same input, and the deviation of the device's per-row values from that oracle.

Nothing is promised about these times: the file records what was measured.
Run:  python tools/bench_stoi.py [--calls 3000] [--out profiles/stoi.json]"""
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

import stoi_ref as R  # noqa: E402
from sehip import _lib  # noqa: E402
from sehip.metric import STOI, stoi_rows, stoi_workspace  # noqa: E402

CASES = (("batch_32x32000_16k", (32, 1, 32000), 16000), ("utt_6s_48k", (1, 1, 288000), 48000), ("utt_6s_44k1", (1, 1, 264600), 44100))


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=3000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stoi.json"))
    args = ap.parse_args()
    _lib.call("sehip_check_device", 0)
    res = {"calls": args.calls, "device": torch.cuda.get_device_name(0), "cpu_threads": torch.get_num_threads(), "cases": {}}
    for name, shape, sr in CASES:
        rows, n = shape[0] * shape[1], shape[-1]
        clean = np.stack([R.am_signal(n, sr, seed=100 + i) for i in range(rows)]).astype(np.float32)
        noisy = clean + 0.03 * np.random.RandomState(7).randn(rows, n).astype(np.float32)
        x, y = torch.from_numpy(clean).cuda().reshape(shape), torch.from_numpy(noisy).cuda().reshape(shape)
        case = {"shape": list(shape), "sr": sr}
        for ext in (False, True):
            tag = "estoi" if ext else "stoi"
            case[f"{tag}_eager_ms"] = timed(lambda: STOI(x, y, sr=sr, extended=ext), args.calls)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                out = STOI(x, y, sr=sr, extended=ext)
            case[f"{tag}_graph_ms"] = timed(g.replay, args.calls)
            case[f"{tag}_value"] = float(out)
        case["last_kernel"] = _lib.lib().sehip_last_kernel().decode()
        d = stoi_rows(x, y, sr=sr).double().cpu().numpy()
        t0 = time.perf_counter()
        ref = np.array([R.stoi(a, b, sr) for a, b in zip(clean, noisy)])
        case["stoi_ref_float64_cpu_s"] = time.perf_counter() - t0
        case["stoi_ref_float64_cpu_ms_per_row"] = 1e3 * case["stoi_ref_float64_cpu_s"] / rows
        case["max_abs_diff_to_stoi_ref"] = float(np.abs(d - ref).max())
        # band magnitudes of the first row against the oracle's, relative to the row's largest
        st = R.stoi_steps(clean[0], noisy[0], sr)
        tob = stoi_workspace(rows, n, sr, x.device)["tob"].double().cpu().numpy()
        case["band_magnitude_max_rel_diff_row0"] = max(
            float(np.abs(tob[s, 0, :, :st["T"]] - st[k]).max() / st[k].max()) for s, k in enumerate(("x_tob", "y_tob")))
        res["cases"][name] = case
        print(name, json.dumps(case))
    # the gate tests/test_gpu_stoi.py computes (8 x the float32 restatement's own deviation over that file's cases), for comparison
    import test_gpu_stoi as T
    res["test_gate_d"], res["test_gate_band_magnitudes"] = T.gates()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
