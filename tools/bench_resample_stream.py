#!/usr/bin/env python3
"""Time per chunk of sehip.ResampleStreamer for S in 1 / 8 / 64 streams (one channel), the ratios 44100 -> 16000, 16000 -> 44100,
48000 -> 16000 and 16000 -> 48000 and chunks of 10 ms and 50 ms of audio, eager and graphed, with the chunk's own audio duration and the
only way to stream without the streamer beside it: torch.cat of the last H samples (rounded up to whole frames) and the chunk,
ops.resample_frac on that buffer, and a slice (whose edges are not the stream's: the offline kernel replicate-pads whatever it is given).

    python tools/bench_resample_stream.py --out profiles/resample_stream.json

Every S runs in a child process of its own under a time limit (the parent opens no GPU; the first child that fails ends the run).  In a
cell the three paths ALTERNATE in rounds: a round feeds the same chunk `--chunks` times back to back on each path, timed with a pair of
device events; rounds go on until the timed windows of the cell add up to `--window` seconds (one second by default) after one untimed
warm-up round.  The median over the rounds is reported per path.  There is no fallback: without a GPU the tool fails."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "speech-enhancement-pytorch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

STREAMS = (1, 8, 64)
RATIOS = ((44100, 16000), (16000, 44100), (48000, 16000), (16000, 48000))
CHUNK_MS = (10, 50)


def cell(S, old_sr, new_sr, ms, chunks, window):
    import torch
    from sehip import ResampleStreamer, ops
    probe = ResampleStreamer(old_sr, new_sr, streams=1, chunk_frames=1)
    old, new, dq, H = probe.in_block, probe.out_block, probe.delay_frames, probe.history
    n = old_sr * ms // 1000
    assert n % old == 0, (old_sr, ms, old)
    C = n // old
    g = torch.Generator().manual_seed(1)
    x = (0.1 * torch.randn(S, 1, n, generator=g)).cuda()
    eager = ResampleStreamer(old_sr, new_sr, streams=S, chunk_frames=C)
    graph = ResampleStreamer(old_sr, new_sr, streams=S, chunk_frames=C, graph=True)
    hist_frames = -(-H // old)
    state = {"hist": torch.zeros(S, 1, hist_frames * old, device="cuda")}
    lo = (hist_frames - dq) * new

    def baseline():
        buf = torch.cat((state["hist"], x), -1)
        y = ops.resample_frac(buf, old_sr, new_sr)[..., lo:lo + C * new]
        state["hist"] = buf[..., n:]
        return y

    paths = (("eager", lambda: eager.feed(x)), ("graph", lambda: graph.feed(x)), ("cat_offline_slice", baseline))
    ms_of = {k: [] for k, _ in paths}
    total, rounds = 0.0, 0
    while rounds == 0 or total < window * 1e3 or rounds < 4:
        for name, step in paths:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(chunks):
                y = step()
            b.record()
            b.synchronize()
            if rounds:                                            # (round 0 warms up: captures, table uploads, allocator)
                t = a.elapsed_time(b)
                ms_of[name].append(t / chunks)
                total += t
        rounds += 1
    assert tuple(y.shape) == (S, 1, C * new) and bool(torch.isfinite(eager.flush()).all()) and bool(torch.isfinite(graph.flush()).all())
    out = {"streams": S, "ratio": f"{old_sr}->{new_sr}", "chunk_ms_of_audio": ms, "chunk_frames": C, "chunk_in": n, "chunk_out": C * new,
           "chunks_per_round": chunks, "timed_rounds": rounds - 1, "timed_window_ms": round(total, 1)}
    for name, _ in paths:
        out[name + "_ms_per_chunk"] = round(statistics.median(ms_of[name]), 5)
    out["slower_than_its_audio"] = bool(max(out["eager_ms_per_chunk"], out["graph_ms_per_chunk"]) > ms)
    out["launches"], out["state_bytes"], out["delay_samples"] = graph.launches, graph.state_bytes, graph.delay
    out["device"] = torch.cuda.get_device_name(0)
    print("CELL " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=None, help="(the child's) run the cells of this S")
    ap.add_argument("--chunks", type=int, default=200, help="chunks per path in one round")
    ap.add_argument("--window", type=float, default=1.0, help="seconds of timed windows per cell")
    ap.add_argument("--limit", type=int, default=300, help="seconds the cells of one S may take")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.streams is not None:
        for old_sr, new_sr in RATIOS:
            for ms in CHUNK_MS:
                cell(args.streams, old_sr, new_sr, ms, args.chunks, args.window)
        return
    cells = []
    for S in STREAMS:
        cmd = [sys.executable, os.path.abspath(__file__), "--streams", str(S), "--chunks", str(args.chunks), "--window", str(args.window)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            sys.exit(f"S={S} ran out of its {args.limit} s: stopping")
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("CELL ")]
        if r.returncode != 0 or len(lines) != len(RATIOS) * len(CHUNK_MS):
            sys.exit(f"S={S} failed with status {r.returncode}: stopping\n{r.stderr[-2000:]}")
        for ln in lines:
            cells.append(json.loads(ln[5:]))
            print(ln, flush=True)
    doc = {"what": "ResampleStreamer, one channel: ms per chunk (median over the rounds; calls queued back to back, device events), eager and "
                   "graphed, the chunk's audio duration, and cat(history, chunk) + ops.resample_frac + slice timed in the same rounds",
           "chunks_per_round": args.chunks, "window_s": args.window, "cells": cells}
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    else:
        print(text)


if __name__ == "__main__":
    main()
