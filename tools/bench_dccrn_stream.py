#!/usr/bin/env python3
"""Time per chunk of sehip.model.DCCRNStreamer at the shipped widths (kernel_num 16 32 64 128 256 256, rnn_units 128, two LSTM layers,
400 / 100 frames) for S in 1 / 8 / 64 streams and Kc in 1 / 4 / 16 hops per chunk, eager and graphed, with the launches per chunk, and
the offline eval forward of the same hops on the same box in the same run beside it.

    python tools/bench_dccrn_stream.py --out profiles/dccrn_stream.json

The parent process opens no GPU: every (S, Kc) cell runs in a child of its own (`--cell S KC`) under a time limit, and the first cell
that fails or runs out of time ends the run (nothing more is started on the device after it).  In a cell the calls are queued back
to back -- the same chunk fed `frames / Kc` times, which is one pass over a signal of `frames` hops per stream -- and timed with a host
clock between two device synchronisations, after a warm-up pass of the same length; `repeats` passes each, the median reported.
Recorded, not asserted: whether a chunk is computed faster than the audio it serves (Kc * win_inc / 16000 s per chunk).  Not measured:
a per-kernel table (no profiler run is made here).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "speech-enhancement-pytorch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

STREAMS, CHUNKS = (1, 8, 64), (1, 4, 16)


def cell(S, Kc, frames, repeats):
    import torch
    from sehip.model import DCCRN, DCCRNStreamer
    torch.manual_seed(0)
    model = DCCRN(length=frames * 100).cuda().eval()
    hop = model.win_inc
    n = frames // Kc
    g = torch.Generator().manual_seed(1)
    x = (0.1 * torch.randn(S, 1, Kc * hop, generator=g)).cuda()
    whole = (0.1 * torch.randn(S, 1, frames * hop, generator=g)).cuda()

    def timed(run):
        run()                                   # warm-up: the same pass
        torch.cuda.synchronize()
        ms = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ms)

    audio_ms = Kc * hop / 16.0
    out = {"streams": S, "chunk_frames": Kc, "chunks_per_pass": n, "chunk_ms_of_audio_at_16k": audio_ms}
    for tag, graph in (("eager", False), ("graph", True)):
        st = DCCRNStreamer(model, streams=S, chunk_frames=Kc, graph=graph)

        def run():
            for _ in range(n):
                st.feed(x)

        ms = timed(run) / n
        out[tag + "_ms_per_chunk"] = round(ms, 5)
        out[tag + "_faster_than_audio"] = bool(ms < audio_ms)
        assert bool(torch.isfinite(st.flush()).all())
    out["launches_per_chunk"] = st.launches
    with torch.no_grad():
        off = timed(lambda: model(whole))
    out["offline_eval_forward_ms"] = round(off, 5)
    out["offline_ms_per_chunk_equivalent"] = round(off / n, 5)
    out["delay_samples"] = st.delay
    out["state_bytes"] = st.state_bytes
    out["device"] = torch.cuda.get_device_name(0)
    print("CELL " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cell", nargs=2, type=int, default=None, metavar=("S", "KC"))
    ap.add_argument("--frames", type=int, default=160, help="hops per stream in one timed pass (a multiple of every Kc)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--limit", type=int, default=120, help="seconds a cell may take")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.cell:
        cell(args.cell[0], args.cell[1], args.frames, args.repeats)
        return
    cells = []
    for S in STREAMS:
        for Kc in CHUNKS:
            cmd = [sys.executable, os.path.abspath(__file__), "--cell", str(S), str(Kc), "--frames", str(args.frames), "--repeats", str(args.repeats)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
            except subprocess.TimeoutExpired:
                sys.exit(f"cell S={S} Kc={Kc} ran out of its {args.limit} s: stopping")
            line = next((ln for ln in r.stdout.splitlines() if ln.startswith("CELL ")), None)
            if r.returncode != 0 or line is None:
                sys.exit(f"cell S={S} Kc={Kc} failed with status {r.returncode}: stopping\n{r.stderr[-2000:]}")
            cells.append(json.loads(line[5:]))
            print(line, flush=True)
    doc = {"what": "DCCRNStreamer, shipped widths, 400 / 100 frames: ms per chunk (median of the passes; calls queued back to back), eager "
                   "and graphed, launches per chunk, whether a chunk is computed faster than the audio it serves (recorded, not asserted), "
                   "and the offline eval forward over the same hops in the same run",
           "not_measured": "no per-kernel table: no profiler run was made",
           "frames_per_pass": args.frames, "repeats": args.repeats, "cells": cells}
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    else:
        print(text)


if __name__ == "__main__":
    main()
