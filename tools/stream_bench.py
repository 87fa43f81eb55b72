"""What the streamer benches share (tools/bench_ctn_stream.py, tools/bench_dccrn_stream.py): the timing loop of a cell, the command line,
the parent loop over the cells and the JSON writer.

The parent process opens no GPU: every (S, Kc) cell runs in a child of its own (`--cell S KC`) under a time limit, and the first cell
that fails or runs out of time ends the run (nothing more is started on the device after it).
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


def timed(run, repeats):
    """median host time of run() in ms between two device synchronisations, after a warm-up pass of the same length"""
    import torch
    run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms)


def main(script, cell, streams, chunks, frames, doc):
    """The command line of the bench `script`: `--cell S KC` runs cell(S, Kc, frames, repeats), which prints one "CELL {json}" line;
    without it, every cell of streams x chunks in a child, collected behind the head `doc` and written to --out (or printed)."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--cell", nargs=2, type=int, default=None, metavar=("S", "KC"))
    ap.add_argument("--frames", type=int, default=frames, help="hops per stream in one timed pass (a multiple of every Kc)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--limit", type=int, default=120, help="seconds a cell may take")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.cell:
        cell(args.cell[0], args.cell[1], args.frames, args.repeats)
        return
    cells = []
    for S in streams:
        for Kc in chunks:
            cmd = [sys.executable, os.path.abspath(script), "--cell", str(S), str(Kc), "--frames", str(args.frames), "--repeats", str(args.repeats)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
            except subprocess.TimeoutExpired:
                sys.exit(f"cell S={S} Kc={Kc} ran out of its {args.limit} s: stopping")
            line = next((ln for ln in r.stdout.splitlines() if ln.startswith("CELL ")), None)
            if r.returncode != 0 or line is None:
                sys.exit(f"cell S={S} Kc={Kc} failed with status {r.returncode}: stopping\n{r.stderr[-2000:]}")
            cells.append(json.loads(line[5:]))
            print(line, flush=True)
    text = json.dumps(dict(doc, frames_per_pass=args.frames, repeats=args.repeats, cells=cells), indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    else:
        print(text)
