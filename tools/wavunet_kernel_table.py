#!/usr/bin/env python3
"""Per-kernel table of one `rocprofv3 --kernel-trace --stats` run of tools/bench_wavunet.py: time per step of every kernel and, for the
streaming kernels of csrc/wavunet.hip, the bytes the algorithm moves per step (from the shapes: every operand read once, every result
written once, bf16 activations) over that time.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/bench_wavunet.py --rounds 1 --steps 5 --warmup 2 --cpu-batch 0
    python tools/wavunet_kernel_table.py DIR 7 [--batch 32 --samples 16384 --layers 12 --interval 24]      # 7 = warm-up + timed steps
"""
import argparse
import csv
import glob


def bytes_per_step(B, T, n, ci):
    enc = [(B * (T >> l), (l + 1) * ci) for l in range(n)]                                   # (rows, channels) of encoder layer l
    mid = (B * (T >> n), n * ci)
    dec = [(B * (T >> (n - 1 - i)), (n - i) * ci) for i in range(n)]
    el = lambda rc: rc[0] * rc[1]
    ups = [mid] + dec[:-1]                                                                   # the tensors the interpolation reads
    bt = B * T
    return {
        "wun_enc0_fwd_kernel": 4 * bt + 2 * el(enc[0]),
        "wun_enc0_wgrad_kernel": 4 * bt + 2 * el(enc[0]),
        "wun_bn_stats_kernel": 2 * sum(map(el, enc + [mid] + dec)),
        "wun_bn_apply_kernel": 4 * (sum(map(el, enc)) + el(dec[-1])),
        "wun_bn_apply_up2_kernel": 6 * sum(map(el, ups)),
        "wun_up2_bwd_kernel": 6 * sum(map(el, ups)),
        "wun_bn_bwd_reduce_kernel": 5 * sum(map(el, enc)) + 4 * sum(map(el, [mid] + dec)),
        "wun_bn_bwd_apply_kernel": 7 * sum(map(el, enc)) + 6 * sum(map(el, [mid] + dec)),
        "wun_out_fwd_kernel": 8 * bt + 2 * el(dec[-1]),
        "wun_out_bwd_kernel": 12 * bt + 4 * el(dec[-1]),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("steps", type=int)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--samples", type=int, default=16384)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--interval", type=int, default=24)
    ap.add_argument("--top", type=int, default=40)
    a = ap.parse_args()
    rows = list(csv.DictReader(open(glob.glob(f"{a.dir}/**/*kernel_stats.csv", recursive=True)[0])))
    moved = bytes_per_step(a.batch, a.samples, a.layers, a.interval)
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    print(f"{'kernel':56s} {'calls/step':>10s} {'us/step':>9s} {'avg us':>8s} {'share':>6s} {'MB/step':>9s} {'GB/s':>7s}")
    for r in rows[:a.top]:
        name = r["Name"].split("(")[0].replace("void ", "")
        us = float(r["TotalDurationNs"]) / 1e3 / a.steps
        mb = moved.get(name.split("<")[0])
        tail = f" {mb / 1e6:9.1f} {mb / 1e3 / us:7.0f}" if mb else ""
        print(f"{name[:56]:56s} {int(r['Calls']) / a.steps:10.1f} {us:9.1f} {float(r['AverageNs']) / 1e3:8.1f} {float(r['Percentage']):5.1f}%{tail}")
    print(f"GPU-busy ms per step: {total / 1e6 / a.steps:.3f}")


if __name__ == "__main__":
    main()
