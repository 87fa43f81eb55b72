#!/usr/bin/env python3
"""Time per chunk of sehip.model.DCCRNStreamer at the shipped widths (kernel_num 16 32 64 128 256 256, rnn_units 128, two LSTM layers,
400 / 100 frames) for S in 1 / 8 / 64 streams and Kc in 1 / 4 / 16 hops per chunk, eager and graphed, with the launches per chunk, and
the offline eval forward of the same hops on the same box in the same run beside it.

    python tools/bench_dccrn_stream.py --out profiles/dccrn_stream.json

Every (S, Kc) cell runs in a child process of its own under a time limit (tools/stream_bench.py).  In a cell the calls are queued back
to back -- the same chunk fed `frames / Kc` times, which is one pass over a signal of `frames` hops per stream -- and timed with a host
clock between two device synchronisations, after a warm-up pass of the same length; `repeats` passes each, the median reported.
Recorded, not asserted: whether a chunk is computed faster than the audio it serves (Kc * win_inc / 16000 s per chunk).  Not measured:
a per-kernel table (no profiler run is made here).
"""
import json

from stream_bench import main, timed

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

    audio_ms = Kc * hop / 16.0
    out = {"streams": S, "chunk_frames": Kc, "chunks_per_pass": n, "chunk_ms_of_audio_at_16k": audio_ms}
    for tag, graph in (("eager", False), ("graph", True)):
        st = DCCRNStreamer(model, streams=S, chunk_frames=Kc, graph=graph)

        def run():
            for _ in range(n):
                st.feed(x)

        ms = timed(run, repeats) / n
        out[tag + "_ms_per_chunk"] = round(ms, 5)
        out[tag + "_faster_than_audio"] = bool(ms < audio_ms)
        assert bool(torch.isfinite(st.flush()).all())
    out["launches_per_chunk"] = st.launches
    with torch.no_grad():
        off = timed(lambda: model(whole), repeats)
    out["offline_eval_forward_ms"] = round(off, 5)
    out["offline_ms_per_chunk_equivalent"] = round(off / n, 5)
    out["delay_samples"] = st.delay
    out["state_bytes"] = st.state_bytes
    out["device"] = torch.cuda.get_device_name(0)
    print("CELL " + json.dumps(out))


DOC = {"what": "DCCRNStreamer, shipped widths, 400 / 100 frames: ms per chunk (median of the passes; calls queued back to back), eager "
               "and graphed, launches per chunk, whether a chunk is computed faster than the audio it serves (recorded, not asserted), "
               "and the offline eval forward over the same hops in the same run",
       "not_measured": "no per-kernel table: no profiler run was made"}


if __name__ == "__main__":
    main(__file__, cell, STREAMS, CHUNKS, 160, DOC)
