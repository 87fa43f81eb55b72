#!/usr/bin/env python3
"""Time per chunk of sehip.model.ConvTasNetStreamer at the C4 widths (causal=True, norm_type='cLN'; N128 L40 B128 H256 P3 X7 R2,
one audio channel, 2 sources) for S in 1 / 8 / 64 streams and Kc in 1 / 8 / 32 frames per chunk, eager and graphed, with the offline
forward over the same total signal beside it as the baseline.

    python tools/bench_ctn_stream.py --out profiles/ctn_stream.json

Every (S, Kc) cell runs in a child process of its own under a time limit (tools/stream_bench.py).  In a cell the calls are queued back
to back -- the same chunk fed `frames / Kc` times, which is one pass over a signal of `frames` hops per stream -- and timed with a host
clock between two device synchronisations, after a warm-up pass of the same length; `repeats` passes each, the median reported.
"""
import json

from stream_bench import main, timed

STREAMS, CHUNKS = (1, 8, 64), (1, 8, 32)


def cell(S, Kc, frames, repeats):
    import torch
    from sehip.model import ConvTasNet, ConvTasNetStreamer
    torch.manual_seed(0)
    model = ConvTasNet(sources=["s0", "s1"], audio_channels=1, causal=True, norm_type="cLN").cuda().eval()
    h = model.L // 2
    n = frames // Kc
    g = torch.Generator().manual_seed(1)
    x = (0.3 * torch.randn(S, 1, Kc * h, generator=g)).cuda()
    whole = (0.3 * torch.randn(S, 1, (frames + 1) * h, generator=g)).cuda()

    out = {"streams": S, "chunk_frames": Kc, "chunks_per_pass": n, "chunk_ms_of_audio_at_16k": Kc * h / 16.0}
    for tag, graph in (("eager", False), ("graph", True)):
        st = ConvTasNetStreamer(model, streams=S, chunk_frames=Kc, graph=graph)

        def run():
            for _ in range(n):
                st.feed(x)

        out[tag + "_ms_per_chunk"] = round(timed(run, repeats) / n, 5)
        assert bool(torch.isfinite(st.flush()).all())
    with torch.no_grad():
        off = timed(lambda: model(whole), repeats)
    out["offline_forward_ms"] = round(off, 5)
    out["offline_ms_per_chunk_equivalent"] = round(off / n, 5)
    out["state_bytes"] = st.state_bytes
    out["device"] = torch.cuda.get_device_name(0)
    print("CELL " + json.dumps(out))


DOC = {"what": "ConvTasNetStreamer, C4 widths, causal cLN: ms per chunk (median of the passes; calls queued back to back), eager and "
               "graphed, and the offline forward over the same total signal"}


if __name__ == "__main__":
    main(__file__, cell, STREAMS, CHUNKS, 640, DOC)
