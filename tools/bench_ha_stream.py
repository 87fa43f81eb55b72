#!/usr/bin/env python3
"""Time per chunk of sehip.ha.AmplifyStreamer at the Clarity settings (44.1 kHz, nfir 220, compressor window W = 8820, tanh) for S in
1 / 8 / 64 streams and chunks of 32 / 64 / 256 / 4096 samples, eager and graphed, with the chunk's own audio duration and the offline
amplify_torch over the same total samples beside it.

    python tools/bench_ha_stream.py --out profiles/ha_stream.json

The method is tools/bench_ctn_stream.py's (tools/stream_bench.py): every (S, C) cell in a child process of its own under a time limit;
in a cell the same chunk is fed `--frames` times back to back (here --frames counts CHUNKS per pass, 400 by default), timed with a host
clock between two device synchronisations after a warm-up pass of the same length; `repeats` passes, the median reported.
"""
import json

from stream_bench import main, timed

STREAMS, CHUNKS = (1, 8, 64), (32, 64, 256, 4096)
FS, NFIR = 44100, 220
AUDIOGRAM = {"audiogram_cfs": [250, 500, 1000, 2000, 3000, 4000, 6000, 8000], "audiogram_levels_l": [25, 40, 55, 65, 65, 70, 65, 60],
             "audiogram_levels_r": [20, 30, 55, 65, 65, 75, 60, 50]}


def cell(S, C, chunks, repeats):
    import torch
    from sehip.audio import amplify_torch
    from sehip.ha import AmplifyStreamer, CompressorTorch, NALRTorch
    amp, comp = NALRTorch(NFIR, FS), CompressorTorch(fs=FS)
    assert comp.win_len == 8820
    g = torch.Generator().manual_seed(1)
    x = (0.05 * torch.randn(S, 2, C, generator=g)).cuda()
    whole = (0.05 * torch.randn(S, 1, 2, chunks * C, generator=g)).cuda()

    out = {"streams": S, "chunk_samples": C, "chunks_per_pass": chunks, "chunk_ms_of_audio": round(C / (FS / 1e3), 5)}
    for tag, graph in (("eager", False), ("graph", True)):
        st = AmplifyStreamer(amp, comp, AUDIOGRAM, streams=S, chunk_samples=C, graph=graph)

        def run():
            for _ in range(chunks):
                st.feed(x)

        out[tag + "_ms_per_chunk"] = round(timed(run, repeats) / chunks, 5)
        assert bool(torch.isfinite(st.flush()).all())
    with torch.no_grad():
        off = timed(lambda: amplify_torch(whole, amp, comp, AUDIOGRAM), repeats)
    out["offline_amplify_ms"] = round(off, 5)
    out["offline_ms_per_chunk_equivalent"] = round(off / chunks, 5)
    out["slower_than_its_audio"] = bool(max(out["eager_ms_per_chunk"], out["graph_ms_per_chunk"]) > out["chunk_ms_of_audio"])
    out["launches"], out["state_bytes"] = st.launches, st.state_bytes
    out["device"] = torch.cuda.get_device_name(0)
    print("CELL " + json.dumps(out))


DOC = {"what": "AmplifyStreamer, 44.1 kHz, nfir 220, W 8820, soft_clip: ms per chunk (median of the passes; calls queued back to back), "
               "eager and graphed, the chunk's audio duration, and offline amplify_torch over the same total samples.  frames_per_pass "
               "counts chunks here"}


if __name__ == "__main__":
    main(__file__, cell, STREAMS, CHUNKS, 400, DOC)
