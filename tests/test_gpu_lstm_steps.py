"""GPU: the recurrent kernels (csrc/lstm.hip: sehip_lstm_fwd/_bwd, the _chunk entry points, sehip_rlstm_fwd/_bwd; csrc/lstm2.hip:
sehip_lstm2_fwd/_bwd) driven directly through the C ABI with synthetic operands, EVERY time step against float64 arithmetic on the
operands the kernel itself read at that step (tests/lstm_steps_ref.py): the stored h[t-1] and c[t-1], the gate records, the stored
dpre[t+1].  Nothing compounds, so every stored bf16 element must be ONE rounding of the float64 result and every fp32 cell state within
fp32 evaluation noise -- a step that read a ring register before its load landed, a wrong step at a prefetch-distance boundary or a
chunk seam, a clamped row leaking into a real one or a stale granule moves a few elements of a few steps and fails here, where the
whole-sequence norm gates (tests/test_gpu_ops_local.py, test_gpu_shapes.py) let the recurrence damp it.  That the gates notice such
faults is shown without a card by tests/test_lstm_steps_host.py, which also sets the mismatch cap.

Shapes: ragged batch tiles (B = 1, 2, 3, 5, 6, 17 with 4 rows per workgroup) and T below, at and just above the prefetch distance (8)
and the layer-2 lag.  Every output and record buffer is a window in a larger tensor between two sentinel bands that must come back
unchanged; the windows themselves start as NaN patterns, so an element the kernel did not write fails its gate.  (h and dpre have
exactly B rows: "row B" of an output is the start of the band behind it, or the next combo's row 0, which the float64 gate covers.)"""
import pytest
import torch

import lstm_steps_ref as R

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
BAND = 1024                                     # sentinel elements on each side (a multiple of the kernels' 16-byte accesses)
SENT = {BF: 0x7FA5, F32: 0x7FA5A5A5}            # NaN patterns
INT = {BF: torch.int16, F32: torch.int32}


@pytest.fixture(scope="module")
def dev():
    from sehip import _lib
    assert torch.cuda.is_available()
    _lib.call("sehip_check_device", 0)
    return torch.device("cuda:0")


class Window:
    """n elements between two sentinel bands"""

    def __init__(self, n, dtype, dev):
        self.raw = torch.full((n + 2 * BAND,), SENT[dtype], dtype=INT[dtype], device=dev)
        self.t = self.raw[BAND:BAND + n].view(dtype)
        self.n = n

    @property
    def ptr(self):
        return self.t.data_ptr()

    def bands_intact(self):
        v = SENT[self.t.dtype]
        return bool((self.raw[:BAND] == v).all()) and bool((self.raw[BAND + self.n:] == v).all())

    def cpu(self):
        return self.t.cpu()


class Bufs(dict):
    def add(self, name, n, dtype, dev):
        self[name] = Window(n, dtype, dev)
        return self[name]

    def check_bands(self, what):
        torch.cuda.synchronize()
        broken = [k for k, w in self.items() if not w.bands_intact()]
        assert not broken, f"{what}: wrote outside {broken}"


def up(t, dev):
    return t.contiguous().to(dev)


def tiles(B):
    return (B + R.NBT - 1) // R.NBT


def report(fig):
    for line in fig.lines():
        print(line)
    bad = fig.violations()
    assert not bad, "\n".join(bad)


def padded_rows_repeat_the_last(recs, B):
    """the rows a ragged tile pads with are clamped to row B - 1: their records are that row's, bit for bit"""
    for r in recs:
        if r.shape[1] > B:
            assert torch.equal(r[:, B:], r[:, B - 1:B].expand_as(r[:, B:])), "a clamped row differs from row B - 1"


# ---- one complex layer / one plain nn.LSTM: csrc/lstm.hip -----------------------------------------------------------------------------
def lstm_buffers(d, dev, real):
    B, T, H = d["B"], d["T"], d["H"]
    C = 1 if real else 4
    bufs = Bufs()
    bufs.add("h", C * B * T * H, BF, dev)
    bufs.add("gates", C * tiles(B) * T * 4 * H * 4, BF, dev)
    bufs.add("c", C * tiles(B) * T * 4 * H, F32, dev)
    for k in (("dpre",) if real else ("dpre_r", "dpre_i")):
        bufs.add(k, B * T * (4 if real else 8) * H, BF, dev)
    g = {k: up(d[k], dev) for k in d if torch.is_tensor(d[k])}
    g["whhT"] = up(d["whh"].transpose(1, 2), dev)
    return bufs, g


def lstm_forward(d, bufs, g, real, ranges=None):
    from sehip import _lib
    B, T, H = d["B"], d["T"], d["H"]
    if real:
        _lib.call("sehip_rlstm_fwd", _lib.ptr(g["pre"]), _lib.ptr(g["whh"]), B, T, H, bufs["h"].ptr, bufs["gates"].ptr, bufs["c"].ptr, _lib.stream())
    elif ranges is None:
        _lib.call("sehip_lstm_fwd", _lib.ptr(g["pre_r"]), _lib.ptr(g["pre_i"]), _lib.ptr(g["whh"]), B, T, H, bufs["h"].ptr, bufs["gates"].ptr,
                  bufs["c"].ptr, _lib.stream())
    else:
        for t0, t1 in ranges:
            _lib.call("sehip_lstm_fwd_chunk", _lib.ptr(g["pre_r"]), _lib.ptr(g["pre_i"]), _lib.ptr(g["whh"]), B, T, H, t0, t1, bufs["h"].ptr,
                      bufs["gates"].ptr, bufs["c"].ptr, _lib.stream())
    bufs.check_bands("forward")


def lstm_backward(d, bufs, g, real, ranges=None):
    from sehip import _lib
    B, T, H = d["B"], d["T"], d["H"]
    if real:
        _lib.call("sehip_rlstm_bwd", _lib.ptr(g["dh_a"]), _lib.ptr(g["whhT"]), bufs["gates"].ptr, bufs["c"].ptr, B, T, H, bufs["dpre"].ptr, _lib.stream())
    elif ranges is None:
        _lib.call("sehip_lstm_bwd", _lib.ptr(g["dh_a"]), _lib.ptr(g["dh_b"]), _lib.ptr(g["whhT"]), bufs["gates"].ptr, bufs["c"].ptr, B, T, H,
                  bufs["dpre_r"].ptr, bufs["dpre_i"].ptr, _lib.stream())
    else:
        state = bufs.add("state", 4 * tiles(B) * 4 * H * 2, F32, g["whh"].device)
        for t0, t1 in reversed(ranges):
            _lib.call("sehip_lstm_bwd_chunk", _lib.ptr(g["dh_a"]), _lib.ptr(g["dh_b"]), _lib.ptr(g["whhT"]), bufs["gates"].ptr, bufs["c"].ptr, B, T, H,
                      t0, t1, state.ptr, bufs["dpre_r"].ptr, bufs["dpre_i"].ptr, _lib.stream())
    bufs.check_bands("backward")


def lstm_gate(d, bufs, real, label):
    """decode what the kernels stored and put every step under the float64 gate"""
    B, T, H = d["B"], d["T"], d["H"]
    C = 1 if real else 4
    h = bufs["h"].cpu().view(C, B, T, H)
    gates_p = R.decode_records(bufs["gates"].cpu(), C, B, T, H, width=4, padded=True)
    c_p = R.decode_records(bufs["c"].cpu(), C, B, T, H, padded=True)[..., 0]
    padded_rows_repeat_the_last((gates_p.view(torch.int16), c_p.view(torch.int32)), B)
    gates, c = gates_p[:, :B], c_p[:, :B]
    if real:
        pre, whh, dh, dpre = d["pre"][None], d["whh"], d["dh_a"][None], bufs["dpre"].cpu().view(1, B, T, 4 * H)
    else:
        pre, whh = R.combo_split(d["pre_r"], d["pre_i"], H), R.combo_weights(d["whh"])
        dh = R.combo_dh(d["dh_a"].double(), d["dh_b"].double())
        dpre = R.combo_split(bufs["dpre_r"].cpu().view(B, T, 8 * H), bufs["dpre_i"].cpu().view(B, T, 8 * H), H)
    fig = R.Figures(label)
    R.check_fwd(fig, "", pre, whh, h, gates, c)
    R.check_bwd(fig, "", gates, c, dh, whh, dpre)
    report(fig)


@pytest.mark.parametrize("n,case", list(enumerate(R.lstm_cases())), ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_complex_layer_every_step(dev, n, case):
    B, T, H, scale = case
    d = R.make_inputs(B, T, H, 100 + n, hh_scale=scale)
    bufs, g = lstm_buffers(d, dev, real=False)
    lstm_forward(d, bufs, g, False)
    lstm_backward(d, bufs, g, False)
    lstm_gate(d, bufs, False, f"lstm B={B} T={T} H={H} x{scale:g}")


@pytest.mark.parametrize("n,case", list(enumerate(R.rlstm_cases())), ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_plain_lstm_every_step(dev, n, case):
    B, T, H, scale = case
    d = R.make_inputs(B, T, H, 200 + n, hh_scale=scale, real=True)
    bufs, g = lstm_buffers(d, dev, real=True)
    lstm_forward(d, bufs, g, True)
    lstm_backward(d, bufs, g, True)
    lstm_gate(d, bufs, True, f"rlstm B={B} T={T} H={H} x{scale:g}")


CHUNKED = [(5, 17, [(0, 1), (1, 8), (8, 9), (9, 17)]), (3, 23, [(0, 7), (7, 14), (14, 21), (21, 23)])]


@pytest.mark.parametrize("B,T,ranges", CHUNKED, ids=["5x17-seams-1-8-9", "3x23-chunk-7"])
def test_chunked_calls_equal_the_whole_sequence_and_pass_every_step(dev, B, T, ranges):
    """forward chunk by chunk (a chunk resumes from the h / c records of the one before), backward in the reverse order through the
    `state` buffer: bit-equal to the whole-sequence calls, and under the float64 gate themselves -- the seams t0 - 1 -> t0 are steps
    like any other there"""
    H = 64
    d = R.make_inputs(B, T, H, 400 + B)
    whole, g = lstm_buffers(d, dev, real=False)
    lstm_forward(d, whole, g, False)
    lstm_backward(d, whole, g, False)
    parts, _ = lstm_buffers(d, dev, real=False)
    lstm_forward(d, parts, g, False, ranges)
    lstm_backward(d, parts, g, False, ranges)
    for k in ("h", "gates", "c", "dpre_r", "dpre_i"):
        assert torch.equal(whole[k].raw, parts[k].raw), f"{k}: the chunked calls differ from the whole-sequence call"
    lstm_gate(d, parts, False, f"lstm chunks B={B} T={T}")


# ---- the two stacked layers in one launch per direction: csrc/lstm2.hip ---------------------------------------------------------------
class Handoff:
    """granule arrays (zeroed ONCE) and the sync block of the fused launches"""

    def __init__(self, shapes, dev):
        from sehip import _lib
        lib = _lib.lib()
        self.fwd = torch.zeros(max(int(lib.sehip_lstm2_gran_bytes(b, t, 0)) for b, t in shapes) // 8, dtype=torch.int64, device=dev)
        self.bwd = torch.zeros(max(int(lib.sehip_lstm2_gran_bytes(b, t, 1)) for b, t in shapes) // 8, dtype=torch.int64, device=dev)
        self.sync = torch.zeros(int(lib.sehip_lstm2_sync_bytes()) // 4, dtype=torch.int32, device=dev)


def lstm2_run_and_gate(d, hand, epoch, dev, label):
    from sehip import _lib
    B, T, H = d["B"], d["T"], d["H"]
    bufs = Bufs()
    for layer in "12":
        bufs.add("h" + layer, 4 * B * T * H, BF, dev)
        bufs.add("gates" + layer, 4 * tiles(B) * T * 4 * H * 4, BF, dev)
        bufs.add("c" + layer, 4 * tiles(B) * T * 4 * H, F32, dev)
        bufs.add(f"dpre{layer}_r", B * T * 8 * H, BF, dev)
        bufs.add(f"dpre{layer}_i", B * T * 8 * H, BF, dev)
    g = {k: up(d[k], dev) for k in d if torch.is_tensor(d[k])}
    for k in ("whh", "whh2", "wih2"):
        g[k + "T"] = up(d[k].transpose(1, 2), dev)
    p = _lib.ptr
    _lib.call("sehip_lstm2_fwd", p(g["pre_r"]), p(g["pre_i"]), p(g["whh"]), p(g["whh2"]), p(g["wih2"]), p(g["bias2"]), B, T, H,
              bufs["h1"].ptr, bufs["gates1"].ptr, bufs["c1"].ptr, bufs["h2"].ptr, bufs["gates2"].ptr, bufs["c2"].ptr, p(hand.fwd), p(hand.sync),
              epoch, _lib.stream())
    bufs.check_bands("lstm2 forward")
    assert int(hand.sync[0]) == 0, "a forward hand-off wait timed out"
    _lib.call("sehip_lstm2_bwd", p(g["dh_a"]), p(g["dh_b"]), p(g["whhT"]), p(g["whh2T"]), p(g["wih2T"]), bufs["gates1"].ptr, bufs["c1"].ptr,
              bufs["gates2"].ptr, bufs["c2"].ptr, B, T, H, bufs["dpre1_r"].ptr, bufs["dpre1_i"].ptr, bufs["dpre2_r"].ptr, bufs["dpre2_i"].ptr,
              p(hand.bwd), p(hand.sync), epoch, _lib.stream())
    bufs.check_bands("lstm2 backward")
    assert int(hand.sync[0]) == 0, "a backward hand-off wait timed out"
    rec = {}
    for layer in "12":
        rec["h" + layer] = bufs["h" + layer].cpu().view(4, B, T, H)
        gp = R.decode_records(bufs["gates" + layer].cpu(), 4, B, T, H, width=4, padded=True)
        cp = R.decode_records(bufs["c" + layer].cpu(), 4, B, T, H, padded=True)[..., 0]
        padded_rows_repeat_the_last((gp.view(torch.int16), cp.view(torch.int32)), B)
        rec["gates" + layer], rec["c" + layer] = gp[:, :B], cp[:, :B]
        rec["dpre" + layer] = R.combo_split(bufs[f"dpre{layer}_r"].cpu().view(B, T, 8 * H), bufs[f"dpre{layer}_i"].cpu().view(B, T, 8 * H), H)
    fig = R.Figures(label)
    R.check_lstm2_fwd(fig, R.combo_split(d["pre_r"], d["pre_i"], H), d["whh"], d["whh2"], d["wih2"], d["bias2"], rec["h1"], rec["gates1"],
                      rec["c1"], rec["h2"], rec["gates2"], rec["c2"])
    R.check_lstm2_bwd(fig, d["dh_a"], d["dh_b"], d["whh"], d["whh2"], d["wih2"], rec["gates1"], rec["c1"], rec["gates2"], rec["c2"],
                      rec["dpre1"], rec["dpre2"])
    report(fig)


@pytest.mark.parametrize("n,case", list(enumerate(R.lstm2_cases())), ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_fused_layers_every_step_twice_on_the_same_granules(dev, n, case):
    """two calls with different epochs AND different operands on the same granule arrays: the second call reads slots the first
    wrote, so a step that accepted a stale granule would carry the first call's h1 / input-gradient partial"""
    B, T, H, scale = case
    hand = Handoff([(B, T)], dev)
    for rep in range(2):
        d = R.make_inputs(B, T, H, 300 + 2 * n + rep, hh_scale=scale, layers=2)
        lstm2_run_and_gate(d, hand, 1 + rep, dev, f"lstm2 B={B} T={T} x{scale:g} epoch {1 + rep}")


def test_fused_layers_two_geometries_on_one_granule_array(dev):
    """(5, 9) at epoch 1, then (3, 13) at epoch 2 on one shared, larger granule array: the slots of the second geometry overlay the
    first's differently, every one of them holds a tag of the earlier epoch"""
    hand = Handoff([(5, 9), (3, 13)], dev)
    for epoch, (B, T) in ((1, (5, 9)), (2, (3, 13))):
        d = R.make_inputs(B, T, 64, 500 + epoch, layers=2)
        lstm2_run_and_gate(d, hand, epoch, dev, f"lstm2 shared granules B={B} T={T} epoch {epoch}")
