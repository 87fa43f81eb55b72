"""DCCRN at the HEADLINE WIDTHS (kernel_num 16 ... 256, rnn_units 128: the network bench.py times), EVERY product launch of one train
step -- sehip_gemm, sehip_gemm_pair, sehip_wgrad, sehip_wgrad_pair and the grouped LSTM weight gradients -- compared AT THE CALL with
float64 arithmetic on the operands the descriptor passed to that call points at (tests/desc_ref.py, proved against the oracle by
tests/test_desc_ref_host.py; the engine is tests/dccrn_products_worker.py).  The counterpart of tests/test_gpu_demucs_fullwidth.py, whose
constants are imported: a bf16 destination within ONE rounding of float64 `A W^T + bias (+ res)` element by element (rms 1.8e-3, max one
ulp), an fp32 destination and every fp32-accumulated weight gradient within 2e-5 -- the weight gradients also per (frame tap, row tap)
slice of K -- bias gradients within 1e-4, destination elements the descriptor does not address bit-identical to before the launch, the
packed weights bit-equal to bf16(+-params) through the plan's own pack entries (the w_tiled order un-done as include/sehip.h words it),
and the fused side outputs against float64 for the first time: the BatchNorm sums of the forward epilogues (`stats`) from the bf16
values the launch stored, the backward reduce sums of the streaming input gradients (`bnr_part`) and the weight gradient that computes
its dOut from bn_dz / bn_y (`bn_dz`), each fp32 sum within 4 * 2^-24 * sqrt(n) * sum |addend|.

Rounding points applied on the reference side (and nowhere else):
  * `res` on the two kernels that stage the product tile as bf16 and carry `res` here (dccrn_products_worker.RES_AFTER_BF16:
    conv_gemm_v3_pair_kernel, convt_stream_kernel): the product is rounded to bf16, the residual added to that and the sum rounded
    again -- two roundings by design, each half an ulp of its own value, so the element is held to one ulp of |product| + |sum|
    (desc_ref.out_err2), same constants.  Any other kernel that meets `res`, and a launch with `res` AND `stats` (conv_gemm_v3 adds
    `res` in fp32 before staging there), is held to the plain one-rounding gate;
  * `bn_dz`: narrow_wgrad_mfma_kernel<5, 2, true> evaluates its dOut in float32 and rounds it to bf16 before it multiplies (pack_bf2 in
    its stage step, as sehip_cbn_bwd_apply would have stored it).  The reference does the same -- the value as float32 arithmetic
    gives it, in the order of the kernel's source expression (desc_ref.bn_apply_f32), rounded to bf16 -- and the dW and dbias rules
    are applied to the plain difference with their constants.  (Rounding the float64 value instead leaves a handful of the 264 192
    elements on the other side of a bf16 tie, and one of them in a large row is 3e-5 of its tap slice.)

Five runs, because WHICH code runs depends on B and T (c3_pick_tm / the pair rule of csrc/conv3.hip pick 192- or 256-row tiles from
B * (T + 2); the streaming kernels of csrc/convt.hip give a workgroup ceil(T / min(32, T)) frames):
  A         B = 1, length 1300 (T = 16): one partly filled tile per conv_gemm_v3 launch, one frame per streaming workgroup
  B         B = 3, length 4000 (T = 43): ragged last tile, two-frame loop with a one-frame last workgroup, odd batch
  B-det     the same under sehip_set_deterministic(1): per-split weight-gradient arrays, statistics from the separate passes
  B-bn_dz   the same on the default schedule with the first layer's BatchNorm backward inside its weight gradient
            (plan.FUSE_ENC0_BN_WGRAD, off by default: the only way to reach the bn_dz operands)
  B-forced  the same in a fresh child process with SEHIP_C3_TM=8, SEHIP_C3_PAIR_TM=8, SEHIP_CT_CHUNKS=2, SEHIP_BNR_CHUNKS=2 (read once
            per process): the 256-row tile instantiations and a 22-frame loop per streaming workgroup that wraps the LDS ring several
            times -- the bench shape's code at a test's cost.
Each run also pins its dispatch: a literal table launch -> sehip_last_kernel string, so that a change that silently moves a layer onto
another kernel shows up here.  Reference math: src/model/dccrn.py:316-450 (ComplexConv2d / ComplexConvTranspose2d), :264-302 (the LSTM's
products), :457-634 (ComplexBatchNorm); that the descriptors ask for those convolutions is pinned by tests/test_host_plan.py and the
whole-chain oracle tests."""
import json
import os
import subprocess
import sys

import pytest

import dccrn_products_worker as W

pytestmark = pytest.mark.gpu

RUNS = {"A": dict(B=1, length=1300, T=16), "B": dict(B=3, length=4000, T=43), "B-det": dict(B=3, length=4000, T=43),
        "B-bn_dz": dict(B=3, length=4000, T=43), "B-forced": dict(B=3, length=4000, T=43)}
FORCED_ENV = {"SEHIP_C3_TM": "8", "SEHIP_C3_PAIR_TM": "8", "SEHIP_CT_CHUNKS": "2", "SEHIP_BNR_CHUNKS": "2"}
HERE = os.path.dirname(os.path.abspath(__file__))

# launch -> sehip_last_kernel, recorded from the first green run of each shape (template booleans print as 0 / 1).  Runs A and B take
# the same instantiations: B and T change the grids, the ragged tiles and the frames per workgroup, not the choice.
_DEFAULT = {
    "enc0.fwd": "convn_stream_kernel<16, 1, 1, 0>",
    "enc1.fwd": "convs_stream_kernel<16, 32, 64, 1, 1, 0>",
    "enc2.fwd": "convs_stream_kernel<32, 64, 32, 1, 1, 0>",
    "enc3.fwd": "conv_gemm_v3_kernel<5, 2, 16, 6, 4, 2, 0>",
    "enc4.fwd": "conv_gemm_v3_kernel<5, 2, 8, 6, 4, 2, 0>",
    "enc5.fwd": "conv_gemm_v3_kernel<5, 2, 4, 6, 4, 2, 0>",
    "ih1_r+ih1_i": "gemm_pair_kernel<128, 64, 2, 2>",
    "proj_r+proj_i": "gemm_pair_kernel<128, 64, 2, 2>",
    "dec0.fwd0+dec0.fwd1": "conv_gemm_v3_pair_kernel<4, 6, 4>",
    "dec1.fwd0+dec1.fwd1": "conv_gemm_v3_pair_kernel<8, 6, 4>",
    "dec2.fwd0+dec2.fwd1": "conv_gemm_v3_pair_kernel<16, 6, 2>",
    "dec3.fwd0+dec3.fwd1": "convt_stream_kernel<64, 2, 32, 32, 1, 0>",
    "dec4.fwd0+dec4.fwd1": "convt_stream_kernel<32, 2, 16, 64, 1, 0>",
    "dec5.fwd0+dec5.fwd1": "convt_stream_kernel<16, 2, 2, 128, 0, 0>",
    "dec5.fwd0.wg+dec5.fwd1.wg": "wgradt2_stream_kernel",
    "dec5.dg": "convn_stream_kernel<32, 2, 0, 1>",
    "dec4.fwd0.wg+dec4.fwd1.wg": "wgradt_stream_kernel<32, 16, 64>",
    "dec4.dg": "convs_stream_kernel<16, 64, 64, 2, 0, 1>",
    "dec3.fwd0.wg+dec3.fwd1.wg": "wgradt_stream_kernel<64, 32, 32>",
    "dec3.dg": "convs_stream_kernel<32, 128, 32, 2, 0, 0>",
    "dec2.fwd0.wg+dec2.fwd1.wg": "conv_wgrad_kernel<2>",
    "dec2.dg": "conv_gemm_v3_kernel<5, 2, 16, 6, 4, 2, 0>",
    "dec1.fwd0.wg+dec1.fwd1.wg": "conv_wgrad_kernel<2>",
    "dec1.dg": "conv_gemm_v3_kernel<5, 2, 8, 6, 4, 2, 0>",
    "dec0.fwd0.wg+dec0.fwd1.wg": "conv_wgrad_kernel<2>",
    "dec0.dg": "conv_gemm_v3_kernel<5, 2, 4, 6, 4, 2, 0>",
    "proj_r.wg": "wgrad_kernel<128, 2, 2, 1>",
    "proj_i.wg": "wgrad_kernel<128, 2, 2, 1>",
    "dproj_r+dproj_i": "gemm_pair_kernel<64, 64, 2, 2>",
    "lstm.wg[12]": "dense_tile_wgrad_kernel",
    "dx1_r+dx1_i": "gemm_pair_kernel<128, 64, 2, 2>",
    "enc5.fwd.wg": "conv_wgrad_v3_kernel<5, 2, 4, 2, 4>",
    "enc5.dg0+enc5.dg1": "conv_gemm_v3_pair_kernel<4, 6, 4>",
    "enc4.fwd.wg": "conv_wgrad_v3_kernel<5, 2, 8, 2, 4>",
    "enc4.dg0+enc4.dg1": "conv_gemm_v3_pair_kernel<8, 6, 4>",
    "enc3.fwd.wg": "conv_wgrad_v3_kernel<5, 2, 16, 2, 4>",
    "enc3.dg0+enc3.dg1": "conv_gemm_v3_pair_kernel<16, 6, 2>",
    "enc2.fwd.wg": "wgrads_stream_kernel<32, 64, 32>",
    "enc2.dg0+enc2.dg1": "convt_stream_kernel<64, 1, 32, 32, 0, 1>",
    "enc1.fwd.wg": "wgrads_stream_kernel<16, 32, 64>",
    "enc1.dg0+enc1.dg1": "convt_stream_kernel<32, 1, 16, 64, 0, 1>",
    "enc0.fwd.wg": "narrow_wgrad_mfma_kernel<5>",
}
DISPATCH = {
    "A": _DEFAULT,
    "B": _DEFAULT,
    "B-bn_dz": _DEFAULT,      # (sehip_last_kernel names narrow_wgrad_mfma_kernel by its tap count only, with and without bn_dz)
    # the deterministic schedule: no fused statistics (the forward streaming kernels exist only with them) and no atomics in the
    # weight gradients (the streaming and LDS-DMA weight-gradient kernels flush with atomics)
    "B-det": dict(_DEFAULT, **{
        "enc0.fwd": "conv_narrow_kernel<16, 4>",
        "enc1.fwd": "conv_small2_kernel<32, 6, 4>",
        "enc2.fwd": "conv_gemm_v3_kernel<5, 2, 32, 6, 2, 2, 0>",
        "dec3.fwd0+dec3.fwd1": "conv_small2_kernel<32, 12, 2, pair>",
        "dec4.fwd0+dec4.fwd1": "conv_small2_kernel<16, 12, 4, pair>",
        "dec5.fwd0.wg+dec5.fwd1.wg": "conv_small_wgrad_kernel<16, 2, 6>",
        "dec4.fwd0.wg+dec4.fwd1.wg": "conv_small_wgrad_kernel<16, 4, 12>",
        "dec3.fwd0.wg+dec3.fwd1.wg": "conv_small_wgrad_kernel<32, 8, 12>",
        "enc5.fwd.wg": "conv_wgrad_kernel<5>",
        "enc4.fwd.wg": "conv_wgrad_kernel<5>",
        "enc3.fwd.wg": "conv_wgrad_kernel<5>",
        "enc2.fwd.wg": "conv_small_wgrad_kernel<64, 5, 6>",
        "enc1.fwd.wg": "conv_small_wgrad_kernel<32, 3, 6>",
    }),
    # the 256-row tiles (TM = 8) of every conv_gemm_v3 launch; the streaming kernels keep their names (their frames per workgroup change)
    "B-forced": dict(_DEFAULT, **{
        "enc3.fwd": "conv_gemm_v3_kernel<5, 2, 16, 8, 4, 2, 0>",
        "enc4.fwd": "conv_gemm_v3_kernel<5, 2, 8, 8, 4, 2, 0>",
        "enc5.fwd": "conv_gemm_v3_kernel<5, 2, 4, 8, 4, 2, 0>",
        "dec0.fwd0+dec0.fwd1": "conv_gemm_v3_pair_kernel<4, 8, 4>",
        "dec1.fwd0+dec1.fwd1": "conv_gemm_v3_pair_kernel<8, 8, 4>",
        "dec2.fwd0+dec2.fwd1": "conv_gemm_v3_pair_kernel<16, 8, 2>",
        "dec2.dg": "conv_gemm_v3_kernel<5, 2, 16, 8, 4, 2, 0>",
        "dec1.dg": "conv_gemm_v3_kernel<5, 2, 8, 8, 4, 2, 0>",
        "dec0.dg": "conv_gemm_v3_kernel<5, 2, 4, 8, 4, 2, 0>",
        "enc5.dg0+enc5.dg1": "conv_gemm_v3_pair_kernel<4, 8, 4>",
        "enc4.dg0+enc4.dg1": "conv_gemm_v3_pair_kernel<8, 8, 4>",
        "enc3.dg0+enc3.dg1": "conv_gemm_v3_pair_kernel<16, 8, 2>",
    }),
}

_reports = {}


def child_report(B, length):
    """the forced run: a fresh process (the switches are read once per process), at most one alive at a time.  A child that was killed
    by a signal, aborted, faulted or hung ends the whole session: nothing more is started on the card."""
    env = dict(os.environ, **FORCED_ENV)
    cmd = [sys.executable, os.path.join(HERE, "dccrn_products_worker.py"), str(B), str(length)]
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired as e:
        pytest.exit(f"dccrn_products_worker.py did not finish in 300 s\n{e.stdout}\n{e.stderr}", returncode=1)
    if r.returncode < 0 or r.returncode in (134, 139):
        pytest.exit(f"dccrn_products_worker.py ended with {r.returncode}\n{r.stdout[-4000:]}\n{r.stderr[-4000:]}", returncode=1)
    assert r.returncode == 0, (r.returncode, r.stdout[-4000:], r.stderr[-4000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def report(tag):
    if tag not in _reports:
        cfg = RUNS[tag]
        if tag == "B-forced":
            _reports[tag] = child_report(cfg["B"], cfg["length"])
        else:
            with pytest.MonkeyPatch.context() as mp:       # plan.call / workspace.call wrapped for this step only
                _reports[tag] = W.run_step(cfg["B"], cfg["length"], deterministic=tag == "B-det", fuse_enc0=tag == "B-bn_dz", patch=mp.setattr)
    return _reports[tag]


@pytest.mark.parametrize("tag", list(RUNS))
def test_every_product_launch_against_float64(tag):
    rep = report(tag)
    print(W.summary(tag, rep))
    assert rep["T"] == RUNS[tag]["T"]
    assert not rep["failures"], rep["failures"]
    assert rep["intercepted"] == rep["compared"] == len(rep["launches"]) > 40        # no product launch goes uncompared
    kinds = set(k.split(".")[-1] for la in rep["launches"] for k in la["figs"])
    assert {"rms", "ulp", "f32", "dW", "dW_slice"} <= kinds
    # the two fused reduce passes: exactly the launches whose descriptor carries the bnr_* operands were compared, both of them
    assert rep["bnr"] == rep["bnr_expected"] == rep["bnr_compared"] == ["dec4.dg", "dec5.dg"]
    assert sum("bnr_part" in la["figs"] for la in rep["launches"]) == 2
    assert ("stats" in kinds) == (tag != "B-det")
    assert rep["enc0_bn_in_wgrad"] == (tag == "B-bn_dz") == ("bn_dz_dW" in kinds) == (rep["bn_dz_dbias"] is not None)
    got = {la["label"]: la["kernel"] for la in rep["launches"]}
    assert len(got) == len(rep["launches"]), "a launch label repeats"
    assert got == DISPATCH[tag], json.dumps(got, indent=1)


def params_of(kernel):
    return [p.strip() for p in kernel.split("<", 1)[1].rsplit(">", 1)[0].split(",")] if "<" in kernel else []


# kernels of the five runs that the recorded bench step does not launch, each with the reason
_DET = "reached only under sehip_set_deterministic (off by default): "
NOT_IN_THE_BENCH_STEP = {
    "conv_narrow_kernel": _DET + "enc0.fwd without the fused statistics (convn_stream_kernel takes a one-destination product only with them)",
    "conv_small2_kernel": _DET + "enc1.fwd, dec3 / dec4 forward pairs without the fused statistics (the same rule of the streaming kernels)",
    "conv_small_wgrad_kernel": _DET + "the outer layers' weight gradients without the atomics of the streaming weight-gradient kernels",
}
# product kernels of the recorded bench step that no run here reaches, each with the reason
NOT_REACHED = {}


def test_dispatch_covers_the_kernels_of_the_bench_step():
    """profiles/r6_kernel_stats.csv is the recorded bench step (B = 32, T = 323).  Every product kernel family it launches is launched
    by one of the five runs, and nothing else is -- with both conv_gemm_v3 tile heights, for the single and the pair kernel"""
    fam = ("conv_gemm_v3", "conv_wgrad", "narrow_wgrad_mfma", "dense_tile_wgrad", "gemm_pair_kernel", "wgrad_kernel")
    bench = set()
    with open(os.path.join(HERE, "..", "profiles", "r6_kernel_stats.csv")) as f:
        for line in f:
            if line.startswith('"'):
                name = W.base_name(line.split('"')[1])
                if name.startswith(fam) or name.endswith("_stream_kernel"):
                    bench.add(name)
    bench.discard("narrow_wgrad_reduce_kernel")          # the second launch of narrow_wgrad_mfma's call: sehip_last_kernel names the first
    assert len(bench) == 14, sorted(bench)
    kernels = set(la["kernel"] for tag in RUNS for la in report(tag)["launches"])
    mine = set(W.base_name(k) for k in kernels)
    assert mine - bench == set(NOT_IN_THE_BENCH_STEP), sorted(mine - bench)
    assert bench - mine == set(NOT_REACHED), sorted(bench - mine)
    tm_single = set(params_of(k)[3] for k in kernels if W.base_name(k) == "conv_gemm_v3_kernel")
    tm_pair = set(params_of(k)[1] for k in kernels if W.base_name(k) == "conv_gemm_v3_pair_kernel")
    assert {"6", "8"} <= tm_single and {"6", "8"} <= tm_pair, (sorted(tm_single), sorted(tm_pair))
