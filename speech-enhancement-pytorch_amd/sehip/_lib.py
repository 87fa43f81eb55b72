"""ctypes binding of libsehip.so -- the C-ABI boundary (include/sehip.h).

There is no fallback: if the shared library is missing or a call fails, a SehipError is raised.
All device pointers are borrowed from torch tensors that the caller keeps alive; every call is
asynchronous on the caller's current HIP stream.
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SEHIP_LIB") or os.path.join(_HERE, "libsehip.so")   # SEHIP_LIB: A/B of two builds in tools/


class SehipError(RuntimeError):
    pass


_lib = None

P = C.c_void_p
I = C.c_int
L = C.c_long
F = C.c_float
U = C.c_uint
D = C.c_double

# name -> argtypes (all return int status unless listed in _RESTYPE)
_PROTOS = {
    "sehip_version": [],
    "sehip_check_device": [I],
    "sehip_set_deterministic": [I],
    "sehip_get_deterministic": [],
    "sehip_event_create": [],
    "sehip_stream_create": [C.c_int],
    "sehip_stream_destroy": [P],
    "sehip_event_destroy": [P],
    "sehip_stream_depend": [P, P, P],
    "sehip_event_record": [P, P],
    "sehip_stream_wait_event": [P, P],
    "sehip_stft_frames": [I, I, I],
    "sehip_stft_custom_frames": [I, I, I, I],
    "sehip_stft_custom_fwd": [P, I, I, I, I, I, I, P, P],
    "sehip_istft_custom_fwd": [P, I, I, I, I, I, I, I, P, P, P],
    "sehip_comm_unique_id": [P],
    "sehip_comm_init": [P, I, I, P],
    "sehip_allreduce_f32": [P, P, L, P],
    "sehip_allreduce_i32_max": [P, P, L, P],
    "sehip_comm_info": [P, P, P, P],
    "sehip_comm_destroy": [P],
    "sehip_wav_row_stats": [P, P, I, P, P],
    "sehip_wav_collate": [P, P, P, P, P, P, I, F, I, I, P, P],
    "sehip_resample_out_len": [L, I, I],
    "sehip_resample_frac": [P, P, I, P, I, I, I, P, P, P],
    "sehip_sisnr_fwd": [P, P, I, I, P, P, P],
    "sehip_sisdr_metric": [P, P, I, I, P, P, P],
    "sehip_stoi_out_len": [L, I],
    "sehip_stoi_frames": [L],
    "sehip_stoi_segment_blocks": [I, I],
    "sehip_stoi_resample": [P, P, I, L, P, I, I, I, P, P],
    "sehip_stoi_levels": [P, I, L, P, P],
    "sehip_stoi_select": [P, I, I, P, P, P],
    "sehip_stoi_bands": [P, P, I, L, P, P, P, P],
    "sehip_stoi_segments": [P, P, I, I, I, P, P, P, P],
    "sehip_stoil_segment_floats": [I, I],
    "sehip_stoil_segments": [P, P, I, I, I, P, I, F, P, P, P],
    "sehip_stoil_bands": [P, I, L, P, P, P, P, P, P],
    "sehip_stoil_compact": [P, P, P, I, L, P, P, P],
    "sehip_stoil_resample_adj": [P, I, L, P, I, I, I, P, P],
    "sehip_mrl_frames": [L, I],
    "sehip_mrl_blocks": [L, I],
    "sehip_mrl_check": [I, P, I, L],
    "sehip_mrl_forward": [P, P, I, L, I, I, I, P, P, P],
    "sehip_mrl_finalize": [P, I, P, I, L, F, F, P, P, P, P],
    "sehip_mrl_backward": [P, P, I, L, I, I, I, P, P, P, F, F, P, P],
    "sehip_mrl_gather": [P, I, L, I, I, I, I, P, P],
    "sehip_mrl_magnitudes": [P, I, L, I, I, I, P, P, P],
    "sehip_mrl_pair_blocks": [I, I, I, L, I],
    "sehip_mrl_pair_forward": [P, P, I, I, I, L, I, I, I, P, P, P],
    "sehip_mrl_pair_select": [P, I, P, I, I, I, L, F, F, P, F, P, P, P, P, P, P],
    "sehip_mrl_pair_backward": [P, P, I, I, I, L, I, I, I, P, P, P, P, F, F, P, P],
    "sehip_sisnr_bwd": [P, P, P, P, I, I, P, P],
    "sehip_sisnr_pit_fwd": [P, P, I, I, I, I, P, P, P, P, P],
    "sehip_sisnr_pit_bwd": [P, P, P, P, P, I, I, I, I, P, P],
    "sehip_pit_pointwise_blocks": [I, I, I, I],
    "sehip_pit_pointwise_fwd": [P, P, I, I, I, I, I, P, P, P, P, P],
    "sehip_pit_pointwise_bwd": [P, P, P, P, I, I, I, I, I, P, P],
    "sehip_psa_loss_fwd": [P, P, P, L, P, P, P],
    "sehip_psa_loss_bwd": [P, P, P, L, P, P, P],
    "sehip_pointwise_loss_fwd": [P, P, L, I, P, P, P],
    "sehip_pointwise_loss_bwd": [P, P, L, I, P, P, P],
    "sehip_grad_sumsq": [P, L, P, P],
    "sehip_opt_step": [P, P, P, P, L, P, F, F, F, F, F, I, P, F, I, F, P],
    "sehip_opt_step_g": [P, P, P, P, L, P, F, F, F, F, F, I, P, F, I, F, P, P],
    "sehip_opt_step_m": [P, P, P, P, L, P, F, F, F, F, F, I, P, F, I, F, P, P, I, P, P, P, P],
    "sehip_opt_begin_g": [P, I, P, P, I, P, P],
    "sehip_counter_add": [P, I, P],
    "sehip_zero_regions": [P, L, P, L, P, L, P, L, P],
    "sehip_gemm_takes_gln_stats": [P],
    "sehip_init": [],
    "sehip_grad_metric": [P, P, I, L, P, P, P, P],
    "sehip_opt_begin": [P, I, P, P, I, P],
    "sehip_grad_sumsq_acc": [P, L, P, P],
    "sehip_grad_metric_acc": [P, P, I, L, P, P, P, P],
    "sehip_cbn_scratch_floats": [L, I],
    "sehip_stft_fwd": [P, P, I, I, I, I, I, P, P, P],
    "sehip_istft_fwd": [P, P, P, P, I, I, I, I, I, I, I, P, P, P],
    "sehip_istft_bwd": [P, P, P, P, P, P, I, I, I, I, I, I, I, P, P],
    "sehip_gemm": [P, P],
    "sehip_gemm_pair": [P, P, P],
    "sehip_wgrad": [P, P],
    "sehip_wgrad_pair": [P, P, P],
    "sehip_bnr_rows": [P, P],
    "sehip_cbn_bwd_finalize_n": [P, I, P, P, P, P, L, I, P, P, P, P, P, P, P, P],
    "sehip_wgrad_group_bytes": [I],
    "sehip_wgrad_group_prepare": [P, I, P, P],
    "sehip_wgrad_group": [P, I, I, P],
    "sehip_wgrad_dense_group_bytes": [I],
    "sehip_wgrad_dense_group_prepare": [P, I, P, L, P],
    "sehip_wgrad_dense_group": [P, I, P, P, P],
    "sehip_gemm_desc_size": [],
    "sehip_conv_small_takes": [P, P],
    "sehip_pack_bf16": [P, P, L, P, P],
    "sehip_pack_f32": [P, P, L, P, P],
    "sehip_pack_head": [P, P, L, P, P, L, P, P, L, P],
    "sehip_unpack_grad": [P, P, L, P, P],
    "sehip_unpack_grad_sums": [P, P, L, P, P, I, P, P, P, P, P],
    "sehip_unpack_grad_sums_perm": [P, P, P, L, P, P, I, P, P, P, P, P],
    "sehip_unpack_grad1": [P, P, L, P, P],
    "sehip_unpack_grad1_sums": [P, P, L, P, P, I, P, P, P, P, P],
    "sehip_unpack_grad_list_sums": [P, P, P, L, P, P, I, P, P, P],
    "sehip_unpack_grad_list": [P, P, P, L, P, P],
    "sehip_pack_bf16_runs": [P, P, P, L, P, P],
    "sehip_pack_bf16_runs_to": [P, P, P, P, L, P, P],
    "sehip_cbn_stats": [P, L, I, P, P],
    "sehip_cbn_finalize": [P, P, P, P, P, P, P, P, P, P, P, P, L, I, F, F, I, P, P],
    "sehip_cbn_finalize_n": [P, I, P, P, P, P, P, P, P, P, P, P, P, L, I, F, F, I, P, P],
    "sehip_cbn_apply": [P, P, P, L, I, P, P],
    "sehip_cbn_finalize_apply_n": [P, P, I, P, P, P, P, P, P, P, P, P, P, P, L, I, F, F, I, P, P, P, P],
    "sehip_cbn_bwd_reduce": [P, P, P, P, P, L, I, I, I, I, P, P],
    "sehip_cbn_bwd_finalize": [P, P, P, P, P, L, I, P, P, P, P, P, P, P, P],
    "sehip_cbn_bwd_apply": [P, P, P, P, P, P, L, I, I, I, I, P, P],
    "sehip_cbn_bwd_fused": [P, P, P, P, P, P, P, P, L, I, I, I, I, P, P, I, P, P, P, P, P, P, P, P],
    "sehip_cbn_bwd_reduce_fin": [P, P, P, P, P, P, P, P, L, I, I, I, I, P, I, P, P, P, P, P, P, P, P, P],
    "sehip_rbn_scratch_floats": [L, I],
    "sehip_rbn_stats": [P, L, I, I, P, P],
    "sehip_rbn_finalize": [P, P, P, P, P, P, P, P, P, P, P, L, I, I, F, F, I, P, P],
    "sehip_rbn_finalize_s": [P, P, P, P, P, P, P, P, P, P, P, L, I, I, F, F, I, P, P, P],
    "sehip_rbn_apply": [P, P, L, I, I, P, P],
    "sehip_rbn_bwd_reduce": [P, P, P, L, I, I, P, P],
    "sehip_rbn_bwd_reduce_fin": [P, P, P, L, I, I, P, P, P, P, P, P, P, P],
    "sehip_rbn_bwd_finalize": [P, P, L, I, I, P, P, P, P, P, P],
    "sehip_rbn_bwd_apply": [P, P, P, P, L, I, I, P, P],
    "sehip_dcunet_pack_input": [P, I, I, I, P, P],
    "sehip_dcunet_mask_fwd": [P, P, P, P, P, P, I, I, I, I, I, I, P, P, P],
    "sehip_dcunet_mask_bwd": [P, P, P, P, P, P, I, I, I, I, I, I, P, P, P],
    "sehip_dcunet_mask_fwd_bn": [P, P, P, P, P, P, P, I, I, I, I, I, I, P, P, P],
    "sehip_dcunet_tail_scratch_floats": [I, I, I, I],
    "sehip_dcunet_tail_bwd": [P, P, P, P, P, P, P, I, I, I, I, I, I, P, P, P, P, P, P, P, P, P],
    "sehip_ctn_encoder_fwd": [P, P, P, P, I, I, I, I, I, P, P, P],
    "sehip_ctn_encoder_bwd": [P, P, P, P, P, I, I, I, I, I, P, P, P],
    "sehip_ctn_codec_bwd_scratch_floats": [I, I, I, I, I],
    "sehip_ctn_gln_stats": [P, P, I, I, I, P, P],
    "sehip_ctn_dwconv_fwd": [P, P, P, P, P, P, I, I, P, I, I, I, P, P, P],
    "sehip_ctn_gln_apply": [P, P, P, P, P, I, I, I, P, P],
    "sehip_ctn_gln_bwd": [P, P, P, P, P, P, P, I, I, I, I, I, I, P, P, P, P, P, P],
    "sehip_ctn_gln_bwd_scratch_floats": [I, I, I],
    "sehip_ctn_dwconv_fwd_causal": [P, P, P, P, P, P, I, I, P, I, I, I, P, P, P],
    "sehip_ctn_gln_bwd_causal": [P, P, P, P, P, P, P, I, I, I, I, I, I, P, P, P, P, P, P],
    "sehip_ctn_cln_apply": [P, P, P, P, I, I, I, P, P],
    "sehip_ctn_cln_dwconv_fwd": [P, P, P, P, P, I, I, I, I, I, I, P, P],
    "sehip_ctn_cln_bwd_scratch_floats": [I, I, I],
    "sehip_ctn_cln_bwd": [P, P, P, P, P, P, I, I, I, I, I, I, I, P, P, P, P, P],
    "sehip_ctn_mask_softmax_fwd": [P, L, I, I, P, P],
    "sehip_ctn_mask_softmax_bwd": [P, P, L, I, I, P],
    "sehip_ctn_decoder_fwd": [P, P, P, I, I, I, I, I, I, I, P, P],
    "sehip_ctn_decoder_bwd": [P, P, P, P, I, I, I, I, I, I, I, P, P, P, P, P],
    "sehip_ctns_encoder": [P, P, P, P, P, P, I, I, I, I, I, P, P, P],
    "sehip_ctns_dwconv": [P, P, P, P, P, P, P, P, I, I, I, I, I, P, P],
    "sehip_ctns_decoder": [P, P, P, P, P, P, I, I, I, I, I, I, P, P],
    "sehip_ctns_advance": [P, P, I, I, P],
    "sehip_dcs_analysis": [P, P, P, P, I, I, I, I, P, P, P, P, P],
    "sehip_dcs_norm_hist": [P, P, P, P, P, P, P, I, I, I, I, I, I, P, P],
    "sehip_dcs_lstm_carry": [P, P, I, I, I, P],
    "sehip_dcs_synthesis": [P, P, P, P, P, P, P, P, P, I, I, I, I, I, P, P, P],
    "sehip_dcs_mark_end": [P, P, I, I, P],
    "sehip_dcs_advance": [P, P, I, I, P],
    "sehip_dmx_prep": [P, I, I, I, I, I, I, I, I, P, I, I, P, P, P, P],
    "sehip_dmx_post": [P, P, I, I, I, L, I, I, I, P, I, I, P, P],
    "sehip_dmx_post_bwd": [P, P, I, I, I, L, I, I, I, P, I, I, P, P],
    "sehip_dmx_gn_stats": [P, I, I, I, I, P, P],
    "sehip_dmx_act_fwd": [P, P, P, P, I, F, I, P, P, P, I, I, I, P, P],
    "sehip_dmx_act_bwd": [P, P, P, P, P, I, F, I, P, I, I, I, P, P, P, P],
    "sehip_dmx_add": [P, P, L, P, P],
    "sehip_dmx_f32_to_bf16": [P, L, P, P],
    "sehip_dmx_frames": [I, P, P, I, I, I, I, I, I, P, P],
    "sehip_dmx_lstm_sync_bytes": [],
    "sehip_dmx_lstm_fwd": [P, P, I, I, I, P, P, P, P],
    "sehip_dmx_lstm_bwd": [P, P, P, P, I, I, I, P, P, P, P],
    "sehip_dmx_attn_fwd": [P, I, I, I, I, I, I, P, P],
    "sehip_dmx_attn_bwd_scratch_floats": [I, I, I],
    "sehip_dmx_attn_bwd": [P, P, I, I, I, I, I, I, P, P, P],
    "sehip_lstm_fwd": [P, P, P, I, I, I, P, P, P, P],
    "sehip_lstm_bwd": [P, P, P, P, P, I, I, I, P, P, P],
    "sehip_rlstm_fwd": [P, P, I, I, I, P, P, P, P],
    "sehip_rlstm_bwd": [P, P, P, P, I, I, I, P, P],
    "sehip_lstm2_gran_bytes": [I, I, I],
    "sehip_lstm2_sync_bytes": [],
    "sehip_lstm2_fwd": [P, P, P, P, P, P, I, I, I, P, P, P, P, P, P, P, P, U, P],
    "sehip_lstm2_bwd": [P, P, P, P, P, P, P, P, P, I, I, I, P, P, P, P, P, P, U, P],
    "sehip_lstm_fwd_chunk": [P, P, P, I, I, I, I, I, P, P, P, P],
    "sehip_lstm_bwd_chunk": [P, P, P, P, P, I, I, I, I, I, P, P, P, P],
    "sehip_wun_bn_scratch_floats": [L, I],
    "sehip_wun_enc0_wgrad_scratch_floats": [I, I, I],
    "sehip_wun_out_bwd_scratch_floats": [L, I],
    "sehip_wun_enc0_fwd": [P, P, P, I, I, I, P, P],
    "sehip_wun_enc0_wgrad": [P, P, I, I, I, P, P, P, P],
    "sehip_wun_bn_stats": [P, L, I, P, P],
    "sehip_wun_bn_finalize": [P, P, P, P, P, P, P, L, I, F, F, I, P, P],
    "sehip_wun_bn_apply": [P, P, L, I, P, P],
    "sehip_wun_bn_apply_up2": [P, P, I, I, I, P, P],
    "sehip_wun_up2_bwd": [P, I, I, I, P, P],
    "sehip_wun_bn_bwd_reduce": [P, P, P, P, L, I, P, P],
    "sehip_wun_bn_bwd_finalize": [P, P, L, I, P, P, P, P],
    "sehip_wun_bn_bwd_apply": [P, P, P, P, P, L, I, P, P],
    "sehip_wun_out_fwd": [P, P, P, P, L, I, P, P],
    "sehip_wun_out_bwd": [P, P, P, P, P, L, I, P, P, P, P, P],
    "sehip_rsm_sum_scratch_floats": [L, I],
    "sehip_rsm_counter_next": [P, P, P],
    "sehip_rsm_features": [P, I, I, I, I, P, P],
    "sehip_rsm_pack_w": [P, I, I, I, I, P, P],
    "sehip_rsm_gemm_nt": [P, I, P, I, I, I, I, I, P, P, I, P],
    "sehip_rsm_gemm_tn": [P, I, P, I, I, I, I, I, I, P, I, P],
    "sehip_rsm_rnn_fwd": [I, P, P, P, P, P, P, I, I, I, I, U, U, P, I, U, F, P],
    "sehip_rsm_rnn_bwd": [I, P, P, P, P, P, P, I, I, I, I, U, U, P, I, U, F, P],
    "sehip_rsm_colsum": [P, I, P, P, L, I, P, P],
    "sehip_rsm_colsum_finalize": [P, L, I, P, P, P, P, P, P],
    "sehip_rsm_bn_apply": [P, P, L, I, P, P],
    "sehip_rsm_bn_bwd_apply": [P, P, P, P, L, I, P, P],
    "sehip_rsm_mask_fwd": [P, P, I, I, I, I, I, I, P, P],
    "sehip_rsm_mask_bwd": [P, P, P, I, I, I, I, I, I, P, P],
    "sehip_rsm_elman_fwd": [P, P, P, P, I, I, I, I, P],
    "sehip_rsm_elman_bwd": [P, P, P, P, I, I, I, I, P],
    "sehip_rsm_gemm_nt_head": [P, I, P, I, I, I, I, I, P, P, I, P, I, P],
    "sehip_rsm_mask_bwd_sigmoid": [P, P, P, I, I, I, I, I, I, P, P],
    "sehip_ha_fir_fwd": [P, L, L, P, I, I, P, P, P],
    "sehip_ha_fir_adj": [P, L, L, P, I, I, P, P, P],
    "sehip_ha_compressor_ws_doubles": [L, L, I],
    "sehip_ha_compressor_fwd": [P, L, L, I, D, D, D, D, I, P, P, P, P],
    "sehip_ha_compressor_bwd": [P, P, P, L, I, P, P],
    "sehip_has_state_bytes": [L, I, I, I],
    "sehip_has_fir": [P, L, I, I, P, I, I, I, P, P, P, P, P, P],
    "sehip_has_compress": [P, L, I, I, I, P, P, D, D, D, D, I, P, P, P, P],
    "sehip_has_advance": [P, P, P, L, I, P],
    "sehip_rss_delay_frames": [I, I, I],
    "sehip_rss_state_bytes": [L, I, I, I, I],
    "sehip_rss_feed": [P, L, I, I, P, I, I, I, P, P, L, P, P],
    "sehip_rss_advance": [P, L, I, P],
    "sehip_unet_features": [P, I, I, I, I, I, P, P],
    "sehip_unet_mask_fwd": [P, P, P, I, I, I, I, I, P, P],
    "sehip_unet_mask_bwd": [P, P, I, I, I, I, I, P, P],
    "sehip_unet_bn_finalize": [P, P, P, P, P, P, P, L, I, I, F, F, I, P, P],
    "sehip_unet_bn_act": [P, P, L, I, U, U, P, I, U, F, P, P],
    "sehip_unet_bn_act_pool": [P, P, I, I, I, I, U, U, P, I, U, F, P, P, P],
    "sehip_unet_bn_bwd_reduce": [P, P, P, P, I, I, I, I, U, U, P, I, U, F, P, P],
    "sehip_unet_bn_bwd_apply": [P, P, P, P, P, I, I, I, I, U, U, P, I, U, F, P, P],
}
_RESTYPE = {"sehip_mrl_frames": C.c_long, "sehip_mrl_blocks": C.c_long, "sehip_mrl_pair_blocks": C.c_long, "sehip_resample_out_len": C.c_long,"sehip_stoi_out_len": C.c_long, "sehip_stoil_segment_floats": C.c_long, "sehip_ha_compressor_ws_doubles": C.c_long, "sehip_has_state_bytes": C.c_long, "sehip_rss_delay_frames": C.c_long, "sehip_rss_state_bytes": C.c_long, "sehip_rsm_sum_scratch_floats": C.c_long, "sehip_wun_bn_scratch_floats": C.c_long, "sehip_wun_enc0_wgrad_scratch_floats": C.c_long, "sehip_wun_out_bwd_scratch_floats": C.c_long,
            "sehip_lstm2_gran_bytes": C.c_long, "sehip_dmx_attn_bwd_scratch_floats": C.c_long, "sehip_ctn_codec_bwd_scratch_floats": C.c_long, "sehip_ctn_gln_bwd_scratch_floats": C.c_long, "sehip_ctn_cln_bwd_scratch_floats": C.c_long, "sehip_wgrad_group_bytes": C.c_long, "sehip_wgrad_dense_group_bytes": C.c_long, "sehip_cbn_scratch_floats": C.c_long, "sehip_rbn_scratch_floats": C.c_long, "sehip_dcunet_tail_scratch_floats": C.c_long, "sehip_event_create": C.c_void_p, "sehip_stream_create": C.c_void_p}


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SehipError(
                f"{LIB_PATH} is missing: build it with `python {os.path.join(_HERE, 'build.py')}` "
                "(hipcc --offload-arch=gfx950). There is no CPU/PyTorch fallback for the HIP path.")
        _lib = C.CDLL(LIB_PATH)
        _lib.sehip_last_error.restype = C.c_char_p
        _lib.sehip_last_kernel.restype = C.c_char_p
        for name, args in _PROTOS.items():
            fn = getattr(_lib, name, None)
            if fn is None:
                continue
            fn.argtypes = args
            fn.restype = _RESTYPE.get(name, C.c_int)
    return _lib


def declared_symbols():
    return ["sehip_last_error", "sehip_last_kernel"] + list(_PROTOS)


def check(status, what=""):
    if status != 0:
        msg = lib().sehip_last_error().decode()
        raise SehipError(f"{what}: status {status}: {msg}")


def call(name, *args):
    fn = getattr(lib(), name)
    check(fn(*args), name)


def ptr(t):
    """Device (or host) pointer of a contiguous tensor, None -> NULL."""
    if t is None:
        return None
    assert t.is_contiguous(), "libsehip needs contiguous tensors"
    return t.data_ptr()


import threading

_tls = threading.local()      # per thread: autograd's backward thread (and any user thread) never sees another thread's cached stream


def stream():
    """hipStream_t of torch's current stream (cached inside a stream_scope of the calling thread)."""
    h = getattr(_tls, "handle", None)
    if h is not None:
        return h
    return torch.cuda.current_stream().cuda_stream


class stream_scope:
    """Looks torch's current stream up ONCE for all library calls the calling thread makes inside the scope: the lookup costs
    ~8 us of host time and a training step makes ~110 of them (a quarter of the step's launch time).  Code inside must not
    switch torch's current stream and then expect stream() to follow (the side streams of sehip/plan.py are passed as explicit
    handles): with SEHIP_DEBUG_STREAMS set the exit checks that torch's current stream is still the cached one."""

    def __enter__(self):
        self._prev = getattr(_tls, "handle", None)
        _tls.handle = torch.cuda.current_stream().cuda_stream
        return self

    def __exit__(self, *exc):
        cached = _tls.handle
        _tls.handle = self._prev
        if exc[0] is None and os.environ.get("SEHIP_DEBUG_STREAMS") and torch.cuda.current_stream().cuda_stream != cached:
            raise SehipError("stream_scope: torch's current stream changed inside the scope; library calls went to the stream "
                             "that was current at entry")
        return False


def require_gpu(t, what):
    if not t.is_cuda:
        raise SehipError(f"{what}: tensor is on {t.device}; the HIP path needs a gfx950 GPU (no CPU fallback)")
