"""ctypes binding of libslotformer_hip.so (include/slotformer_hip.h).

The product path has NO fallback: if the HIP library is missing or a call fails, a
RuntimeError is raised.  Nothing here imports oracle/.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('SF_LIB_PATH') or os.path.join(_HERE, 'libslotformer_hip.so')   # (SF_LIB_PATH: a variant build, tools/ only)

FP = C.c_void_p  # device float*


class sf_tfm_layer(C.Structure):
    _fields_ = [(n, FP) for n in (
        'norm1_g', 'norm1_b', 'in_proj_w', 'in_proj_b', 'out_proj_w', 'out_proj_b',
        'norm2_g', 'norm2_b', 'lin1_w', 'lin1_b', 'lin2_w', 'lin2_b', 'lin1_packed', 'lin2_packed', 'attn_in_packed', 'attn_out_packed', 'tok_packed')]


class sf_rollouter(C.Structure):
    _fields_ = [(n, C.c_int) for n in (
        'num_slots', 'slot_size', 'd_model', 'num_layers', 'num_heads', 'ffn_dim', 'norm_first',
        'window_len', 'single_step')] + [(n, FP) for n in (
            'in_proj_w', 'in_proj_b', 'out_proj_w', 'out_proj_b', 'pe_tok')] + [
                ('layers', C.POINTER(sf_tfm_layer)), ('in_proj_packed', C.c_void_p), ('out_proj_packed', C.c_void_p)]


class sf_aloe(C.Structure):
    _fields_ = [(n, C.c_int) for n in ('num_slots', 'slot_size', 'T', 'text_len', 'question_len', 'd_model', 'num_heads', 'ffn_dim', 'num_layers',
                                       'vocab', 'emb_dim')] + [(n, FP) for n in ('cls', 'pos', 'vision_w', 'vision_b', 'q_in_proj_w', 'text_table')] + [
                                           ('layers', C.POINTER(sf_tfm_layer))]


class sf_rollout_opts(C.Structure):
    _fields_ = [(n, C.c_int) for n in ('precision', 'seam_fused', 'ffn_rows', 'attn_heads_per_wg', 'attn_qkv_rows', 'ffn_tile', 'cus_available', 'layer_tok')]


class sf_tfm_layer_grads(C.Structure):
    _fields_ = [(n, FP) for n in (
        'norm1_g', 'norm1_b', 'in_proj_w', 'in_proj_b', 'out_proj_w', 'out_proj_b',
        'norm2_g', 'norm2_b', 'lin1_w', 'lin1_b', 'lin2_w', 'lin2_b')]


class sf_phyre_readout_model(C.Structure):
    _fields_ = [(n, C.c_int) for n in ('num_slots', 'slot_size', 'd_model', 'num_heads', 'ffn_dim', 'num_layers')] + [
        (n, FP) for n in ('in_proj_w', 'in_proj_b', 'enc_t_pe', 'cls')] + [('layers', C.POINTER(sf_tfm_layer))] + [
            (n, FP) for n in ('mlp_w1', 'mlp_b1', 'mlp_w2', 'mlp_b2')]


class sf_phyre_readout_grads(C.Structure):
    _fields_ = [(n, FP) for n in ('in_proj_w', 'in_proj_b', 'enc_t_pe', 'cls')] + [('layers', C.POINTER(sf_tfm_layer_grads))] + [
        (n, FP) for n in ('mlp_w1', 'mlp_b1', 'mlp_w2', 'mlp_b2')]


_ALOE_HEADS = ('cls_w1', 'cls_b1', 'cls_w2', 'cls_b2', 'mc_w1', 'mc_b1', 'mc_w2', 'mc_b2')
_ALOE_LEAVES = ('cls', 'pos', 'vision_w', 'vision_b', 'q_embedding', 'q_in_proj_w', 'q_in_proj_b')


class sf_aloe_model(C.Structure):
    _fields_ = [(n, C.c_int) for n in ('num_slots', 'slot_size', 'T', 'text_len', 'question_len', 'd_model', 'num_heads', 'ffn_dim', 'num_layers',
                                       'vocab', 'emb_dim', 'mlp_hidden', 'num_answers')] + [(n, FP) for n in _ALOE_LEAVES] + [
                                           ('layers', C.POINTER(sf_tfm_layer))] + [(n, FP) for n in _ALOE_HEADS]


class sf_aloe_grads(C.Structure):
    _fields_ = [(n, FP) for n in _ALOE_LEAVES] + [('layers', C.POINTER(sf_tfm_layer_grads))] + [(n, FP) for n in _ALOE_HEADS]


class sf_rollouter_grads(C.Structure):
    _fields_ = [(n, FP) for n in ('in_proj_w', 'in_proj_b', 'out_proj_w', 'out_proj_b')] + [
        ('layers', C.POINTER(sf_tfm_layer_grads)), ('pe_tok', FP)]


_SA_LEAVES = ('norm_in_g', 'norm_in_b', 'wk', 'wv', 'q_ln_g', 'q_ln_b', 'wq', 'gru_w_ih', 'gru_w_hh', 'gru_b_ih', 'gru_b_hh',
              'mlp_ln_g', 'mlp_ln_b', 'mlp_w1', 'mlp_b1', 'mlp_w2', 'mlp_b2')


class sf_slot_attention(C.Structure):
    _fields_ = [(n, C.c_int) for n in ('in_features', 'slot_size', 'mlp_hidden', 'num_slots')] + [
        (n, FP) for n in _SA_LEAVES] + [('eps', C.c_float)]


class sf_slot_attention_grads(C.Structure):
    _fields_ = [(n, FP) for n in _SA_LEAVES]


class sf_adam_group(C.Structure):
    _fields_ = [('begin', C.c_longlong), ('lr', C.c_float)]


class sf_savi_decoder_grads(C.Structure):
    _fields_ = [('deconv_w', FP * 8), ('deconv_b', FP * 8)] + [(n, FP) for n in ('out_w', 'out_b', 'pos_w', 'pos_b')]


class sf_savi_features(C.Structure):
    _fields_ = [(n, C.c_int) for n in ('resolution', 'layers', 'channels', 'ks', 'hidden', 'out_channels')] + [
        ('conv_w', FP * 8), ('conv_b', FP * 8)] + [(n, FP) for n in ('pos_grid', 'pos_w', 'pos_b', 'ln_g', 'ln_b', 'fc1_w', 'fc1_b',
                                                                      'fc2_w', 'fc2_b')]


class sf_savi_features_grads(C.Structure):
    _fields_ = [('conv_w', FP * 8), ('conv_b', FP * 8)] + [(n, FP) for n in ('pos_w', 'pos_b', 'ln_g', 'ln_b', 'fc1_w', 'fc1_b',
                                                                              'fc2_w', 'fc2_b')]


class sf_savi_encoder(C.Structure):
    _fields_ = (
        [('resolution', C.c_int), ('enc_layers', C.c_int), ('enc_channels', C.c_int * 9),
         ('enc_ks', C.c_int)] +
        [(n, C.c_int) for n in ('enc_out_channels', 'num_slots', 'slot_size', 'slot_mlp_size',
                                'num_iterations')] +
        [('conv_w', FP * 8), ('conv_b', FP * 8), ('pos_table', FP)] +
        [(n, FP) for n in ('enc_ln_g', 'enc_ln_b', 'enc_fc1_w', 'enc_fc1_b', 'enc_fc2_w', 'enc_fc2_b',
                           'sa_norm_in_g', 'sa_norm_in_b', 'sa_q_ln_g', 'sa_q_ln_b', 'sa_q_w', 'sa_kv_w',
                           'gru_w_ih', 'gru_w_hh', 'gru_b_ih', 'gru_b_hh',
                           'mlp_ln_g', 'mlp_ln_b', 'mlp_w1', 'mlp_b1', 'mlp_w2', 'mlp_b2',
                           'init_latents')] +
        [('kd_mode', C.c_int)] +
        [(n, FP) for n in ('kd_w0', 'kd_b0', 'kd_ln_g', 'kd_ln_b', 'kd_w3', 'kd_b3')] +
        [(n, C.c_int) for n in ('pred_type', 'pred_rnn', 'pred_norm_first', 'pred_num_layers',
                                'pred_num_heads', 'pred_ffn_dim', 'pred_hidden')] +
        [(n, FP) for n in ('pm_ln_g', 'pm_ln_b', 'pm_w0', 'pm_b0', 'pm_w2', 'pm_b2')] +
        [('pred_layers', C.POINTER(sf_tfm_layer))] +
        [(n, FP) for n in ('lstm_w_ih', 'lstm_w_hh', 'lstm_b_ih', 'lstm_b_hh', 'proj_w', 'proj_b')] +
        [('sa_eps', C.c_float), ('sa_q_w_t', FP), ('pm_w0_t', FP), ('pm_w2_t', FP), ('kd_w0_t', FP),
         ('sa_gru_ih_p', C.c_void_p), ('sa_gru_hh_p', C.c_void_p), ('sa_mlp_w1_p', C.c_void_p), ('sa_mlp_w2_p', C.c_void_p),
         ('sa_q_w_p', C.c_void_p), ('sa_fold_q_w', FP), ('sa_fold_q_w_t', FP), ('sa_fold_gru_ih_t', FP), ('sa_fold_q_w_p', C.c_void_p),
         ('sa_fold_gru_ih_p', C.c_void_p), ('pred_packed', C.POINTER(C.c_void_p)), ('enc_fc1_p', C.c_void_p), ('enc_fc2_p', C.c_void_p),
         ('conv_w_frag', C.c_void_p * 8), ('pm_w0_p', C.c_void_p), ('pm_w2_p', C.c_void_p), ('kd_w0_p', C.c_void_p)])


class sf_slate_block(C.Structure):
    _fields_ = [(n, FP) for n in ('ln1_g', 'ln1_b', 'wqkv', 'wo', 'ln2_g', 'ln2_b', 'wq_c', 'wkv_c', 'wo_c', 'ln3_g', 'ln3_b',
                                  'w1', 'b1', 'w2', 'b2')] + [('is_first', C.c_int)]


class sf_slate_decoder(C.Structure):
    _fields_ = [(n, C.c_int) for n in ('d_model', 'num_heads', 'num_layers', 'vocab_size', 'num_slots', 'max_len')] + [
        (n, FP) for n in ('in_proj_w', 'in_proj_b', 'tok_emb', 'pos_emb', 'lnf_g', 'lnf_b', 'head_w')] + [
            ('blocks', C.POINTER(sf_slate_block))]


class sf_slate_step_opts(C.Structure):
    _fields_ = [('soft_rows', FP), ('conv0_t', FP), ('conv0_width', C.c_int), ('soft_scale', C.c_float), ('soft_seed', C.c_ulonglong),
                ('sample', C.c_int), ('inv_temperature', C.c_float), ('sample_seed', C.c_ulonglong), ('row_base', C.c_longlong)]


class sf_savi_decoder(C.Structure):
    _fields_ = ([('resolution', C.c_int), ('dec_layers', C.c_int), ('dec_channels', C.c_int * 9),
                 ('dec_strides', C.c_int * 8), ('dec_ks', C.c_int), ('dec_res', C.c_int), ('num_slots', C.c_int),
                 ('slot_size', C.c_int), ('deconv_w', FP * 8), ('deconv_b', FP * 8), ('out_w', FP), ('out_b', FP),
                 ('pos_table', FP), ('deconv_w_flipped', FP * 8), ('deconv_w_frag', C.c_void_p * 8), ('l0_weff', FP), ('l0_posterm', FP)])


class sf_egress_tile(C.Structure):
    _fields_ = [('kind', C.c_int), ('N', C.c_int), ('a', C.c_void_p), ('b', C.c_void_p), ('scale', C.c_float), ('ids_i64', C.c_int), ('P', C.c_int),
                ('history_len', C.c_int)]


class sf_lpips_model(C.Structure):
    _fields_ = [('conv_w', C.c_void_p * 13), ('conv_b', FP * 13), ('lin_w', FP * 5), ('shift', FP), ('scale', FP)]


I, LL, F32, SZ, VP = C.c_int, C.c_longlong, C.c_float, C.c_size_t, C.c_void_p

# name -> (restype, argtypes): exactly the declarations of include/slotformer_hip.h
SIGNATURES = {
    'sf_version': (I, []),
    'sf_last_error_string': (C.c_char_p, []),
    'sf_get_precision': (I, []),
    'sf_set_precision': (I, [I]),
    'sf_profile_enable': (I, [I]),
    'sf_profile_sample': (I, [I]),
    'sf_set_seam_fused': (I, [I]),
    'sf_get_seam_fused': (I, []),
    'sf_set_ffn_rows64': (I, [I]),
    'sf_get_ffn_rows64': (I, []),
    'sf_profile_read': (I, [I, C.POINTER(C.c_double), C.POINTER(C.c_longlong), C.POINTER(C.c_double)]),
    'sf_linear_f32': (I, [FP, I, FP, FP, FP, FP, F32, FP, I, FP, I, I, I, I, I, VP]),
    'sf_linear_config': (I, [I, I, I, I]),
    'sf_layernorm_f32': (I, [FP, FP, FP, FP, I, I, F32, VP]),
    'sf_conv2d_nchw_in_f32': (I, [FP, LL, FP, FP, FP, FP, I, I, I, I, I, I, I, I, VP]),
    'sf_conv2d_nchw_in_grouped_f32': (I, [FP, LL, I, LL, FP, FP, FP, FP, I, I, I, I, I, I, I, I, VP]),
    'sf_conv2d_nhwc_f32': (I, [FP, FP, FP, FP, FP, I, I, I, I, I, I, I, VP]),
    'sf_pack_conv_weight_f32': (I, [FP, FP, I, I, I, VP]),
    'sf_pixel_feat_f32': (I, [FP] * 10 + [I, F32, I, VP]),
    'sf_conv_frag_bytes': (SZ, [I, I, I]),
    'sf_set_conv_fp16x2': (I, [I]),
    'sf_get_conv_fp16x2': (I, []),
    'sf_pack_conv_frag_weights': (I, [FP, VP, I, I, I, VP]),
    'sf_conv5x5_frag_f32': (I, [FP, VP, FP, FP, FP, I, I, I, I, VP]),
    'sf_conv5x5_ws_f32': (I, [FP, VP, FP, FP, FP, I, I, I, I, I, VP]),
    'sf_deconv_frag_bytes': (SZ, [I, I, I, I]),
    'sf_pack_deconv_frag_weights': (I, [FP, VP, I, I, I, I, VP]),
    'sf_deconv5x5s2_frag_f32': (I, [FP, VP, FP, FP, I, I, I, I, VP]),
    'sf_deconv5x5s2_head_frag_f32': (I, [FP, VP, FP, FP, FP, FP, I, I, I, VP]),
    'sf_decode_l0_expand_f32': (I, [FP, FP, FP, I, I, I, VP]),
    'sf_conv_transpose2d_nhwc_f32': (I, [FP, FP, FP, FP, I, I, I, I, I, I, I, I, VP]),
    'sf_pack_deconv_weight_f32': (I, [FP, FP, I, I, I, VP]),
    'sf_slot_broadcast_f32': (I, [FP, FP, FP, I, I, I, VP]),
    'sf_decode_combine_f32': (I, [FP, FP, FP, FP, I, I, I, VP]),
    'sf_savi_decode_workspace_bytes': (SZ, [C.POINTER(sf_savi_decoder), I]),
    'sf_savi_decode_f32': (I, [C.POINTER(sf_savi_decoder), FP, FP, FP, FP, I, VP, SZ, VP]),
    'sf_savi_decode_seg_f32': (I, [C.POINTER(sf_savi_decoder), FP, FP, FP, FP, VP, VP, F32, I, VP, SZ, VP]),
    'sf_decode_combine_seg_f32': (I, [FP, FP, FP, FP, VP, VP, F32, VP, I, I, I, VP]),
    'sf_postproc_mask_f32': (I, [FP, VP, VP, F32, VP, I, I, I, VP]),
    'sf_vp_metrics_workspace_bytes': (SZ, [I, I, I]),
    'sf_vp_image_metrics_f32': (I, [FP, FP, VP, VP, VP, I, I, I, I, VP, SZ, VP]),
    'sf_vp_mask_metrics': (I, [VP, VP, I, VP, FP, VP, VP, VP, VP, I, I, I, I, VP, SZ, VP]),
    'sf_vp_bbox_pr_f32': (I, [FP, VP, FP, VP, VP, I, I, I, F32, VP]),
    'sf_masks_to_boxes': (I, [VP, I, FP, VP, I, I, I, I, VP]),
    'sf_vp_mean_over_videos_f64': (I, [VP, VP, I, I, I, VP]),
    'sf_lpips_pack_conv_weights': (I, [FP, VP, I, I, VP]),
    'sf_lpips_pack_conv_weights_host': (I, [VP, VP, I, I]),
    'sf_lpips_workspace_bytes': (SZ, [I, I, I]),
    'sf_lpips_f32': (I, [C.POINTER(sf_lpips_model), FP, FP, FP, I, I, I, I, I, VP, SZ, VP]),
    'sf_lpips_mean_over_videos_f32': (I, [FP, VP, VP, I, I, VP]),
    'sf_ingest_tables_bytes': (SZ, [I, I, I, I, I]),
    'sf_ingest_tables_host': (I, [VP, SZ, I, I, I, I, I]),
    'sf_ingest_frames_u8': (I, [VP, VP, I, VP, FP, FP, FP, I, I, I, I, I, I, I, VP]),
    'sf_resize_masks_nearest': (I, [VP, I, VP, VP, VP, I, I, I, I, I, VP]),
    'sf_rle_label_maps': (I, [VP, VP, VP, VP, VP, VP, VP, I, I, I, I, I, I, I, VP]),
    'sf_rle_boxes_pad': (I, [VP, FP, VP, VP, I, I, VP]),
    'sf_egress_frames_u8': (I, [FP, VP, LL, I, I, I, I, I, VP]),
    'sf_egress_grid_shape': (I, [I, I, I, I, I, I, C.POINTER(I), C.POINTER(I)]),
    'sf_egress_grid': (I, [C.POINTER(sf_egress_tile), I, VP, I, I, I, I, I, I, F32, I, VP]),
    'sf_egress_draw_boxes': (I, [VP, FP, VP, VP, I, I, I, I, I, I, VP]),
    'sf_pos_embed_table_f32': (I, [FP, FP, FP, FP, I, I, VP]),
    'sf_slot_attn_num_partials': (I, [I]),
    'sf_slot_attn_iter_f32': (I, [FP, FP, I, LL, FP, FP, FP, FP, I, I, I, I, F32, F32, VP]),
    'sf_slot_update_f32': (I, [FP, FP, I, FP] + [FP] * 10 + [FP, I, I, I, I, F32, VP]),
    'sf_slot_update_packed_f32': (I, [FP, FP, I, FP, VP, VP, FP, FP, FP, FP, VP, FP, VP, FP, FP, FP, FP, VP, FP, I, I, I, I, F32, VP]),
    'sf_slot_attn_iter_planes_f32': (I, [VP, LL, FP, FP, FP, FP, LL, I, I, I, F32, F32, VP]),
    'sf_slot_prologue_f32': (I, [FP] * 8 + [I, FP, FP, FP, LL, FP, LL, FP, FP, FP, FP, FP, I, I, I, F32, VP]),
    'sf_slot_update_packed_next_f32': (I, [FP, FP, I, FP, VP, VP, FP, FP, FP, FP, VP, FP, VP, FP, FP, FP, FP, VP, FP, I, I, I, I, F32,
                                           FP, LL, I, FP, FP, VP, FP, VP, FP, I, VP, FP, FP, LL, FP, LL, FP, VP]),
    'sf_mha_f32': (I, [FP, FP, I, I, I, I, I, VP]),
    'sf_qkv_attention_f32': (I, [FP, FP, FP, F32, FP, FP, FP, I, I, I, I, I, VP]),
    'sf_lstm_pointwise_f32': (I, [FP, FP, FP, FP, I, I, VP]),
    'sf_sample_dist_f32': (I, [FP, FP, FP, I, I, VP]),
    'sf_bilinear_resize_f32': (I, [FP, FP, LL, I, I, I, I, VP]),
    'sf_rollout_workspace_bytes': (SZ, [C.POINTER(sf_rollouter), I]),
    'sf_rollout_f32': (I, [C.POINTER(sf_rollouter), FP, I, I, I, VP, SZ, VP]),
    'sf_rollout_opts_f32': (I, [C.POINTER(sf_rollouter), FP, I, I, I, VP, SZ, VP, C.POINTER(sf_rollout_opts)]),
    'sf_rollout_phases_workspace_bytes': (SZ, [C.POINTER(sf_rollouter), I, I]),
    'sf_rollout_phases_f32': (I, [C.POINTER(sf_rollouter), FP, I, I, I, I, I, VP, SZ, VP, C.POINTER(sf_rollout_opts)]),
    'sf_rollout_uses_seam': (I, [C.POINTER(sf_rollouter), I]),
    'sf_rollout_uses_seam_opts': (I, [C.POINTER(sf_rollouter), I, C.POINTER(sf_rollout_opts)]),
    'sf_rollout_is_fused': (I, [C.POINTER(sf_rollouter)]),
    'sf_rollout_tok_ok': (I, [C.POINTER(sf_rollouter)]),
    'sf_rollout_tok_layers': (I, [C.POINTER(sf_rollouter), I, C.POINTER(sf_rollout_opts)]),
    'sf_ffn_chunk_partials_f32': (I, [C.POINTER(sf_tfm_layer), FP, LL, FP, LL, I, I, I, VP]),
    'sf_attn_block_f32': (I, [C.POINTER(sf_tfm_layer), FP, FP, I, I, I, I, VP]),
    'sf_ffn_block_rows_f32': (I, [C.POINTER(sf_tfm_layer), FP, FP, I, I, VP]),
    'sf_set_layer_tok': (I, [I]),
    'sf_get_layer_tok': (I, []),
    'sf_layer_tok_packed_bytes': (SZ, []),
    'sf_layer_tok_packed_bytes_ex': (SZ, [I, I, I]),
    'sf_pack_layer_tok_weights': (I, [C.POINTER(sf_tfm_layer), VP, I, I, I, VP]),
    'sf_layer_tok_block_f32': (I, [C.POINTER(sf_tfm_layer), I, FP, FP, I, I, VP]),
    'sf_layer_tok_block_ex_f32': (I, [C.POINTER(sf_tfm_layer), I, I, I, I, FP, FP, I, I, VP]),
    'sf_debug_read_ts_layer_tok': (I, [C.POINTER(C.c_longlong)]),
    'sf_attn_rows_planes_bytes': (SZ, [I]),
    'sf_attn_block_rows_f32': (I, [C.POINTER(sf_tfm_layer), FP, FP, VP, I, I, I, VP]),
    'sf_slot_attn_iter_bwd_workspace_bytes': (SZ, [I, I, I, I]),
    'sf_slot_attn_iter_bwd_f32': (I, [FP, FP, I, LL, FP, FP, FP, I, FP, FP, FP, I, FP, I, I, I, I, F32, F32, VP, SZ, VP]),
    'sf_slot_attn_iter_bwd16_workspace_bytes': (SZ, [I, I, I, I]),
    'sf_slot_attn_iter_bwd16_f32': (I, [FP, FP, I, LL, FP, FP, FP, I, FP, FP, FP, I, FP, I, I, I, I, F32, F32, VP, SZ, VP]),
    'sf_set_slot_attn_tile16': (I, [I]),
    'sf_get_slot_attn_tile16': (I, []),
    'sf_slot_attention_train_workspace_bytes': (SZ, [C.POINTER(sf_slot_attention), I, I, I]),
    'sf_slot_attention_train_fwd_f32': (I, [C.POINTER(sf_slot_attention), FP, FP, I, I, I, FP, VP, SZ, VP]),
    'sf_slot_attention_train_bwd_f32': (I, [C.POINTER(sf_slot_attention), FP, FP, FP, FP, C.POINTER(sf_slot_attention_grads), I, I, I,
                                            VP, SZ, VP]),
    'sf_savi_decode_train_workspace_bytes': (SZ, [C.POINTER(sf_savi_decoder), I]),
    'sf_savi_decode_train_fwd_f32': (I, [C.POINTER(sf_savi_decoder), FP, FP, FP, FP, I, VP, SZ, VP]),
    'sf_savi_decode_train_bwd_f32': (I, [C.POINTER(sf_savi_decoder), C.POINTER(C.c_void_p), FP, FP, FP, C.POINTER(sf_savi_decoder_grads),
                                         I, VP, SZ, VP]),
    'sf_conv_wgrad_partial_floats': (SZ, [I, I]),
    'sf_conv_wgrad_f32': (I, [FP, I, I, I, I, FP, I, I, I, I, LL, FP, FP, SZ, VP]),
    'sf_conv2d_nhwc_bwd_data_f32': (I, [FP, FP, FP, FP, I, I, I, I, I, I, I, VP]),
    'sf_pack_conv_bwd_weight_f32': (I, [FP, FP, I, I, I, VP]),
    'sf_conv_first_wgrad_workspace_bytes': (SZ, [I]),
    'sf_conv_first_wgrad_f32': (I, [FP, LL, I, FP, I, FP, VP, SZ, VP]),
    'sf_pos_dense_grad_f32': (I, [FP, I, I, I, FP, FP, FP, FP, VP]),
    'sf_savi_decode_head_bwd_workspace_bytes': (SZ, [I]),
    'sf_savi_decode_head_bwd_f32': (I, [FP, FP, FP, FP, FP, FP, FP, FP, I, I, I, I, VP, SZ, VP]),
    'sf_savi_features_train_workspace_bytes': (SZ, [C.POINTER(sf_savi_features), I]),
    'sf_savi_features_train_fwd_f32': (I, [C.POINTER(sf_savi_features), FP, LL, I, FP, VP, SZ, VP]),
    'sf_savi_features_train_bwd_f32': (I, [C.POINTER(sf_savi_features), FP, LL, FP, C.POINTER(sf_savi_features_grads), I, VP, SZ, VP]),
    'sf_linear_bwd_workspace_bytes': (SZ, [LL, I, I]),
    'sf_linear_bwd_f32': (I, [FP, FP, FP, FP, FP, FP, FP, LL, I, I, I, VP, SZ, VP]),
    'sf_mha_train_fwd_f32': (I, [FP, FP, I, I, I, I, F32, C.c_ulonglong, VP]),
    'sf_mha_train_bwd_f32': (I, [FP, FP, FP, I, I, I, I, F32, C.c_ulonglong, VP]),
    'sf_dropout_f32': (I, [FP, FP, FP, LL, F32, C.c_ulonglong, VP]),
    'sf_adam_flat_f32': (I, [FP, FP, FP, FP, LL, I, F32, F32, F32, F32, VP]),
    'sf_grad_norm_workspace_bytes': (SZ, [LL]),
    'sf_grad_clip_coef_f32': (I, [FP, LL, F32, FP, VP, SZ, VP]),
    'sf_adam_flat_groups_f32': (I, [FP, FP, FP, FP, LL, I, C.POINTER(sf_adam_group), I, F32, F32, F32, FP, VP]),
    'sf_layernorm_bwd_workspace_bytes': (SZ, [I]),
    'sf_layernorm_bwd_f32': (I, [FP, FP, FP, FP, FP, FP, LL, I, F32, VP, SZ, VP]),
    'sf_rollout_train_workspace_bytes': (SZ, [C.POINTER(sf_rollouter), I, I]),
    'sf_rollout_train_fwd_f32': (I, [C.POINTER(sf_rollouter), FP, FP, I, I, F32, C.c_ulonglong, VP, SZ, VP]),
    'sf_rollout_train_bwd_f32': (I, [C.POINTER(sf_rollouter), FP, FP, C.POINTER(sf_rollouter_grads), I, I, F32,
                                     C.c_ulonglong, VP, SZ, VP]),
    'sf_rollout_train_clips_fwd_f32': (I, [C.POINTER(sf_rollouter), FP, I, VP, VP, I, FP, I, I, F32, C.c_ulonglong, VP, SZ, VP]),
    'sf_clip_mse_workspace_bytes': (SZ, [I, I, LL]),
    'sf_clip_mse_f32': (I, [FP, FP, VP, VP, I, I, I, FP, VP, I, F32, FP, VP, I, I, LL, VP, SZ, VP]),
    'sf_clip_frames_f32': (I, [VP, I, VP, VP, I, I, FP, FP, FP, I, I, I, I, VP]),
    'sf_normal_noise_f32': (I, [FP, LL, C.c_ulonglong, C.c_uint, VP]),
    'sf_kernel_sample_workspace_bytes': (SZ, [LL, I]),
    'sf_kernel_sample_fwd_f32': (I, [FP, FP, C.c_ulonglong, C.c_uint, F32, FP, VP, LL, I, VP, SZ, VP]),
    'sf_kernel_sample_bwd_f32': (I, [FP, FP, C.c_ulonglong, C.c_uint, F32, FP, FP, F32, FP, LL, I, VP]),
    'sf_savi_encode_workspace_bytes': (SZ, [C.POINTER(sf_savi_encoder), I]),
    'sf_savi_encode_f32': (I, [C.POINTER(sf_savi_encoder), FP, FP, FP, FP, FP, I, FP, FP, FP, I, I, VP, SZ,
                               VP]),
    'sf_groupnorm1_workspace_bytes': (SZ, [I]),
    'sf_groupnorm1_nhwc_f32': (I, [FP, FP, FP, FP, I, I, I, I, F32, I, I, VP, SZ, VP]),
    'sf_groupnorm1_bwd_workspace_bytes': (SZ, [I, I, I, I]),
    'sf_groupnorm1_nhwc_bwd_f32': (I, [FP, FP, FP, FP, FP, FP, FP, I, I, I, I, F32, I, I, VP, SZ, VP]),
    'sf_slate_attention_f32': (I, [FP, FP, FP, FP, I, I, I, I, I, I, I, I, I, I, VP]),
    'sf_slate_attention_strided_f32': (I, [FP, FP, FP, FP, I, I, I, I, LL, LL, LL, LL, I, I, I, I, I, I, VP]),
    'sf_slate_attention_bwd_workspace_bytes': (SZ, [I, I, I]),
    'sf_slate_attention_bwd_f32': (I, [FP, FP, FP, FP, FP, FP, FP, FP, I, I, I, I, LL, LL, LL, LL, I, I, I, I, I, I, VP, SZ, VP]),
    'sf_slate_attention_train_fwd_f32': (I, [FP, FP, FP, FP, FP, I, I, I, I, LL, LL, LL, LL, I, I, I, I, I, I, F32, C.c_ulonglong, VP]),
    'sf_slate_attention_train_bwd_f32': (I, [FP, FP, FP, FP, FP, FP, FP, FP, FP, I, I, I, I, LL, LL, LL, LL, I, I, I, I, I, I, F32,
                                             C.c_ulonglong, VP, SZ, VP]),
    'sf_embed_tokens_f32': (I, [VP, FP, FP, FP, I, I, I, VP]),
    'sf_argmax_rows_f32': (I, [FP, LL, VP, LL, I, VP]),
    'sf_cross_entropy_f32': (I, [FP, VP, FP, FP, LL, I, VP]),
    'sf_softmax_rows_f32': (I, [FP, FP, F32, FP, LL, I, VP]),
    'sf_softmax_rows_bwd_f32': (I, [FP, FP, F32, FP, LL, I, VP]),
    'sf_log_softmax_rows_f32': (I, [FP, FP, LL, I, VP]),
    'sf_cross_entropy_bwd_f32': (I, [FP, VP, FP, FP, LL, I, VP]),
    'sf_gumbel_softmax_rows_f32': (I, [FP, C.c_ulonglong, F32, FP, LL, I, VP]),
    'sf_slate_generate_workspace_bytes': (SZ, [C.POINTER(sf_slate_decoder), I, I]),
    'sf_slate_generate_f32': (I, [C.POINTER(sf_slate_decoder), FP, I, I, VP, FP, VP, SZ, VP]),
    'sf_slate_step_ok': (I, [C.POINTER(sf_slate_decoder)]),
    'sf_slate_generate_tok_workspace_bytes': (SZ, [C.POINTER(sf_slate_decoder), I, I]),
    'sf_slate_generate_tok_f32': (I, [C.POINTER(sf_slate_decoder), FP, I, I, VP, FP, I, VP, SZ, VP, C.POINTER(I)]),
    'sf_slate_generate_tok_opts_workspace_bytes': (SZ, [C.POINTER(sf_slate_decoder), I, I, C.POINTER(sf_slate_step_opts)]),
    'sf_slate_generate_tok_opts_f32': (I, [C.POINTER(sf_slate_decoder), FP, I, I, VP, FP, I, VP, SZ, VP, C.POINTER(I),
                                           C.POINTER(sf_slate_step_opts)]),
    'sf_gather_rows_f32': (I, [FP, VP, FP, LL, I, LL, VP]),
    'sf_dvae_tokens_ok': (I, [I, I, I, I, I]),
    'sf_dvae_head_packed_bytes': (SZ, [I, I]),
    'sf_dvae_pack_head_weights': (I, [FP, VP, I, I, VP]),
    'sf_dvae_pack_head_weights_host': (I, [VP, VP, I, I]),
    'sf_dvae_patch_embed_f32': (I, [FP, FP, FP, I, I, I, I, VP]),
    'sf_dvae_head_argmax_f32': (I, [FP, LL, VP, FP, VP, VP, LL, I, I, VP]),
    'sf_head_ce_ok': (I, [I, I]),
    'sf_head_ce_packed_bytes': (SZ, [I, I]),
    'sf_head_ce_workspace_bytes': (SZ, [LL]),
    'sf_head_ce_pack_weights': (I, [FP, VP, I, I, VP]),
    'sf_head_ce_pack_weights_host': (I, [VP, VP, I, I]),
    'sf_head_ce_fwd_f32': (I, [FP, LL, VP, VP, VP, FP, I, FP, FP, VP, LL, I, I, VP, SZ, VP]),
    'sf_head_ce_bwd_f32': (I, [FP, LL, VP, VP, VP, FP, I, FP, FP, FP, LL, LL, I, I, VP]),
    'sf_head_ce_wgrad_workspace_bytes': (SZ, [LL, I, I]),
    'sf_head_ce_wgrad_f32': (I, [FP, LL, VP, VP, VP, FP, FP, FP, FP, LL, LL, I, I, I, VP, SZ, VP]),
    'sf_physion_readout_ok': (I, [I, I, I]),
    'sf_physion_readout_fwd_f32': (I, [FP, LL, LL, I, VP, FP, FP, FP, FP, FP, VP, FP, VP, I, I, I, I, I, I, I, VP]),
    'sf_physion_readout_bwd_workspace_bytes': (SZ, [I, I, I]),
    'sf_physion_readout_bwd_f32': (I, [FP, LL, LL, I, VP, FP, FP, FP, FP, VP, VP, FP, FP, FP, FP, I, I, I, I, I, I, VP, SZ, VP]),
    'sf_physion_readout_score_f32': (I, [FP, FP, VP, C.POINTER(F32), I, I, FP, FP, VP, VP, I, I, VP]),
    'sf_phyre_readout_ok': (I, [I, I, I, I, I, I, I]),
    'sf_phyre_readout_workspace_bytes': (SZ, [I, I, I]),
    'sf_phyre_readout_fwd_f32': (I, [FP, LL, LL, I, I, VP, C.POINTER(C.c_int), FP, FP, FP, FP, C.POINTER(sf_tfm_layer), I, I, I, I, FP, FP, FP, FP, FP,
                                     FP, VP, FP, LL, I, I, I, I, VP, SZ, VP]),
    'sf_phyre_auccess_f32': (I, [FP, VP, VP, I, I, VP]),
    'sf_phyre_readout_train_workspace_bytes': (SZ, [C.POINTER(sf_phyre_readout_model), I, I]),
    'sf_phyre_readout_train_fwd_f32': (I, [C.POINTER(sf_phyre_readout_model), FP, LL, LL, I, I, VP, C.POINTER(C.c_int), I, I, F32, C.c_ulonglong, FP,
                                           VP, VP, VP, SZ, VP]),
    'sf_phyre_readout_train_bwd_f32': (I, [C.POINTER(sf_phyre_readout_model), FP, LL, LL, I, I, VP, C.POINTER(C.c_int), I, I, FP,
                                           C.POINTER(sf_phyre_readout_grads), F32, C.c_ulonglong, VP, SZ, VP]),
    'sf_aloe_ok': (I, [I, I, I, I, I, I, I, I]),
    'sf_aloe_workspace_bytes': (SZ, [I, I, I, I, I, I]),
    'sf_aloe_text_table_f32': (I, [FP, FP, FP, FP, I, I, I, VP]),
    'sf_aloe_fwd_f32': (I, [C.POINTER(sf_aloe), FP, LL, LL, I, I, VP, VP, I, VP, VP, I, FP, FP, FP, FP, I, I, FP, VP, I, VP, SZ, VP]),
    'sf_aloe_score_f32': (I, [FP, VP, I, I, FP, FP, VP, I, VP, I, FP, VP, VP, VP]),
    'sf_aloe_train_ok': (I, [I, I, I, I, I, I, I, I]),
    'sf_aloe_train_workspace_bytes': (SZ, [C.POINTER(sf_aloe_model), I]),
    'sf_aloe_train_fwd_f32': (I, [C.POINTER(sf_aloe_model), FP, LL, LL, I, I, VP, VP, I, VP, VP, I, I, F32, C.c_ulonglong, FP, FP, VP, VP, VP, SZ, VP]),
    'sf_aloe_train_bwd_f32': (I, [C.POINTER(sf_aloe_model), FP, LL, LL, I, I, VP, VP, I, VP, VP, I, I, FP, FP, C.POINTER(sf_aloe_grads), F32,
                                  C.c_ulonglong, VP, SZ, VP]),
    'sf_aloe_score_grad_f32': (I, [FP, VP, I, I, FP, FP, I, F32, F32, FP, FP, FP, VP]),
    'sf_packed_linear_bytes': (SZ, [I, I]),
    'sf_pack_linear_weights': (I, [FP, VP, I, I, VP]),
    'sf_attn_packed_bytes': (SZ, [I, I]),
    'sf_pack_attn_weights': (I, [FP, FP, VP, VP, I, I, VP]),
    'sf_ffn_packed_bytes': (SZ, [I, I]),
    'sf_pack_ffn_weights': (I, [FP, FP, VP, VP, I, I, VP]),
    'sf_savi_cnn_workspace_bytes': (SZ, [C.POINTER(sf_savi_encoder), I]),
    'sf_savi_cnn_f32': (I, [C.POINTER(sf_savi_encoder), FP, I, I, I, I, FP, VP, SZ, VP]),
    'sf_savi_encode_pre_f32': (I, [C.POINTER(sf_savi_encoder), FP, FP, I, FP, FP, FP, FP, I, FP, FP, FP, I, I, VP, SZ,
                                   VP]),
    'sf_savi_encode_fork_workspace_bytes': (SZ, [C.POINTER(sf_savi_encoder), I, I]),
    'sf_savi_encode_batched_workspace_bytes': (SZ, [C.POINTER(sf_savi_encoder), I, I]),
    'sf_set_encode_fuse_next': (I, [I]),
    'sf_get_encode_fuse_next': (I, []),
    'sf_set_slot_chain': (I, [I]),
    'sf_get_slot_chain': (I, []),
    'sf_set_slot_attn_planes': (I, [I]),
    'sf_get_slot_attn_planes': (I, []),
    'sf_set_pixel_tok': (I, [I]),
    'sf_get_pixel_tok': (I, []),
    'sf_savi_chain_ok': (I, [C.POINTER(sf_savi_encoder), I, I]),
    'sf_savi_planes_bytes': (SZ, [C.POINTER(sf_savi_encoder), I, I]),
    'sf_savi_features_workspace_bytes': (SZ, [C.POINTER(sf_savi_encoder), I, I]),
    'sf_savi_features_planes_f32': (I, [C.POINTER(sf_savi_encoder), FP, I, I, VP, VP, SZ, VP]),
    'sf_savi_slots_chain_workspace_bytes': (SZ, [C.POINTER(sf_savi_encoder), I]),
    'sf_savi_slots_chain_f32': (I, [C.POINTER(sf_savi_encoder), VP, FP, FP, FP, LL, FP, FP, I, I, I, VP, SZ, VP]),
    'sf_savi_encode_fork_f32': (I, [C.POINTER(sf_savi_encoder), FP, FP, I, FP, FP, FP, FP, I, FP, FP, FP, I, I, VP, SZ,
                                    VP, VP]),
    'sf_kv_producer_workspace_bytes': (SZ, [I, I]),
    'sf_kv_producer_f32': (I, [FP] * 11 + [I, I, I, I, F32, VP, SZ, VP]),
    # device-memory helpers + host-buffer twins (same signatures as the device entry points)
    'sf_device_alloc': (I, [C.POINTER(VP), SZ]),
    'sf_device_free': (I, [VP]),
    'sf_device_upload': (I, [VP, VP, SZ]),
    'sf_device_download': (I, [VP, VP, SZ]),
    'sf_device_synchronize': (I, []),
    'sf_stream_create_cu_mask': (I, [C.POINTER(VP), C.POINTER(C.c_uint), I]),
    'sf_stream_cus': (I, [VP]),
    'sf_stream_set_cus': (I, [VP, I]),
    'sf_debug_spin': (I, [I, VP]),
    'sf_debug_clock_probe': (I, [I, VP, VP]),
    'sf_stream_destroy': (I, [VP]),
    'sf_slot_attn_iter_f32_host': (I, [FP, FP, I, LL, FP, FP, FP, FP, I, I, I, I, F32, F32, VP]),
    'sf_rollout_f32_host': (I, [C.POINTER(sf_rollouter), FP, I, I, I, VP, SZ, VP]),
    'sf_savi_encode_f32_host': (I, [C.POINTER(sf_savi_encoder), FP, FP, FP, FP, FP, I, FP, FP, FP, I, I, VP, SZ,
                                    VP]),
    'sf_savi_decode_f32_host': (I, [C.POINTER(sf_savi_decoder), FP, FP, FP, FP, I, VP, SZ, VP]),
    'sf_seam_timeouts': (I, []),
    'sf_slot_attn_iter_bf16': (I, [VP, VP, I, LL, FP, FP, FP, FP, I, I, I, I, F32, F32, VP]),
    'sf_rollout_bf16': (I, [C.POINTER(sf_rollouter), FP, I, I, I, VP, SZ, VP]),
    'sf_rollout_bf16_host': (I, [C.POINTER(sf_rollouter), FP, I, I, I, VP, SZ, VP]),
    'sf_slot_update_f32_host': (I, [FP, FP, I, FP] + [FP] * 10 + [FP, I, I, I, I, F32, VP]),
    'sf_kv_producer_f32_host': (I, [FP] * 11 + [I, I, I, I, F32, VP, SZ, VP]),
}

_lib = None


class _CaptureGate:
    """Stream capture and kernel launches from other host threads do not mix on this runtime: with a hipGraph capture under way on one thread
    (thread-local capture mode) launches from other threads were seen to return wrong results, `invalid argument`, or to crash hipStreamEndCapture
    (tests/test_rollout_opts_gpu.py::test_options_are_per_call_and_per_thread late in a long process).  So every call into the library holds this
    gate SHARED and a capture (EncodeRolloutPipeline building its graphs) holds it EXCLUSIVE: launches of other threads wait the few milliseconds a
    capture takes; the capturing thread's own calls pass."""

    def __init__(self):
        import threading
        self._cond = threading.Condition()
        self._readers = 0
        self._writer = None
        self._depth = 0
        self._ident = threading.get_ident

    def enter_shared(self):
        me = self._ident()
        with self._cond:
            if self._writer == me:
                return False
            while self._writer is not None:
                self._cond.wait()
            self._readers += 1
            return True

    def exit_shared(self):
        with self._cond:
            self._readers -= 1
            if self._readers == 0:
                self._cond.notify_all()

    def __enter__(self):
        me = self._ident()
        with self._cond:
            if self._writer == me:
                self._depth += 1
                return self
            while self._writer is not None or self._readers > 0:
                self._cond.wait()
            self._writer, self._depth = me, 1
        return self

    def __exit__(self, *exc):
        with self._cond:
            self._depth -= 1
            if self._depth == 0:
                self._writer = None
                self._cond.notify_all()
        return False


CAPTURE_GATE = _CaptureGate()


class _Gated:
    """The loaded library with every entry point behind CAPTURE_GATE (shared)."""

    def __init__(self, h):
        self.__dict__['_h'] = h

    def __getattr__(self, name):
        f = getattr(self._h, name)
        if not callable(f):
            return f
        gate = CAPTURE_GATE

        def call(*a):
            held = gate.enter_shared()
            try:
                return f(*a)
            finally:
                if held:
                    gate.exit_shared()
        call.__name__ = name
        self.__dict__[name] = call
        return call


def lib():
    """Load the HIP library (once).  Fails loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f'{LIB_PATH} not found: the HIP extension is not built. Run '
                '`python -m slotformer_amd.build` (or __graft_entry__.build()). There is no fallback path.')
        try:
            h = C.CDLL(LIB_PATH)
        except OSError as e:  # pragma: no cover
            raise RuntimeError(f'cannot load {LIB_PATH}: {e}') from e
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(h, name)  # AttributeError if the symbol is missing
            fn.restype, fn.argtypes = res, args
        _lib = _Gated(h)
    return _lib


def check(rc):
    if rc != 0:
        msg = lib().sf_last_error_string().decode(errors='replace')
        raise RuntimeError(f'libslotformer_hip: {msg}')
