// The entry tables: one row per stream entry `int entry(const ARGS*, void* stream)` of include/wavjepa_hip.h (and, under WJ_LAB, of
// include/wavjepa_hip_lab.h), then of each side library's header.  WJ_ABI_QUERIES (csrc/abi_queries.h) generates a library's struct-size
// and workspace queries and a compile-time check of every row against the header's prototype from its table; nothing else lists the
// entries.  Every library has an <X>_ENTRIES table and an <X>_OTHER_STRUCTS list (the argument structs of its header that no stream
// entry takes; it may be empty).
//   E(entry, ARGS)        the entry takes no scratch: the query answers 0
//   W(entry, ARGS, rule)  `int64_t rule(const ARGS*)`, defined beside the launch that consumes the scratch, answers the bytes for the
//                         dimensions in ARGS (pointers ignored), -1 for dimensions it refuses; it never faults
#pragma once

#ifdef WJ_LAB
#define WJ_LAB_ENTRIES(E, W) E(wj_collective_footprint, wj_collective_footprint_args)
#else
#define WJ_LAB_ENTRIES(E, W)
#endif

#define WJ_STREAM_ENTRIES(E, W)                                                        \
    W(wj_gemm_bf16, wj_gemm_args, wj_gemm_ws_bytes)                                    \
    E(wj_gemm_mxfp8, wj_gemm_fp8_args)                                                 \
    E(wj_quantize_mxfp8, wj_quantize_fp8_args)                                         \
    W(wj_wgrad_grouped, wj_wgrad_group_args, wj_wgrad_group_ws_bytes)                  \
    E(wj_layernorm_fwd, wj_ln_fwd_args)                                                \
    W(wj_layernorm_bwd, wj_ln_bwd_args, wj_ln_bwd_ws_bytes)                            \
    W(wj_colsum_bf16, wj_colsum_args, wj_colsum_bf16_ws_bytes)                         \
    E(wj_colsum_f32, wj_colsum_args)                                                   \
    E(wj_colsum_f32_group, wj_colsum_group_args)                                       \
    E(wj_layernorm_pre_fwd, wj_ln_pre_fwd_args)                                        \
    W(wj_layernorm_pre_bwd, wj_ln_pre_bwd_args, wj_ln_pre_bwd_ws_bytes)                \
    E(wj_attn_fwd, wj_attn_fwd_args)                                                   \
    W(wj_attn_bwd, wj_attn_bwd_args, wj_attn_bwd_ws_bytes)                             \
    E(wj_attn_stream_fwd, wj_attn_fwd_args)                                            \
    W(wj_attn_stream_bwd, wj_attn_bwd_args, wj_attn_bwd_ws_bytes)                      \
    W(wj_conv0_gn_gelu_fwd, wj_conv0_fwd_args, wj_conv0_fwd_ws_bytes)                  \
    W(wj_conv0_gn_gelu_bwd, wj_conv0_bwd_args, wj_conv0_bwd_ws_bytes)                  \
    E(wj_gelu_bwd_bf16, wj_gelu_bwd_args)                                              \
    E(wj_conv_ln_gelu_fwd, wj_conv_ln_fwd_args)                                        \
    W(wj_conv_ln_gelu_bwd, wj_conv_ln_bwd_args, wj_conv_ln_bwd_ws_bytes)               \
    E(wj_conv0_ln_gelu_fwd, wj_conv0_ln_fwd_args)                                      \
    W(wj_conv0_ln_gelu_bwd, wj_conv0_ln_bwd_args, wj_conv0_ln_bwd_ws_bytes)            \
    E(wj_spin, wj_spin_args)                                                           \
    E(wj_zero_rows, wj_zero_rows_args)                                                 \
    E(wj_conv_weight_layout, wj_conv_w_args)                                           \
    E(wj_add_pos, wj_add_pos_args)                                                     \
    E(wj_mask_gather_rows, wj_gather_args)                                             \
    E(wj_mask_scatter_fill_pos, wj_scatter_fill_args)                                  \
    W(wj_mask_scatter_fill_pos_bwd, wj_scatter_fill_bwd_args, wj_scatter_fill_bwd_ws_bytes) \
    E(wj_unmask_rows_f32, wj_unmask_rows_args)                                         \
    E(wj_instnorm_accumulate, wj_instnorm_args)                                        \
    E(wj_instnorm_mean, wj_instnorm_mean_args)                                         \
    W(wj_masked_mse, wj_mse_args, wj_masked_mse_ws_bytes)                              \
    W(wj_masked_loss, wj_loss_args, wj_masked_loss_ws_bytes)                           \
    E(wj_ema_update, wj_ema_args)                                                      \
    W(wj_grad_sumsq, wj_sumsq_args, wj_grad_sumsq_ws_bytes)                            \
    E(wj_adamw_step, wj_adamw_args)                                                    \
    E(wj_transpose_bf16, wj_transpose_args)                                            \
    E(wj_rccl_bucket_allreduce_launch, wj_rccl_launch_args)                            \
    E(wj_rccl_bucket_allreduce_wait, wj_rccl_wait_args)                                \
    E(wj_cast_f32_to_bf16, wj_cast_args)                                               \
    E(wj_crop_normalize_bf16, wj_crop_args)                                            \
    W(wj_rir_convolve, wj_rir_conv_args, wj_rir_conv_ws_bytes)                         \
    W(wj_snr_mix, wj_snr_mix_args, wj_snr_mix_ws_bytes)                                \
    E(wj_resample_fir, wj_resample_args)                                               \
    W(wj_mse_groups, wj_mse_groups_args, wj_mse_groups_ws_bytes)                       \
    W(wj_audio_prepare, wj_audio_prepare_args, wj_audio_prepare_ws_bytes)              \
    W(wj_noise_prepare, wj_noise_prepare_args, wj_noise_prepare_ws_bytes)              \
    WJ_LAB_ENTRIES(E, W)

#define WJ_OTHER_STRUCTS(S) S(wj_rccl_init_args)

// libwavjepa_hip_dropout.so (include/wavjepa_hip_dropout.h, csrc/dropout.hip)
#define WJ_DROPOUT_ENTRIES(E, W)                                                       \
    E(wj_dropout_rows, wj_dropout_rows_args)                                           \
    E(wj_layernorm_fwd_drop, wj_ln_fwd_drop_args)                                      \
    W(wj_layernorm_bwd_drop, wj_ln_bwd_drop_args, wj_ln_bwd_drop_ws_bytes)             \
    E(wj_attn_stream_fwd_drop, wj_attn_fwd_drop_args)                                  \
    W(wj_attn_stream_bwd_drop, wj_attn_bwd_drop_args, wj_attn_bwd_drop_ws_bytes)
#define WJ_DROPOUT_OTHER_STRUCTS(S) S(wj_dropout_args)

// libwavjepa_hip_act.so (include/wavjepa_hip_act.h, csrc/gemm.hip under WJ_ACT_LIB; the forward GELU forms take no scratch)
#define WJ_ACT_ENTRIES(E, W)                                                           \
    E(wj_gemm_bf16_act, wj_gemm_act_args)
#define WJ_ACT_OTHER_STRUCTS(S)

// libwavjepa_hip_monitor.so (include/wavjepa_hip_monitor.h, csrc/monitor.hip)
#define WJ_MONITOR_ENTRIES(E, W)                                                       \
    W(wj_masked_moments, wj_moments_args, wj_masked_moments_ws_bytes)
#define WJ_MONITOR_OTHER_STRUCTS(S)

// libwavjepa_hip_optim.so (include/wavjepa_hip_optim.h, csrc/optim.hip)
#define WJ_OPTIM_ENTRIES(E, W)                                                         \
    E(wj_adamw_groups_step, wj_adamw_groups_args)
#define WJ_OPTIM_OTHER_STRUCTS(S)
