"""The C-ABI library builds, loads, and exports every symbol include/cmda_hip.h declares (no compute, no GPU)."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, 'include', 'cmda_hip.h')).read()
    return sorted(set(re.findall(r'\bint (cmda_\w+)\(', text)))


def test_header_symbols_exported_by_hip_library():
    lib_path = os.path.join(ROOT, 'cmda_amd', 'libcmda_hip.so')
    if not os.path.exists(lib_path):
        subprocess.check_call(['make', '-j8', 'hip'], cwd=ROOT, stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(lib_path)  # loads without a GPU: no HIP call happens at load time
    syms = declared_symbols()
    assert len(syms) >= 33
    for s in syms:
        assert hasattr(lib, s), f'{s} declared in include/cmda_hip.h but not exported'
    assert lib.cmda_abi_version() == 8


def test_every_exported_entry_point_is_declared():
    srcs = os.path.join(ROOT, 'cmda_amd', 'csrc')
    defined = set()
    for f in os.listdir(srcs):
        if f.endswith('.hip'):
            defined |= set(re.findall(r'extern "C" int (cmda_\w+)\(', open(os.path.join(srcs, f)).read()))
    defined = {d for d in defined if not d.startswith('cmda_debug_')}  # tuning-build-only hooks (-DCMDA_GEMM_TIMING)
    assert defined == set(declared_symbols())


def test_product_has_no_cpu_fallback():
    import torch
    from cmda_amd import _lib, ops
    _lib._unbind_for_tests()
    x = torch.randn(4, 64)
    try:
        ops.layernorm_fwd(x, torch.ones(64), torch.zeros(64), 1e-6)
    except _lib.CmdaError as e:
        assert 'no CPU fallback' in str(e)
    else:
        raise AssertionError('CPU tensors must be rejected by the product path')


# Every entry point of include/cmda_hip.h -> the tests that exercise it AT KERNEL LEVEL (against torch / float64 / a golden file, not
# only inside a full model).  A new entry point fails test_every_entry_point_has_a_kernel_level_test until its test exists and is
# listed here.  Queries map to the test that asserts their value.
_K, _G, _O, _P, _F, _I = 'test_kernels.py', 'test_gemm.py', 'test_optim.py', 'test_pipeline.py', 'test_fdist.py', 'test_image_uda.py'
_R = 'test_row_statistics.py'
KERNEL_TESTS = {
    'cmda_abi_version': ['test_abi.py::test_header_symbols_exported_by_hip_library'],
    'cmda_adamw_step': [f'{_O}::test_adamw_step_stream', f'{_K}::test_classmix_ema_adamw'],
    'cmda_attention_bwd': [f'{_K}::test_fused_attention', f'{_R}::test_attention_two_pass_blocks', f'{_R}::test_attention_dkv_regimes',
                           f'{_R}::test_attention_key_slices', f'{_R}::test_attention_one_hot_addressing',
                           f'{_R}::test_attention_dkv32_accumulates', f'{_R}::test_attention_wide_heads'],
    'cmda_attention_bwd_direct': [f'{_K}::test_fused_attention', f'{_R}::test_attention_dkv_regimes'],
    'cmda_attention_bwd_x3': [f'{_K}::test_fused_attention_split_bf16', f'{_R}::test_attention_two_pass_blocks',
                              f'{_R}::test_attention_dkv_regimes', f'{_R}::test_attention_key_slices',
                              f'{_R}::test_attention_one_hot_addressing', f'{_R}::test_attention_dkv32_accumulates'],
    'cmda_attention_fwd': [f'{_K}::test_fused_attention', f'{_K}::test_fused_attention_eval_keys', f'{_R}::test_attention_two_pass_blocks',
                           f'{_R}::test_attention_key_slices', f'{_R}::test_attention_eval_keys_forward',
                           f'{_R}::test_attention_one_hot_addressing', f'{_R}::test_attention_wide_heads'],
    'cmda_attention_fwd_x3': [f'{_K}::test_fused_attention_split_bf16', f'{_R}::test_attention_two_pass_blocks',
                              f'{_R}::test_attention_key_slices', f'{_R}::test_attention_one_hot_addressing'],
    'cmda_axpby': [f'{_K}::test_permute_cast_colsum_axpby'],
    'cmda_bilinear_bwd': [f'{_K}::test_bilinear'],
    'cmda_bilinear_fwd': [f'{_K}::test_bilinear'],
    'cmda_bn_apply': [f'{_K}::test_bn_apply'],
    'cmda_bn_train_bwd': [f'{_K}::test_batchnorm', f'{_K}::test_batchnorm_shapes', f'{_K}::test_batchnorm_head_shapes'],
    'cmda_bn_train_fwd': [f'{_K}::test_batchnorm', f'{_K}::test_batchnorm_shapes', f'{_K}::test_batchnorm_head_shapes',
                          f'{_K}::test_batchnorm_conditioning', f'{_G}::test_gemm_fused_column_statistics'],
    'cmda_bn_train_fwd2': [f'{_K}::test_bn_train_fwd2', f'{_K}::test_bn_train_fwd2_epilogue_statistics'],
    'cmda_cast_clear': [f'{_K}::test_cast_clear'],
    'cmda_cast_pad_cols': [f'{_K}::test_rows_fill_cast_pad_nchw_pad'],
    'cmda_ce_upsample_bwd': [f'{_K}::test_ce_upsample', f'{_R}::test_ce_upsample_range'],
    'cmda_ce_upsample_fwd': [f'{_K}::test_ce_upsample', f'{_R}::test_ce_upsample_range'],
    'cmda_class_mix': [f'{_K}::test_classmix_ema_adamw'],
    'cmda_class_mix_label': [f'{_K}::test_classmix_ema_adamw'],
    'cmda_color_jitter': [f'{_K}::test_strong_augmentation'],
    'cmda_colsum': [f'{_K}::test_permute_cast_colsum_axpby'],
    'cmda_conv_co1': [f'{_K}::test_conv_co1'],
    'cmda_conv_co3': [f'{_I}::test_conv_co3'],
    'cmda_copy2d': [f'{_K}::test_copy2d'],
    'cmda_crop_flip_resize_f32': [f'{_P}::test_target_pipeline_golden'],
    'cmda_dwconv3x3_bwd_data': [f'{_K}::test_dwconv'],
    'cmda_dwconv3x3_bwd_weight': [f'{_K}::test_dwconv'],
    'cmda_dwconv3x3_fwd': [f'{_K}::test_dwconv', f'{_R}::test_gelu_range_depthwise'],
    'cmda_dwconv3x3_fwd_stats': [f'{_K}::test_dwconv'],
    'cmda_dwconv3x3_gelu_bwd_fused': [f'{_K}::test_dwconv', f'{_R}::test_gelu_range_depthwise'],
    'cmda_dwconv3x3_gelu_bwd_prep': [f'{_K}::test_dwconv', f'{_R}::test_gelu_range_depthwise'],
    'cmda_ema_update': [f'{_O}::test_ema_update_stream', f'{_K}::test_classmix_ema_adamw'],
    'cmda_event_prep': [f'{_P}::test_target_pipeline_golden'],
    'cmda_events_norm': [f'{_K}::test_voxel_golden'],
    'cmda_events_to_voxel_grid': [f'{_K}::test_voxel_golden'],
    'cmda_fdist_fwd_bwd': [f'{_F}::test_fdist_distance_matches_autograd'],
    'cmda_fdist_label_mask': [f'{_F}::test_fdist_label_mask_matches_reference'],
    'cmda_gaussian_blur': [f'{_K}::test_strong_augmentation'],
    'cmda_gemm': [f'{_G}::test_gemm_layouts', f'{_G}::test_gemm_batched_heads', f'{_G}::test_conv_implicit_gemm',
                  f'{_G}::test_gemm_grouped_tile_walk', f'{_R}::test_gelu_range_gemm_epilogue', f'{_R}::test_attention_unfused_path'],
    'cmda_gemm_grouped': [f'{_G}::test_gemm_deferred_grouped_weight_gradients'],
    'cmda_isr_from_gray': [f'{_K}::test_isr_golden'],
    'cmda_isr_gray': [f'{_K}::test_isr_golden'],
    'cmda_layernorm_bwd': [f'{_K}::test_layernorm_single_dtype_entry_points', f'{_R}::test_layernorm_backward_at_ratio_1000'],
    'cmda_layernorm_bwd2': [f'{_K}::test_layernorm', f'{_K}::test_layernorm_fp32_stream_bf16_operands',
                            f'{_K}::test_layernorm_deferred_parameter_gradients', f'{_R}::test_layernorm_backward_at_ratio_1000'],
    'cmda_layernorm_fold_batch': [f'{_K}::test_layernorm_deferred_parameter_gradients'],
    'cmda_layernorm_fwd': [f'{_K}::test_layernorm_single_dtype_entry_points', f'{_R}::test_layernorm_conditioning'],
    'cmda_layernorm_fwd2': [f'{_K}::test_layernorm', f'{_K}::test_layernorm_fp32_stream_bf16_operands', f'{_R}::test_layernorm_conditioning'],
    'cmda_layernorm_slots': [f'{_K}::test_layernorm_single_dtype_entry_points'],
    'cmda_luma_u8': [f'{_P}::test_source_pipeline_golden'],
    'cmda_nchw_to_nhwc_pad': [f'{_K}::test_rows_fill_cast_pad_nchw_pad'],
    'cmda_permute4': [f'{_K}::test_permute_cast_colsum_axpby'],
    'cmda_permute4_batch': [f'{_K}::test_permute4_batch'],
    'cmda_pil_resize_u8': [f'{_P}::test_pil_resize_bit_exact_at_loader_sizes', f'{_P}::test_target_pipeline_golden'],
    'cmda_pseudo_label': [f'{_K}::test_pseudo_label', f'{_R}::test_pseudo_label_range'],
    'cmda_pseudo_weight': [f'{_K}::test_pseudo_label'],
    'cmda_rows_fill': [f'{_K}::test_rows_fill_cast_pad_nchw_pad'],
    'cmda_sample_scale': [f'{_K}::test_sample_scale'],
    'cmda_softmax_bwd': [f'{_K}::test_softmax', f'{_R}::test_softmax_row_lengths', f'{_R}::test_softmax_grid_stride', f'{_R}::test_softmax_range',
                         f'{_R}::test_softmax_refuses_rows_longer_than_1024', f'{_R}::test_attention_unfused_path'],
    'cmda_softmax_fwd': [f'{_K}::test_softmax', f'{_R}::test_softmax_row_lengths', f'{_R}::test_softmax_grid_stride', f'{_R}::test_softmax_range',
                         f'{_R}::test_softmax_refuses_rows_longer_than_1024', f'{_R}::test_attention_unfused_path'],
    'cmda_split_bf16': [f'{_G}::test_gemm_x3_big_three_launch_path'],
    'cmda_time_residual_u8': [f'{_P}::test_source_pipeline_golden'],
    'cmda_upsample_logits_nchw': [f'{_K}::test_upsample_logits_nchw', f'{_R}::test_upsample_logits_range'],
}


def test_every_entry_point_has_a_kernel_level_test():
    declared = set(declared_symbols())
    assert set(KERNEL_TESTS) == declared, f'untested: {sorted(declared - set(KERNEL_TESTS))}, gone: {sorted(set(KERNEL_TESTS) - declared)}'
    here = os.path.dirname(os.path.abspath(__file__))
    defs = {}
    for sym, tests in KERNEL_TESTS.items():
        assert tests, f'{sym}: no test listed'
        for t in tests:
            fname, func = t.split('::')
            if fname not in defs:
                defs[fname] = set(re.findall(r'^def (test_\w+)\(', open(os.path.join(here, fname)).read(), re.M))
            assert func in defs[fname], f'{sym}: {t} does not exist'
