"""ctypes loader for libtdk_hip.so -- the C-ABI kernel library (include/tdk_hip.h).

The library is built in-tree by torch-darktable_amd/build.py.  There is no CPU fallback: if
the library is missing, import of `torch_darktable.torch_darktable_extension` fails, and every
op rejects non-GPU tensors exactly like the reference's TORCH_CHECKs do.
"""

from __future__ import annotations

import ctypes as C
from pathlib import Path

import os

_LIB_PATH = Path(__file__).resolve().parent / 'libtdk_hip.so'
# Measurement knob (profiles/ab_*.sh, profiles/rcd_ab.py): load another build of the same library (an experiment variant under
# variants/) instead of copying it over the in-tree one.  Never set by the product, the tests or bench.py; announced on stderr.
if os.environ.get('TDK_LIB_PATH'):
  _LIB_PATH = Path(os.environ['TDK_LIB_PATH']).resolve()
  import sys as _sys

  print(f'torch_darktable: loading the kernel library from TDK_LIB_PATH={_LIB_PATH}', file=_sys.stderr)

c_void_p, c_int, c_int64, c_uint32, c_float, c_size_t = C.c_void_p, C.c_int, C.c_int64, C.c_uint32, C.c_float, C.c_size_t

# name -> (restype, argtypes); mirrors include/tdk_hip.h declaration by declaration
SIGNATURES = {
  'tdk_abi_version': (c_int, []),
  'tdk_last_error': (C.c_char_p, []),
  'tdk_profile_enable': (c_int, [c_int]),
  'tdk_profile_filter': (c_int, [C.c_char_p]),
  'tdk_profile_report': (c_int64, [C.c_char_p, c_int64]),
  'tdk_encode12_u16': (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p]),
  'tdk_encode12_f32': (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p]),
  'tdk_decode12_f32': (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p]),
  'tdk_decode12_f16': (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p]),
  'tdk_decode12_u16': (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p]),
  'tdk_bilinear5x5': (c_int, [c_void_p, c_void_p, c_int, c_int, c_uint32, c_int, c_void_p]),
  'tdk_ppg_workspace_bytes': (c_size_t, [c_int, c_int, c_float]),
  'tdk_ppg': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_uint32, c_float, c_int, c_void_p]),
  'tdk_rcd_workspace_bytes': (c_size_t, [c_int, c_int]),
  'tdk_rcd': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_uint32, c_int, c_void_p]),
  'tdk_rcd_ex': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_uint32, c_int, C.c_uint, c_void_p]),
  'tdk_decode12_wb_rcd_workspace_bytes': (c_size_t, [c_int, c_int]),
  'tdk_decode12_wb_rcd': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_uint32, c_int, c_int, c_void_p]),
  'tdk_decode12_wb_rcd_ex': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_uint32, c_int, c_int, C.c_uint, c_void_p]),
  'tdk_postprocess_workspace_bytes': (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
  'tdk_postprocess': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_uint32, c_int, c_int, c_int, c_float, c_void_p]),
  'tdk_apply_white_balance': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_uint32, c_void_p]),
  'tdk_wb_collect_samples': (c_int, [c_void_p, c_int, c_int, c_uint32, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
  'tdk_color_op': (c_int, [c_void_p, c_void_p, c_int64, c_int, C.POINTER(c_float), c_void_p, c_void_p]),
  'tdk_compute_luminance': (c_int, [c_void_p, c_void_p, c_int64, c_int, c_float, c_int, c_int, c_void_p]),
  'tdk_modify_luminance': (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_void_p]),
  'tdk_normalize': (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int, c_void_p]),
  'tdk_image_bounds_init': (c_int, [c_void_p, c_void_p]),
  'tdk_image_bounds_accumulate': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p]),
  'tdk_image_bounds_tickets': (c_int, [c_int, c_int, c_int]),
  'tdk_image_bounds': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, C.c_uint, c_int, c_void_p]),
  'tdk_image_metrics_init': (c_int, [c_void_p, c_void_p]),
  'tdk_image_metrics_accumulate': (c_int, [c_void_p, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_int, c_void_p]),
  'tdk_image_metrics_finish': (c_int, [c_void_p, c_void_p, c_void_p]),
  'tdk_image_metrics_accumulate_rows': (c_int, [c_void_p, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_int, c_void_p]),
  'tdk_image_metrics_finish_reset': (c_int, [c_void_p, c_void_p, c_void_p]),
  'tdk_image_metrics': (c_int, [c_void_p, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
  'tdk_tonemap': (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p, c_float, c_float, c_float, c_float, c_int, c_void_p]),
  'tdk_wiener_workspace_bytes': (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
  'tdk_wiener': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p]),
  'tdk_wiener_log_luminance_workspace_bytes': (c_size_t, [c_int, c_int, c_int, c_int]),
  'tdk_wiener_log_luminance': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_float, c_int, c_void_p]),
  'tdk_wiener_log_luminance_lum': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_float, c_int, c_void_p, c_int, c_float, c_void_p]),
  'tdk_bilateral_rgb_lum': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_float, c_float, c_int, c_float, c_int, c_void_p]),
  'tdk_compute_log_luminance_lab': (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_float, c_void_p, c_int, c_void_p]),
  'tdk_wiener_log_luminance_lab': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_float, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
  'tdk_bilateral_lab': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_float, c_float, c_int, C.c_uint, c_void_p]),
  'tdk_bilateral_grid_size': (c_int, [c_int, c_int, c_float, c_float, C.POINTER(c_int)]),
  'tdk_bilateral_workspace_bytes': (c_size_t, [c_int, c_int, c_float, c_float]),
  'tdk_bilateral_prepare': (c_int, [c_void_p, c_int, c_int, c_float, c_float, c_void_p]),
  'tdk_bilateral_ex': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_float, c_float, c_int, C.c_uint, c_void_p]),
  'tdk_bilateral_rgb_ex': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_float, c_float, c_int, c_float, c_int, C.c_uint, c_void_p]),
  'tdk_bilateral': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_float, c_float, c_int, c_void_p]),
  'tdk_bilateral_rgb_workspace_bytes': (c_size_t, [c_int, c_int, c_float, c_float]),
  'tdk_bilateral_rgb': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_float, c_float, c_int, c_float, c_int, c_void_p]),
  'tdk_laplacian_workspace_bytes': (c_size_t, [c_int, c_int, c_int]),
  'tdk_laplacian': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_float, c_float, c_float, c_void_p]),
  'tdk_postprocess_workspace_bytes_ex': (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int]),
  'tdk_postprocess_ex': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_uint32, c_int, c_int, c_int, c_float, c_int, c_void_p]),
  'tdk_apply_white_balance_ex': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_uint32, c_int, c_void_p]),
  'tdk_wb_collect_samples_ex': (c_int, [c_void_p, c_int, c_int, c_uint32, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
  'tdk_color_op_ex': (c_int, [c_void_p, c_void_p, c_int64, c_int, C.POINTER(c_float), c_void_p, c_int, c_void_p]),
  'tdk_laplacian_ex': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_float, c_float, c_float, c_int, c_void_p]),
  'tdk_jpeg_workspace_bytes': (c_size_t, [c_int, c_int, c_int]),
  'tdk_jpeg_encode': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, C.POINTER(c_size_t), c_void_p]),
  'tdk_jpeg_retrieve': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p]),
  'tdk_jpeg_coefficients': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
}

# name -> (restype, argtypes); mirrors include/tdk_hip_ext.h, the entry points beyond the reference's surface
EXT_SIGNATURES = {
  'tdk_ext_abi_version': (c_int, []),
  'tdk_jpeg_device_workspace_bytes': (c_size_t, [c_int, c_int, c_int]),
  'tdk_jpeg_device_max_stream_bytes': (c_size_t, [c_int, c_int, c_int, c_int]),
  'tdk_jpeg_encode_device': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
  'tdk_jpeg_huffman_tables': (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
}

# name -> (restype, argtypes); mirrors include/tdk_hip_denoise.h, the denoisers the reference does not have
DENOISE_SIGNATURES = {
  'tdk_denoise_abi_version': (c_int, []),
  'tdk_nlmeans': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p]),
  'tdk_nlmeans_lds_bytes': (c_size_t, [c_int, c_int, c_int]),
}

# name -> (restype, argtypes); mirrors include/tdk_hip_resample.h, the antialiased scaler
RESAMPLE_SIGNATURES = {
  'tdk_resample_abi_version': (c_int, []),
  'tdk_resample': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
  'tdk_resample_lds_bytes': (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int]),
}

# name -> (restype, argtypes); mirrors include/tdk_hip_warp.h, the parametric warp (map: a host pointer to 18 floats)
WARP_SIGNATURES = {
  'tdk_warp_abi_version': (c_int, []),
  'tdk_warp': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_float, c_int, c_void_p]),
  'tdk_warp_coordinates': (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p]),
  'tdk_warp_lds_bytes': (c_size_t, [c_int, c_int, c_int]),
}

# name -> (restype, argtypes); mirrors include/tdk_hip_raw.h, the sensor correction (black, scale: host pointers to 4 floats each)
RAW_SIGNATURES = {
  'tdk_raw_abi_version': (c_int, []),
  'tdk_raw_prepare': (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_uint32, c_void_p, c_void_p, c_int, c_float, c_float, c_int, c_void_p,
                              c_int, c_int, c_void_p, c_int, c_void_p]),
  'tdk_raw_prepare_lds_bytes': (c_size_t, [c_int, c_int]),
}

# name -> (restype, argtypes); mirrors include/tdk_hip_sharpen.h, the unsharp mask (weights: a host pointer to radius + 1 floats)
SHARPEN_SIGNATURES = {
  'tdk_sharpen_abi_version': (c_int, []),
  'tdk_sharpen_weights': (c_int, [c_float, c_void_p, c_void_p]),
  'tdk_sharpen': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_float, c_float, c_float, c_int, c_void_p]),
  'tdk_sharpen_lds_bytes': (c_size_t, [c_int, c_int, c_int, c_int]),
}

# name -> (restype, argtypes); mirrors include/tdk_hip_wavelet.h, the wavelet denoiser (thresholds: a host pointer to scales * channels floats)
WAVELET_SIGNATURES = {
  'tdk_wavelet_abi_version': (c_int, []),
  'tdk_wavelet_band_norms': (c_int, [c_int, c_void_p]),
  'tdk_wavelet_workspace_bytes': (c_size_t, [c_int, c_int, c_int, c_int]),
  'tdk_wavelet': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p]),
  'tdk_wavelet_lds_bytes': (c_size_t, [c_int, c_int, c_int, c_int]),
}

# name -> (restype, argtypes); mirrors include/tdk_hip_highlights.h, the highlight reconstruction (gains, chroma, stats: device pointers)
HIGHLIGHTS_SIGNATURES = {
  'tdk_highlights_abi_version': (c_int, []),
  'tdk_highlights_workspace_bytes': (c_size_t, []),
  'tdk_highlights_lds_bytes': (c_size_t, [c_int]),
  'tdk_highlights_chrominance': (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_uint32, c_void_p, c_float, c_float, c_int, c_void_p, c_void_p, c_void_p]),
  'tdk_highlights': (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_uint32, c_void_p, c_float, c_float, c_int, c_int, c_void_p, c_void_p]),
}

# name -> (restype, argtypes); mirrors include/tdk_hip_stats.h, the frame statistics (frames, quantiles: host pointers; counts, values: device pointers)
STATS_SIGNATURES = {
  'tdk_framestats_abi_version': (c_int, []),
  'tdk_framestats_workspace_bytes': (c_size_t, [c_int, c_int, c_int]),
  'tdk_framestats_lds_bytes': (c_size_t, [c_int, c_int]),
  'tdk_framestats': (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_uint32, c_int, c_int, c_float, c_float, c_int, c_void_p, c_int, c_void_p,
                             c_void_p, c_void_p]),
}

# name -> (restype, argtypes); mirrors include/tdk_hip_noise.h, the noise profile (frames: a host pointer; counts, model, curve, gains: device pointers)
NOISE_SIGNATURES = {
  'tdk_noise_abi_version': (c_int, []),
  'tdk_noise_workspace_bytes': (c_size_t, [c_int]),
  'tdk_noise_lds_bytes': (c_size_t, [c_int]),
  'tdk_noise_profile': (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_uint32, c_int, c_float, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                c_void_p]),
  'tdk_noise_stabilize': (c_int, [c_void_p, c_int, c_void_p, c_int, c_int64, c_int, c_int, c_uint32, c_void_p, c_void_p, c_float, c_void_p]),
  'tdk_noise_unstabilize': (c_int, [c_void_p, c_int, c_void_p, c_int, c_int64, c_int, c_int, c_uint32, c_void_p, c_void_p, c_float, c_int, c_void_p]),
}

# name -> (restype, argtypes); mirrors include/tdk_hip_temporal.h, the temporal denoiser (src, out, state, model, gains: device pointers)
TEMPORAL_SIGNATURES = {
  'tdk_temporal_abi_version': (c_int, []),
  'tdk_temporal_state_bytes': (c_size_t, [c_int, c_int, c_int]),
  'tdk_temporal_lds_bytes': (c_size_t, [c_int]),
  'tdk_temporal_reset': (c_int, [c_void_p, c_void_p]),
  'tdk_temporal_denoise': (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_uint32, c_void_p, c_void_p, c_int, c_float, c_float,
                                   c_float, c_float, c_float, c_void_p]),
}

# name -> (restype, argtypes); mirrors include/tdk_hip_lut.h, the colour transform (matrix, lut_lo, lut_scale: host pointers; shaper, lut: device pointers)
LUT_SIGNATURES = {
  'tdk_lut_abi_version': (c_int, []),
  'tdk_color_lut': (c_int, [c_void_p, c_int, c_void_p, c_int, c_int64, c_void_p, c_void_p, c_int, c_int, c_float, c_float, c_void_p, c_int, c_void_p, c_void_p,
                            c_int, c_int, c_void_p]),
  'tdk_lut_lds_bytes': (c_size_t, [c_int, c_int, c_int, c_int]),
}

# name -> (restype, argtypes); mirrors include/tdk_hip_motion.h, the motion estimator and the compensated temporal denoiser (every pointer a device pointer)
MOTION_SIGNATURES = {
  'tdk_motion_abi_version': (c_int, []),
  'tdk_motion_pyramid_bytes': (c_size_t, [c_int, c_int, c_int]),
  'tdk_motion_pyramid': (c_int, [c_void_p, c_int, c_int, c_int, c_float, c_int, c_void_p, c_void_p, c_int, c_void_p]),
  'tdk_motion_match': (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p]),
  'tdk_motion_temporal_denoise': (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_uint32, c_void_p, c_void_p, c_int, c_float, c_float,
                                          c_float, c_float, c_float, c_void_p, c_void_p]),
}

# name -> (restype, argtypes); mirrors include/tdk_hip_hdr.h, the exposure-bracket merge (frames: a host array of device pointers; the others device pointers)
HDR_SIGNATURES = {
  'tdk_hdr_abi_version': (c_int, []),
  'tdk_hdr_lds_bytes': (c_size_t, [c_int]),
  'tdk_hdr_merge': (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_uint32, c_void_p, c_int, c_void_p, c_int, c_float, c_float, c_float,
                            c_float, c_float, c_void_p]),
}

# name -> (restype, argtypes); mirrors include/tdk_hip_hdralign.h, the aligned bracket merge (frames: a host array of device pointers; the others device pointers)
HDRALIGN_SIGNATURES = {
  'tdk_hdralign_abi_version': (c_int, []),
  'tdk_hdralign_lds_bytes': (c_size_t, [c_int]),
  'tdk_hdralign_pyramid': (c_int, [c_void_p, c_int, c_int, c_int, c_float, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p]),
  'tdk_hdralign_merge': (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_uint32, c_void_p, c_int, c_void_p, c_int, c_float, c_float,
                                 c_float, c_float, c_float, c_void_p, c_void_p]),
}

# name -> (restype, argtypes); mirrors include/tdk_hip_ca.h, the chromatic aberration (frames: a host array of device pointers; the others device pointers)
CA_SIGNATURES = {
  'tdk_ca_abi_version': (c_int, []),
  'tdk_ca_lds_bytes': (c_size_t, [c_int, c_int]),
  'tdk_ca_correct': (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_uint32, c_void_p, c_float, c_float, c_float, c_int, c_void_p]),
  'tdk_ca_workspace_bytes': (c_size_t, [c_int, c_int, c_int]),
  'tdk_ca_estimate': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_uint32, c_void_p, c_int, c_float, c_int, c_float, c_float, c_float, c_float, c_void_p, c_void_p,
                              c_void_p]),
}

# name -> (restype, argtypes); mirrors include/tdk_hip_rawcodec.h, the lossless raw codec (every pointer a device pointer)
RAWCODEC_SIGNATURES = {
  'tdk_rawcodec_abi_version': (c_int, []),
  'tdk_rawcodec_table_bytes': (c_size_t, [c_int, c_int]),
  'tdk_rawcodec_max_stream_bytes': (c_size_t, [c_int, c_int]),
  'tdk_rawcodec_encode': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p, c_void_p]),
  'tdk_rawcodec_decode': (c_int, [c_void_p, c_size_t, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
}

# name -> (restype, argtypes); mirrors include/tdk_hip_toneeq.h, the tone equalizer (weights: a host pointer to 3 floats; the others device pointers)
TONEEQ_SIGNATURES = {
  'tdk_toneeq_abi_version': (c_int, []),
  'tdk_toneeq_workspace_bytes': (c_size_t, [c_int, c_int, c_int]),
  'tdk_toneeq_lds_bytes': (c_size_t, [c_int, c_int, c_int]),
  'tdk_toneeq': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p, c_int, c_void_p]),
}

# name -> (restype, argtypes); mirrors include/tdk_hip_wiener.h, the Wiener entry points with flags and the strip kernel's interior rule (host queries)
WIENER_SIGNATURES = {
  'tdk_wiener_abi_version': (c_int, []),
  'tdk_wiener_ex': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_uint32, c_void_p]),
  'tdk_wiener_log_luminance_lab_ex': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_float, c_void_p, c_int, c_void_p, c_void_p, c_uint32,
                                              c_void_p]),
  'tdk_wiener_strip_interior': (c_int, [c_int, c_int, c_int, c_int, c_int]),
  'tdk_wiener_strip_order': (c_int, [c_int, c_int, c_int, c_int]),
}

# name -> (restype, argtypes); mirrors include/tdk_hip_tables.h, the point operators of binary16 pixels that go through a table over the 65 536 codes
TABLES_SIGNATURES = {
  'tdk_tables_abi_version': (c_int, []),
  'tdk_tonemap_ex': (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p, c_float, c_float, c_float, c_float, c_int, c_void_p, c_uint32, c_void_p]),
}

# name -> (restype, argtypes); mirrors include/tdk_hip_dehaze.h, the haze removal (weights: a host pointer to 3 floats; the others device pointers)
DEHAZE_SIGNATURES = {
  'tdk_dehaze_abi_version': (c_int, []),
  'tdk_dehaze_workspace_bytes': (c_size_t, [c_int, c_int, c_int]),
  'tdk_dehaze_lds_bytes': (c_size_t, [c_int, c_int, c_int, c_int]),
  'tdk_dehaze_ambient': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
  'tdk_dehaze': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_float, c_float, c_void_p,
                         c_int, c_void_p]),
}

# name -> (restype, argtypes); mirrors include/tdk_hip_deconv.h, the capture sharpening (weights, luma: host pointers; the others device pointers)
DECONV_SIGNATURES = {
  'tdk_deconv_abi_version': (c_int, []),
  'tdk_deconv_weights': (c_int, [c_float, c_void_p, c_void_p]),
  'tdk_deconv_fused_iterations': (c_int, [c_int]),
  'tdk_deconv_workspace_bytes': (c_size_t, [c_int, c_int, c_int, c_int]),
  'tdk_deconv_lds_bytes': (c_size_t, [c_int, c_int, c_int, c_int]),
  'tdk_deconv': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_float, c_float, c_void_p, c_int, c_void_p]),
}

# name -> (restype, argtypes); mirrors include/tdk_hip_lmmse.h, the demosaic for noisy frames (device pointers)
LMMSE_SIGNATURES = {
  'tdk_lmmse_abi_version': (c_int, []),
  'tdk_lmmse_lds_bytes': (c_size_t, [c_int, c_int, c_int]),
  'tdk_lmmse': (c_int, [c_void_p, c_void_p, c_int, c_int, c_uint32, c_int, c_int, c_int, c_void_p]),
}

# name -> (restype, argtypes); mirrors include/tdk_hip_defringe.h, the purple-fringe removal (weights: a host pointer to radius + 1 floats; the others device pointers)
DEFRINGE_SIGNATURES = {
  'tdk_defringe_abi_version': (c_int, []),
  'tdk_defringe_weights': (c_int, [c_float, c_void_p, c_void_p]),
  'tdk_defringe_workspace_bytes': (c_size_t, [c_int, c_int]),
  'tdk_defringe_lds_bytes': (c_size_t, [c_int, c_int, c_int, c_int]),
  'tdk_defringe': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_float, c_float, c_int, c_void_p]),
}

# name -> (restype, argtypes); mirrors include/tdk_hip_scaled.h, the reduced-size demosaic (tile_width, tile_height: host pointers; the others device pointers)
SCALED_SIGNATURES = {
  'tdk_scaled_abi_version': (c_int, []),
  'tdk_demosaic_scaled_lds_bytes': (c_size_t, [c_int, c_int, c_int, c_int]),
  'tdk_demosaic_scaled_tile': (c_int, [c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
  'tdk_demosaic_scaled': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_uint32, c_int, c_int, c_void_p]),
  'tdk_decode12_demosaic_scaled': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_uint32, c_int, c_int, c_void_p]),
}

# name -> (restype, argtypes); mirrors include/tdk_hip_filmic.h, the scene-referred tone mapping (weights: a host pointer to 3 floats; the others device pointers)
FILMIC_SIGNATURES = {
  'tdk_filmic_abi_version': (c_int, []),
  'tdk_filmic_lds_bytes': (c_size_t, []),
  'tdk_filmic': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_void_p, c_int, c_void_p]),
}

# one row per public header, in the order of build.HEADERS:
# (header, its signature table, its version function, the version this package was written against, its name in the ImportError)
HEADERS = (
  ('tdk_hip.h', SIGNATURES, 'tdk_abi_version', 4, 'ABI'),
  ('tdk_hip_ext.h', EXT_SIGNATURES, 'tdk_ext_abi_version', 1, 'extension ABI'),
  ('tdk_hip_denoise.h', DENOISE_SIGNATURES, 'tdk_denoise_abi_version', 1, 'denoise ABI'),
  ('tdk_hip_resample.h', RESAMPLE_SIGNATURES, 'tdk_resample_abi_version', 1, 'resample ABI'),
  ('tdk_hip_warp.h', WARP_SIGNATURES, 'tdk_warp_abi_version', 1, 'warp ABI'),
  ('tdk_hip_raw.h', RAW_SIGNATURES, 'tdk_raw_abi_version', 1, 'raw ABI'),
  ('tdk_hip_sharpen.h', SHARPEN_SIGNATURES, 'tdk_sharpen_abi_version', 1, 'sharpen ABI'),
  ('tdk_hip_wavelet.h', WAVELET_SIGNATURES, 'tdk_wavelet_abi_version', 1, 'wavelet ABI'),
  ('tdk_hip_highlights.h', HIGHLIGHTS_SIGNATURES, 'tdk_highlights_abi_version', 1, 'highlights ABI'),
  ('tdk_hip_temporal.h', TEMPORAL_SIGNATURES, 'tdk_temporal_abi_version', 1, 'temporal ABI'),
  ('tdk_hip_motion.h', MOTION_SIGNATURES, 'tdk_motion_abi_version', 1, 'motion ABI'),
  ('tdk_hip_hdr.h', HDR_SIGNATURES, 'tdk_hdr_abi_version', 1, 'hdr ABI'),
  ('tdk_hip_hdralign.h', HDRALIGN_SIGNATURES, 'tdk_hdralign_abi_version', 1, 'hdr alignment ABI'),
  ('tdk_hip_ca.h', CA_SIGNATURES, 'tdk_ca_abi_version', 1, 'chromatic aberration ABI'),
  ('tdk_hip_rawcodec.h', RAWCODEC_SIGNATURES, 'tdk_rawcodec_abi_version', 1, 'raw codec ABI'),
  ('tdk_hip_toneeq.h', TONEEQ_SIGNATURES, 'tdk_toneeq_abi_version', 1, 'tone equalizer ABI'),
  ('tdk_hip_dehaze.h', DEHAZE_SIGNATURES, 'tdk_dehaze_abi_version', 1, 'dehaze ABI'),
  ('tdk_hip_filmic.h', FILMIC_SIGNATURES, 'tdk_filmic_abi_version', 1, 'filmic ABI'),
  ('tdk_hip_deconv.h', DECONV_SIGNATURES, 'tdk_deconv_abi_version', 1, 'deconvolution ABI'),
  ('tdk_hip_lmmse.h', LMMSE_SIGNATURES, 'tdk_lmmse_abi_version', 1, 'LMMSE demosaic ABI'),
  ('tdk_hip_defringe.h', DEFRINGE_SIGNATURES, 'tdk_defringe_abi_version', 1, 'defringe ABI'),
  ('tdk_hip_scaled.h', SCALED_SIGNATURES, 'tdk_scaled_abi_version', 1, 'scaled demosaic ABI'),
  ('tdk_hip_wiener.h', WIENER_SIGNATURES, 'tdk_wiener_abi_version', 1, 'wiener ABI'),
  ('tdk_hip_tables.h', TABLES_SIGNATURES, 'tdk_tables_abi_version', 1, 'tables ABI'),
  ('tdk_hip_stats.h', STATS_SIGNATURES, 'tdk_framestats_abi_version', 1, 'stats ABI'),
  ('tdk_hip_noise.h', NOISE_SIGNATURES, 'tdk_noise_abi_version', 1, 'noise ABI'),
  ('tdk_hip_lut.h', LUT_SIGNATURES, 'tdk_lut_abi_version', 1, 'lut ABI'),
)
ALL_SIGNATURES = tuple(table for _, table, _, _, _ in HEADERS)
ABI_VERSIONS = {version_fn: (expected, label) for _, _, version_fn, expected, label in HEADERS}

TDK_F32, TDK_F16 = 0, 1
TDK_U8 = 2  # include/tdk_hip_resample.h: taken by tdk_resample and tdk_warp only
TDK_WARP_DIRECT = 1  # include/tdk_hip_warp.h: flags of tdk_warp
# include/tdk_hip_raw.h: src_format and defects of tdk_raw_prepare
TDK_RAW_PACKED12, TDK_RAW_PACKED12_IDS, TDK_RAW_U16, TDK_RAW_F32, TDK_RAW_F16 = 0, 1, 2, 3, 4
TDK_RAW_HOT, TDK_RAW_DEAD = 1, 2
TDK_SHARPEN_LUMA, TDK_SHARPEN_LIMIT = 1, 2  # include/tdk_hip_sharpen.h: flags of tdk_sharpen
TDK_SHARPEN_MAX_RADIUS = 12
TDK_WAVELET_YCC = 1  # include/tdk_hip_wavelet.h: flags of tdk_wavelet
TDK_WAVELET_MAX_SCALES = 5
TDK_HL_CLIP, TDK_HL_OPPOSED = 0, 1  # include/tdk_hip_highlights.h: mode of tdk_highlights
TDK_LUT_TETRAHEDRAL, TDK_LUT_TRILINEAR = 0, 1  # include/tdk_hip_lut.h: interp of tdk_color_lut
TDK_LUT_GLOBAL = 1  # ... and its flag
TDK_LUT_MAX_SHAPER, TDK_LUT_MAX_SIZE = 1024, 65
TDK_U16 = 3  # include/tdk_hip_stats.h: taken by tdk_framestats only
TDK_STATS_MAX_BINS, TDK_STATS_MAX_FRAMES, TDK_STATS_MAX_QUANTILES = 1024, 16, 8
TDK_STATS_GRID, TDK_STATS_CHUNK = 512, 8192  # workgroups of the gather launch, pixels of a workgroup per step
# include/tdk_hip_noise.h: limits of tdk_noise_profile, the workgroups of its gather launch and the bytes of a row they take per step
TDK_NOISE_MAX_BINS, TDK_NOISE_MAX_FRAMES, TDK_NOISE_LEVELS = 32, 16, 128
TDK_NOISE_GRID, TDK_NOISE_STRIP_BYTES = 512, 512
TDK_NOISE_MEDIAN_FACTOR = 0.9796
TDK_NOISE_ALGEBRAIC, TDK_NOISE_UNBIASED = 0, 1  # inverse of tdk_noise_unstabilize
# include/tdk_hip_temporal.h: the output tile of a workgroup of tdk_temporal_denoise, the head of its state, the largest n_max
TDK_TEMPORAL_TILE_W, TDK_TEMPORAL_TILE_H = 64, 32
TDK_TEMPORAL_HEAD_BYTES, TDK_TEMPORAL_MAX_FRAMES = 16, 64
# include/tdk_hip_motion.h: the tile of one displacement, the limits of tdk_motion_pyramid and tdk_motion_match
TDK_MOTION_TILE_W, TDK_MOTION_TILE_H = 64, 32
TDK_MOTION_MAX_LEVELS, TDK_MOTION_MAX_SEARCH, TDK_MOTION_MAX_DISPLACEMENT, TDK_MOTION_MAX_ZERO_BIAS = 4, 4, 78, 65535
# include/tdk_hip_hdr.h: the output tile of a workgroup of tdk_hdr_merge, the largest bracket
TDK_HDR_TILE_W, TDK_HDR_TILE_H = 32, 32
TDK_HDR_MAX_FRAMES = 8
# include/tdk_hip_ca.h: the largest displacement, the output tile of a workgroup of tdk_ca_correct, interp, fit, the limits of tdk_ca_estimate
TDK_CA_MAX_SHIFT = 8
TDK_CA_TILE_W, TDK_CA_TILE_H = 64, 32
TDK_CA_BILINEAR, TDK_CA_BICUBIC = 0, 1
TDK_CA_LINEAR, TDK_CA_POLY3 = 0, 1
TDK_CA_MAX_FRAMES, TDK_CA_SUMS, TDK_CA_MIN_SITES = 16, 17, 16
TDK_CA_QSCALE, TDK_CA_QMAX = 65535.0, 65535
# include/tdk_hip_rawcodec.h: the format's constants and the bits of the status of tdk_rawcodec_decode
TDK_RAWCODEC_FORMAT_VERSION, TDK_RAWCODEC_HEADER_BYTES, TDK_RAWCODEC_SPAN, TDK_RAWCODEC_SEGMENT, TDK_RAWCODEC_MAX_SITES = 1, 32, 64, 512, 1 << 30
TDK_RAWCODEC_BAD_MAGIC, TDK_RAWCODEC_BAD_SIZE, TDK_RAWCODEC_BAD_TABLES = 1, 2, 4
# include/tdk_hip_toneeq.h: the gain table (exposures covered, nodes per octave, entries) and the largest radius
TDK_TONEEQ_EV_MIN, TDK_TONEEQ_EV_MAX, TDK_TONEEQ_STEPS, TDK_TONEEQ_TABLE = -16, 4, 32, 641
TDK_TONEEQ_MAX_RADIUS = 8
# include/tdk_hip_dehaze.h: the largest radii and grid, the float32 cell planes of the workspace
TDK_DEHAZE_MAX_DARK_RADIUS, TDK_DEHAZE_MAX_RADIUS, TDK_DEHAZE_MAX_CELLS, TDK_DEHAZE_PLANES = 4, 8, 1 << 24, 10
# include/tdk_hip_deconv.h: the flag of tdk_deconv, the bits of its fused count, the limits, the tile of a workgroup
TDK_DECONV_MASK, TDK_DECONV_FUSE_SHIFT, TDK_DECONV_FUSE_MASK = 1, 8, 0xF00
TDK_DECONV_MAX_RADIUS, TDK_DECONV_MAX_ITERATIONS, TDK_DECONV_MAX_FUSED, TDK_DECONV_TILE = 6, 50, 4, 32
# include/tdk_hip_lmmse.h: the flag of tdk_lmmse, the output tile of a workgroup, what a stored site depends on, the sizes taken
TDK_LMMSE_LINEAR = 1
TDK_LMMSE_TILE_W, TDK_LMMSE_TILE_H, TDK_LMMSE_APRON = 32, 32, 11
TDK_LMMSE_MIN_SIZE, TDK_LMMSE_MAX_SIZE = 2, 65535
# include/tdk_hip_defringe.h: the flags of tdk_defringe, the bits of its workgroup cap, the limits, the tile of a workgroup, the statistic's scale and cap
TDK_DEFRINGE_GLOBAL, TDK_DEFRINGE_LINEAR, TDK_DEFRINGE_STATIC = 0, 1, 2
TDK_DEFRINGE_GROUPS_SHIFT, TDK_DEFRINGE_GROUPS_MASK = 8, 0x7FF00
TDK_DEFRINGE_MAX_RADIUS, TDK_DEFRINGE_MAX_SAMPLE_RADIUS, TDK_DEFRINGE_MAX_GROUPS, TDK_DEFRINGE_TILE = 12, 8, 1024, 32
TDK_DEFRINGE_STAT_SCALE, TDK_DEFRINGE_STAT_CAP = 1048576, 1024
# include/tdk_hip_filmic.h: the curve tables (exposures covered, nodes per octave, entries), the encoding table, the norms
TDK_FILMIC_EV_MIN, TDK_FILMIC_EV_MAX, TDK_FILMIC_STEPS, TDK_FILMIC_TABLE = -20, 12, 32, 1025
TDK_FILMIC_ENC_EV_MIN, TDK_FILMIC_ENC_TABLE = -16, 513
TDK_FILMIC_MAX, TDK_FILMIC_LUMA, TDK_FILMIC_POWER, TDK_FILMIC_NONE = 0, 1, 2, 3
TDK_SCALED_MIN_RATIO, TDK_SCALED_MAX_RATIO, TDK_SCALED_MAX_TAPS = 2, 16, 32  # include/tdk_hip_scaled.h: the ratios of tdk_demosaic_scaled, its taps per axis
TDK_WIENER_GENERAL_BODY = 1  # include/tdk_hip_wiener.h: flags of tdk_wiener_ex and tdk_wiener_log_luminance_lab_ex
TDK_TONEMAP_TABLE_BYTES, TDK_TONEMAP_DIRECT = 3 * 65536, 1  # include/tdk_hip_tables.h: the table of tdk_tonemap_ex and its flag


def load() -> C.CDLL:
  if not _LIB_PATH.exists():
    raise ImportError(
      f'{_LIB_PATH} is missing: build the HIP kernel library first (python torch-darktable_amd/build.py). '
      'torch_darktable has no CPU or pure-PyTorch fallback.'
    )
  lib = C.CDLL(str(_LIB_PATH))
  for table in ALL_SIGNATURES:
    for name, (restype, argtypes) in table.items():
      fn = getattr(lib, name)  # AttributeError here == ABI mismatch between header and library
      fn.restype = restype
      fn.argtypes = argtypes
  for name, (expected, label) in ABI_VERSIONS.items():
    if getattr(lib, name)() != expected:
      raise ImportError(f'libtdk_hip.so {label} version {getattr(lib, name)()} != {expected}')
  return lib


lib = load()


def check(status: int) -> None:
  """Map a tdk_status to the reference's error type (TORCH_CHECK -> RuntimeError)."""
  if status != 0:
    raise RuntimeError(lib.tdk_last_error().decode('utf-8', 'replace'))


def profile_enable(on: bool, only: str | None = None) -> None:
  """Switch the library's per-kernel event timer on (clearing old records) or off.  `only`
  restricts it to kernels whose name contains that string (None: every launch)."""
  check(lib.tdk_profile_filter(only.encode() if only else None))
  check(lib.tdk_profile_enable(int(on)))


def profile_report() -> dict:
  """{kernel name: (launches, total device ms)} for everything launched since profile_enable(True)."""
  need = lib.tdk_profile_report(None, 0)
  buf = C.create_string_buffer(int(need) + 16)
  lib.tdk_profile_report(buf, len(buf))
  out = {}
  for line in buf.value.decode().splitlines():
    name, count, ms = line.rsplit(' ', 2)
    out[name] = (int(count), float(ms))
  return out
