"""torch_darktable for AMD Instinct MI355X: RAW image-signal-processing ops as hand-written HIP kernels.

Drop-in for the public surface of uc-vision/torch-darktable's hot path (debayer, denoise,
local_contrast, tonemap, color_conversion, plus the codec and white balance around it)."""

from . import bayer, chromatic, color_conversion, colorlut, debayer, deconvolve, defringe, dehaze, denoise, device_jpeg, extension, filmic, framestats, hdralign, hdrmerge, highlights, jpeg, lmmse, local_contrast, motion, nlmeans, noiseprofile, rawcodec, rawprepare, resample, scaled_demosaic, sharpen, temporal, toneequal, tonemap, warp, wavelet, white_balance
from .bayer import BayerPattern, PackedFormat, load_as_bayer, rgb_to_bayer
from .chromatic import ChromaticAberration
from .color_conversion import (color_transform_3x3, compute_log_luminance, compute_luminance, lab_to_rgb, lab_to_xyz, modify_hsl,
                               modify_log_luminance, modify_luminance, modify_vibrance, rgb_to_lab, rgb_to_xyz, xyz_to_lab, xyz_to_rgb)
from .colorlut import ColorLUT
from .debayer import (PPG, RCD, Bilinear5x5, PostProcess, bilinear5x5_demosaic, decode12, decode12_float, decode12_half, decode12_u16,
                      encode, encode12_float, encode12_u16)
from .deconvolve import Deconvolve
from .defringe import Defringe
from .dehaze import Dehaze
from .denoise import Wiener, estimate_channel_noise
from .device_jpeg import DeviceJpeg, DeviceJpegResult
from .filmic import Filmic
from .framestats import FrameStatistics, FrameStats
from .hdralign import MotionHdrMerge
from .hdrmerge import HdrMerge
from .highlights import Highlights
from .jpeg import InputFormat, Jpeg, JpegException, Subsampling
from .lmmse import LMMSE
from .local_contrast import Bilateral, Laplacian, LaplacianParams
from .motion import MotionEstimate, MotionTemporalDenoise
from .nlmeans import NLMeans
from .noiseprofile import NoiseModel, NoiseProfile, NoiseStatistics
from .rawcodec import RawCodec, RawCodecResult
from .rawprepare import RawPrepare
from .resample import Resize
from .scaled_demosaic import ScaledDemosaic
from .sharpen import Sharpen
from .temporal import TemporalDenoise
from .toneequal import ToneEqualizer
from .tonemap import (TonemapParameters, aces_tonemap, compute_image_bounds, compute_image_metrics, linear_tonemap, metrics_from_dict,
                      metrics_to_dict, print_metrics, reinhard_tonemap)
from .warp import Warp
from .wavelet import Wavelet
from .white_balance import apply_white_balance, estimate_white_balance

__all__ = [
    'PPG', 'RCD', 'BayerPattern', 'Bilateral', 'Bilinear5x5', 'ChromaticAberration', 'ColorLUT', 'Deconvolve', 'Defringe', 'Dehaze', 'DeviceJpeg', 'DeviceJpegResult', 'Filmic', 'FrameStatistics', 'FrameStats', 'HdrMerge', 'Highlights', 'InputFormat', 'Jpeg', 'JpegException', 'LMMSE', 'Laplacian', 'LaplacianParams',
    'MotionEstimate', 'MotionHdrMerge', 'MotionTemporalDenoise', 'NLMeans', 'NoiseModel', 'NoiseProfile', 'NoiseStatistics', 'PackedFormat', 'PostProcess', 'RawCodec', 'RawCodecResult', 'RawPrepare', 'Resize', 'ScaledDemosaic', 'Sharpen', 'Subsampling', 'TemporalDenoise', 'ToneEqualizer', 'TonemapParameters', 'Warp', 'Wavelet', 'Wiener', 'aces_tonemap', 'apply_white_balance', 'bayer',
    'bilinear5x5_demosaic', 'chromatic', 'color_conversion', 'color_transform_3x3', 'colorlut', 'compute_image_bounds', 'compute_image_metrics',
    'compute_log_luminance', 'compute_luminance', 'debayer', 'decode12', 'decode12_float', 'decode12_half', 'decode12_u16', 'deconvolve', 'defringe', 'dehaze', 'denoise', 'device_jpeg',
    'encode', 'encode12_float', 'encode12_u16', 'estimate_channel_noise', 'estimate_white_balance', 'extension', 'filmic', 'framestats', 'hdralign', 'hdrmerge', 'highlights', 'jpeg', 'lab_to_rgb',
    'lab_to_xyz', 'linear_tonemap', 'lmmse', 'load_as_bayer', 'local_contrast', 'metrics_from_dict', 'metrics_to_dict', 'modify_hsl',
    'modify_log_luminance', 'modify_luminance', 'modify_vibrance', 'motion', 'nlmeans', 'noiseprofile', 'print_metrics', 'rawcodec', 'rawprepare', 'reinhard_tonemap', 'resample', 'rgb_to_bayer', 'rgb_to_lab',
    'rgb_to_xyz', 'scaled_demosaic', 'sharpen', 'temporal', 'toneequal', 'tonemap', 'warp', 'wavelet', 'white_balance', 'xyz_to_lab', 'xyz_to_rgb',
]
