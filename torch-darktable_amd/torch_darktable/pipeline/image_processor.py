"""packed raw bytes -> uint8 RGB: decode -> [temporal denoise of the raw mosaic | merge of an exposure bracket (process_bracket)] -> [chromatic aberration] -> [white balance | highlight reconstruction] -> demosaic -> [post-process] ->
[wavelet chroma denoise, with `noise_model` inside the variance-stabilising transform] -> [colour transform] -> [tone equalizer] ->
normalise -> [Wiener log-L] -> [bilateral] -> metrics -> tonemap -> [look] -> [sharpen] -> orientation
(reference torch_darktable/pipeline/image_processor.py).  With `exposure` (a FrameStats) the frames are normalised by percentile bounds
instead of the minimum and maximum over the set.  `process_resized` / `process_image_set_resized` put the
antialiased scaler to `final_size` between the tone mapper and the sharpener; `process` / `process_image_set` ignore
`resize_width`, as the reference does.  `process_preview` / `process_image_set_preview` put `preview` (a ScaledDemosaic) in the place
of the demosaic and run the rest of the chain on the reduced frames, in `preview_processor`.

Everything between the byte upload and the uint8 result stays on the device: bounds / metrics
and their moving averages are device tensors, no `.item()` anywhere, so one process can keep
its GPU busy and several processes (one per GPU) scale without host-side serialisation."""

from __future__ import annotations

import torch

from .. import debayer as _debayer
from .. import tonemap as _tonemap
from ..bayer import BayerPattern, PackedFormat
from ..chromatic import ChromaticAberration
from ..colorlut import ColorLUT
from ..denoise import Wiener
from ..framestats import FrameStats
from ..hdrmerge import HdrMerge
from ..highlights import Highlights
from ..lmmse import LMMSE
from ..local_contrast import Bilateral
from ..noiseprofile import NoiseModel
from ..rawcodec import RawCodec, RawCodecResult
from ..rawprepare import RawPrepare
from ..resample import Resize
from ..scaled_demosaic import ScaledDemosaic
from ..sharpen import Sharpen
from ..temporal import TemporalDenoise
from ..deconvolve import Deconvolve
from ..defringe import Defringe
from ..dehaze import Dehaze
from ..filmic import Filmic
from ..toneequal import ToneEqualizer
from ..wavelet import Wavelet
from ..white_balance import apply_white_balance
from .camera_settings import CameraSettings
from .config import Debayer, ImageProcessingSettings, ToneMapper
from .transform import ImageTransform, transform
from .util import lerp, normalize_image, resize_longest_edge


class ImageSizeMismatchError(Exception):
    """A raw buffer does not have the byte / pixel count the processor was built for."""

    def __init__(self, message: str, image_size: tuple[int, int], packed_format: PackedFormat, padding: int):
        super().__init__(message)
        self.image_size = image_size
        self.packed_format = packed_format
        self.padding = padding
        self.compressed_status: dict[str, torch.Tensor] = {}   # the raw codec's status per frame of the last process_*_compressed call


def _stage_property(attr: str, name: str, cls: type, article: str, doc: str, sized: bool = True, also=None) -> property:
    """The property `name` of an ImageProcessor that keeps an optional stage of type `cls` in `attr`.  The setter takes None or a
    `cls`, built for the processor's image size when `sized`, that passes also(processor, stage) when given."""
    def setter(self, stage) -> None:
        if stage is not None:
            if not isinstance(stage, cls):
                raise TypeError(f'{name} must be {article} {cls.__name__} or None, got {type(stage).__name__}')
            if sized and stage.image_size != tuple(self.image_size):
                raise ValueError(f'{name} is for {stage.width}x{stage.height}, the processor for {self.image_size[0]}x{self.image_size[1]}')
            if also is not None:
                also(self, stage)
        setattr(self, attr, stage)

    return property(lambda self: getattr(self, attr), setter, doc=doc)


def _check_mosaic_stage(name: str, stage, cls: type | None, article: str, hint: str, image_size, bayer_pattern: BayerPattern) -> None:
    """A stage on the raw mosaic in the constructor's slot `name`: None, or a `cls` (None: any type) built for the processor's image size
    and pattern.  hint: how to pass the slot, for a caller whose positional arguments have slipped."""
    if stage is None:
        return
    if cls is not None and not isinstance(stage, cls):
        raise TypeError(f'{name} must be {article} {cls.__name__} or None, got {type(stage).__name__} ({hint})')
    if stage.image_size != tuple(image_size) or stage.bayer_pattern != bayer_pattern:
        raise ValueError(f'{name} is for {stage.image_size} {stage.bayer_pattern.name}, the processor for {tuple(image_size)} {bayer_pattern.name}')


def _same_pattern(processor, stage: LMMSE) -> None:
    if stage.bayer_pattern != processor.bayer_pattern:
        raise ValueError(f'demosaic is for {stage.bayer_pattern.name}, the processor for {processor.bayer_pattern.name}')


class _SidePath:
    """A slot made by _stage_property for a stage that is no stage of the chain `process` runs: the same getter, setter and checks, as a
    data descriptor of its own type, so that what enumerates the chain's stages (the properties with a setter) does not list it."""

    def __init__(self, slot: property):
        self._slot, self.__doc__ = slot, slot.__doc__

    def __get__(self, obj, owner=None):
        return self if obj is None else self._slot.fget(obj)

    def __set__(self, obj, stage) -> None:
        self._slot.fset(obj, stage)


def _build_preview_processor(processor, stage: ScaledDemosaic) -> None:
    """The chain behind `preview`: a processor for the reduced frames, see ImageProcessor.preview."""
    if stage.bayer_pattern != processor.bayer_pattern:
        raise ValueError(f'preview is for {stage.bayer_pattern.name}, the processor for {processor.bayer_pattern.name}')
    reduced = ImageProcessor(stage.output_size, processor.bayer_pattern, processor.packed_format, processor.settings.model_copy(update={'resize_width': 0}),
                             processor.device, white_balance=None, transforms=processor.transforms, storage_dtype=processor.storage_dtype,
                             color=processor.color, look=processor.look)
    reduced.filmic = processor.filmic
    processor._preview_processor = reduced


class ImageProcessor:
    # haze removal on every demosaiced frame, behind `color` and in front of the tone equalizer: the property `dehaze` (every
    # constructor slot is pinned by the test of an earlier stage).  A class-level default, so that an object made without the
    # constructor has the slot too; None: the reference's chain
    _dehaze: Dehaze | None = None
    # the scene-referred display transform in place of `tonemap`: the property `filmic`, a class-level default for the same reason;
    # None: the reference's mappers
    _filmic: Filmic | None = None
    # capture sharpening on every demosaiced frame, behind `chroma_denoise` and in front of `color`: the property `capture_sharpen`,
    # a class-level default for the same reason; None: no such stage
    _capture_sharpen: Deconvolve | None = None
    # purple-fringe removal on every demosaiced frame, behind `chroma_denoise` and in front of `capture_sharpen`: the property
    # `defringe`, a class-level default for the same reason; None: no such stage
    _defringe: Defringe | None = None
    # the demosaic for noisy frames in place of the method `settings.debayer` names: the property `demosaic` (the Debayer enum is
    # pinned to the reference), a class-level default for the same reason; None: the reference's three methods
    _lmmse: LMMSE | None = None
    # the reduced-size demosaic of process_preview and the processor of the reduced frames behind it: the property `preview`, class-level
    # defaults for the same reason; None: the processor makes no previews
    _preview: ScaledDemosaic | None = None
    _preview_processor: 'ImageProcessor | None' = None

    def __init__(self, image_size: tuple[int, int], bayer_pattern: BayerPattern, packed_format: PackedFormat,
                 settings: ImageProcessingSettings, device: torch.device, white_balance: tuple[float, float, float] | None,
                 transforms: ImageTransform | dict[str, ImageTransform] = ImageTransform.none, chromatic: ChromaticAberration | None = None, padding: int = 0, hdr: HdrMerge | None = None,
                 storage_dtype: torch.dtype = torch.float32, temporal: TemporalDenoise | None = None, exposure: FrameStats | None = None, noise_model: NoiseModel | None = None, highlights: Highlights | None = None, color: ColorLUT | None = None, look: ColorLUT | None = None,
                 sharpen: Sharpen | None = None, chroma_denoise: Wavelet | None = None,
                 raw_correction: RawPrepare | None = None):
        assert device.index is not None, f'Device not fully specified: {device}'
        self.device = device
        self.settings = settings
        self.image_size = image_size
        self.bayer_pattern = bayer_pattern
        self.packed_format = packed_format
        self.transforms = transforms
        self.padding = padding
        # image storage between the stages: float32 (the reference) or float16 (fp32 arithmetic, half the HBM traffic)
        assert storage_dtype in (torch.float32, torch.float16)
        self.storage_dtype = storage_dtype
        # sensor correction in front of the demosaic (black / white level, defect pixels, lens shading): replaces decode + white
        # balance by one kernel that also applies the white balance; None: the reference's chain
        _check_mosaic_stage('raw_correction', raw_correction, None, '', '', image_size, bayer_pattern)
        self.raw_correction = raw_correction
        # recursive temporal denoiser on the linear mosaic without gains (where its noise model was measured), one sequence per
        # image name, in front of the white balance; load_image then takes the unfused path; None: the reference's chain
        _check_mosaic_stage('temporal', temporal, TemporalDenoise, 'a', 'pass the arguments behind storage_dtype by keyword', image_size, bayer_pattern)
        self.temporal = temporal
        # merge of an exposure bracket on the linear mosaics without gains, for process_bracket; None: the processor takes no brackets
        _check_mosaic_stage('hdr', hdr, HdrMerge, 'an', 'pass the arguments behind padding by keyword', image_size, bayer_pattern)
        self.hdr = hdr
        # lateral chromatic aberration: the red and the blue plane of the linear mosaic are resampled onto the green one, behind the
        # decode (or raw_correction, temporal, hdr) and in front of highlights or the white balance; load_image then takes the unfused
        # path; None: the reference's chain.  (Every slot behind padding is pinned by the test of an earlier stage.)
        _check_mosaic_stage('chromatic', chromatic, ChromaticAberration, 'a', 'pass it and padding by keyword', image_size, bayer_pattern)
        self.chromatic = chromatic
        # output sharpening of the tone-mapped uint8 frame, after the scaler and before the orientation; None: the reference's chain
        if sharpen is not None and not isinstance(sharpen, Sharpen):
            raise TypeError(f'sharpen must be a Sharpen or None, got {type(sharpen).__name__} (raw_correction is the argument after it: pass both by keyword)')
        self.sharpen = sharpen
        # wavelet shrinkage of every demosaiced frame (luma/chroma: the colour noise the log-lightness denoiser never sees), in
        # front of the bounds; None: the reference's chain
        if chroma_denoise is not None:
            if not isinstance(chroma_denoise, Wavelet):
                raise TypeError(f'chroma_denoise must be a Wavelet or None, got {type(chroma_denoise).__name__} (raw_correction is the argument after it: pass both by keyword)')
            if (chroma_denoise.width, chroma_denoise.height) != tuple(image_size):
                raise ValueError(f'chroma_denoise is for {chroma_denoise.width}x{chroma_denoise.height}, the processor for {image_size[0]}x{image_size[1]}')
            if chroma_denoise.channels == 1:
                raise ValueError('chroma_denoise has thresholds for one channel, the demosaiced frames have three channels')
        self.chroma_denoise = chroma_denoise
        # the measured noise model of the sensor: chroma_denoise then runs between stabilize and unstabilize, where the noise of every
        # channel has one level (build the stage with Wavelet.from_sigma(..., sigma=(s, s, s)), s the sigma_out = 1 of the transform);
        # None: the stage runs on the frame as it is
        if noise_model is not None:
            if not isinstance(noise_model, NoiseModel):
                raise TypeError(f'noise_model must be a NoiseModel or None, got {type(noise_model).__name__} (pass the arguments behind storage_dtype by keyword)')
            if chroma_denoise is None:
                raise ValueError('noise_model needs chroma_denoise: it is the stage the transform goes around')
        self.noise_model = noise_model
        # white balance that reconstructs clipped highlights, in the place of the white balance in front of the demosaic; None: the
        # reference's chain
        _check_mosaic_stage('highlights', highlights, Highlights, 'a', 'color is the argument after it: pass both by keyword', image_size, bayer_pattern)
        if highlights is not None and white_balance is None:
            raise ValueError('highlights needs white_balance: it applies the gains itself')
        self.highlights = highlights
        # colour management: `color` is the input transform (camera matrix, curves) on every demosaiced frame, behind the chroma
        # denoiser and in front of the bounds, storage type in and out; `look` grades the tone-mapped uint8 frame in front of the
        # scaler; None: the reference's chain
        for name, stage in (('color', color), ('look', look)):
            if stage is not None and not isinstance(stage, ColorLUT):
                raise TypeError(f'{name} must be a ColorLUT or None, got {type(stage).__name__} (pass the arguments behind highlights by keyword)')
        self.color, self.look = color, look
        # percentile bounds in the place of the minimum and maximum over the set: a FrameStats on the demosaiced frames, whose first
        # and last pooled quantile normalise them; None: the reference's chain
        if exposure is not None:
            if not isinstance(exposure, FrameStats):
                raise TypeError(f'exposure must be a FrameStats or None, got {type(exposure).__name__} (pass the arguments behind storage_dtype by keyword)')
            if exposure.image_size != tuple(image_size):
                raise ValueError(f'exposure is for {exposure.width}x{exposure.height}, the processor for {image_size[0]}x{image_size[1]}')
            if exposure.bayer_pattern is not None or exposure.channels != 3:
                raise ValueError('exposure measures the demosaiced frames: it needs channels=3 and no bayer_pattern')
            if not exposure.quantiles:
                raise ValueError('exposure needs at least one quantile: the bounds are its first and last')
        self.exposure = exposure
        # dodge and burn by exposure band on every demosaiced frame, behind `color` and in front of the bounds: the property
        # `tone_equalizer` (every constructor slot is pinned by the test of an earlier stage); None: the reference's chain
        self._tone_equalizer: ToneEqualizer | None = None
        self._lum_plane: torch.Tensor | None = None  # lightness plane handed from the denoiser to the bilateral stage
        self._ab_plane: torch.Tensor | None = None   # ... and the chroma (a, b) plane of the Lab hand-over
        self.metrics: torch.Tensor | None = None  # moving averages, device-resident
        self.bounds: torch.Tensor | None = None
        self.rcd_workspace = _debayer.RCD(device, image_size, bayer_pattern)
        self.wiener_workspace = Wiener(device, image_size)
        self._build_tunable_workspaces(settings)
        self._build_resize_workspace()
        self.white_balance = torch.tensor(white_balance, device=device, dtype=torch.float32) if white_balance is not None else None

    def _build_tunable_workspaces(self, s: ImageProcessingSettings, which=('bilateral', 'ppg', 'postprocess')) -> None:
        if 'bilateral' in which:
            self.bil_workspace = Bilateral(self.device, self.image_size, sigma_s=s.bil_sigma_spatial, sigma_r=s.bil_sigma_luminance)
        if 'ppg' in which:
            self.ppg_workspace = _debayer.PPG(self.device, self.image_size, self.bayer_pattern, median_threshold=s.ppg_median_threshold)
        if 'postprocess' in which:
            self.postprocess_workspace = _debayer.PostProcess(
                self.device, self.image_size, self.bayer_pattern, color_smoothing_passes=s.color_smoothing_passes,
                green_eq_local=False, green_eq_global=True, green_eq_threshold=s.green_eq_threshold)

    def _build_resize_workspace(self) -> None:
        """The scaler of process_resized (None: resize_width == 0).  A resize_width the scaler cannot serve (beyond 16:1) is
        reported by process_resized, not here: every other call ignores resize_width."""
        self.resize_workspace: Resize | None = None
        self._resize_error: ValueError | None = None
        if self.settings.resize_width != 0:
            try:
                self.resize_workspace = Resize(self.device, self.image_size, self.final_size)
            except ValueError as e:
                self._resize_error = e

    def __repr__(self) -> str:
        wb = 'None' if self.white_balance is None else '({:.3f}, {:.3f}, {:.3f})'.format(*self.white_balance.tolist())
        tf = self.transforms.name if isinstance(self.transforms, ImageTransform) else '{' + ', '.join(f'{k}: {v.name}' for k, v in self.transforms.items()) + '}'
        return (f'ImageProcessor(size={self.image_size}, bayer={self.bayer_pattern.name}, format={self.packed_format.name}, device={self.device}, '
                f'wb={wb}, padding={self.padding}, transform={tf}, debayer={self.settings.debayer.name}, tonemap={self.settings.tone_mapping.name})')

    @staticmethod
    def from_camera_settings(camera_settings: CameraSettings, device: torch.device, storage_dtype: torch.dtype = torch.float32) -> 'ImageProcessor':
        return ImageProcessor(camera_settings.image_size, camera_settings.bayer_pattern, camera_settings.packed_format,
                              camera_settings.image_processing, device=device, white_balance=camera_settings.white_balance,
                              transforms=camera_settings.transform, padding=camera_settings.padding, storage_dtype=storage_dtype)

    def update_settings(self, settings: ImageProcessingSettings) -> None:
        """Swap settings; only workspaces whose parameters changed are rebuilt."""
        old, self.settings = self.settings, settings

        def changed(*names: str) -> bool:
            return any(getattr(old, n) != getattr(settings, n) for n in names)

        stale = []
        if changed('bil_sigma_spatial', 'enable_bilateral', 'bil_sigma_luminance'):
            stale.append('bilateral')
        if changed('ppg_median_threshold'):
            stale.append('ppg')
        if changed('color_smoothing_passes', 'green_eq_threshold'):
            stale.append('postprocess')
        self._build_tunable_workspaces(settings, tuple(stale))
        if changed('resize_width'):
            self._build_resize_workspace()
        if self.preview_processor is not None:
            self.preview_processor.update_settings(settings.model_copy(update={'resize_width': 0}))

    @property
    def final_size(self) -> tuple[int, int]:
        return resize_longest_edge(self.image_size, self.settings.resize_width)

    dehaze = _stage_property('_dehaze', 'dehaze', Dehaze, 'a', """The haze removal run on every demosaiced frame behind `color` and in front of `tone_equalizer`, so that bounds and metrics see
        its result; None: no such stage.""")
    demosaic = _stage_property('_lmmse', 'demosaic', LMMSE, 'an', """The demosaic that takes the place of the method `settings.debayer` names, still followed by PostProcess when
        `settings.postprocess` is set; load_image then takes the unfused path (decode, white balance, demosaic), and with binary16
        storage the stage writes binary16 itself.  None: bilinear, PPG or RCD, as `settings.debayer` says.""", also=_same_pattern)
    defringe = _stage_property('_defringe', 'defringe', Defringe, 'a', """The purple-fringe removal run on every demosaiced frame behind `chroma_denoise` and in front of `capture_sharpen`: noise
        does not set its threshold, and the deconvolution does not sharpen the halo; None: no such stage.""")
    capture_sharpen = _stage_property('_capture_sharpen', 'capture_sharpen', Deconvolve, 'a', """The deconvolution run on every demosaiced frame behind `chroma_denoise` and in front of `color`: on linear camera RGB, after
        the noise has been dealt with, so that every later stage sees its detail; None: no such stage.""")
    filmic = _stage_property('_filmic', 'filmic', Filmic, 'a', """The scene-referred tone mapping that takes the place of `tonemap` on every frame (uint8 out); bounds, metrics and their moving
        averages are computed as without it.  None: the mapper of the settings.""", sized=False)
    tone_equalizer = _stage_property('_tone_equalizer', 'tone_equalizer', ToneEqualizer, 'a',
                                     """The tone equalizer run on every demosaiced frame behind `color`, so that bounds and metrics see its result; None: no such stage.""")
    preview = _SidePath(_stage_property('_preview', 'preview', ScaledDemosaic, 'a', """The reduced-size demosaic of `process_preview` / `process_image_set_preview`, built for the processor's image size and
        pattern.  Setting it builds `preview_processor`: an ImageProcessor for `preview.output_size` with the same pattern, packed
        format, device, storage type and transforms, the same settings except resize_width = 0, no white balance (the gains are in the
        reduced frame already) and the unsized stages `color`, `look` and `filmic` as they are at that moment.  The stages bound to a
        frame size (chroma_denoise, defringe, capture_sharpen, dehaze, tone_equalizer, sharpen, exposure) are the caller's to set on
        `preview_processor`, built for the reduced size.  `update_settings` reaches it.  No other method looks at `preview`.
        None: the processor makes no previews.""", also=_build_preview_processor))

    @property
    def preview_processor(self) -> 'ImageProcessor | None':
        """The processor of the reduced frames behind `preview` (its bounds and metrics are the previews' own); None without `preview`."""
        return self._preview_processor if self._preview is not None else None

    @property
    def expected_bytes(self) -> int:
        w, h = self.image_size
        if self.packed_format not in (PackedFormat.Packed12, PackedFormat.Packed12_IDS):
            raise ValueError(f'Unsupported packed format: {self.packed_format}')
        return (w * h * 3) // 2 + self.padding

    def _mismatch(self, message: str) -> ImageSizeMismatchError:
        return ImageSizeMismatchError(message, image_size=self.image_size, packed_format=self.packed_format, padding=self.padding)

    # ---- stages
    def load_bytes(self, bytes: torch.Tensor) -> torch.Tensor:
        """Packed raw bytes (+ trailing padding) -> (H, W) float32 mosaic."""
        if bytes.numel() != self.expected_bytes:
            raise self._mismatch(f'Image size mismatch: expected {self.expected_bytes} bytes for {self.image_size} {self.packed_format.name} '
                                 f'with {self.padding} padding, got {bytes.numel()} bytes. ')
        if self.padding > 0:
            bytes = bytes[: -self.padding]
        decoded = _debayer.decode12(bytes, output_dtype=torch.float32, format_type=self.packed_format)
        w, h = self.image_size
        if decoded.numel() != w * h:
            raise self._mismatch(f'Decoded image size mismatch: expected {w * h} pixels ({w}x{h}), got {decoded.numel()} pixels.')
        return decoded.view(h, w)

    def load_image(self, bytes: torch.Tensor, image_name: str | None = None) -> torch.Tensor:
        if self.temporal is not None:
            # the filter sees the linear mosaic as the noise model does: sensor correction without gains (or the plain decode) ->
            # temporal (the sequence of this image name) -> highlights or white balance -> demosaic
            if self.raw_correction is not None:
                if bytes.numel() != self.expected_bytes:
                    raise self._mismatch(f'Image size mismatch: expected {self.expected_bytes} bytes for {self.image_size} {self.packed_format.name} '
                                         f'with {self.padding} padding, got {bytes.numel()} bytes. ')
                payload = bytes[: bytes.numel() - self.padding] if self.padding > 0 else bytes
                mosaic = self.raw_correction.process_packed(payload, self.packed_format, white_balance=None)
            else:
                mosaic = self.load_bytes(bytes)
            mosaic = self.temporal.process(mosaic, key=image_name)
            if self.chromatic is not None:
                mosaic = self.chromatic.correct(mosaic)
            if self.highlights is not None:
                mosaic = self.highlights.process(mosaic, self.white_balance)
            elif self.white_balance is not None:
                mosaic = apply_white_balance(mosaic, self.white_balance, self.bayer_pattern)
            return self._demosaic(mosaic).to(self.storage_dtype)
        if self.highlights is not None or self.chromatic is not None:
            # the gains are applied by the highlight stage, on the linear mosaic: sensor correction without gains (or the plain
            # decode) -> [chromatic aberration] -> highlights or white balance -> demosaic; the fused decode + white balance + RCD
            # kernel has no place for either
            if self.raw_correction is not None:
                if bytes.numel() != self.expected_bytes:
                    raise self._mismatch(f'Image size mismatch: expected {self.expected_bytes} bytes for {self.image_size} {self.packed_format.name} '
                                         f'with {self.padding} padding, got {bytes.numel()} bytes. ')
                payload = bytes[: bytes.numel() - self.padding] if self.padding > 0 else bytes
                mosaic = self.raw_correction.process_packed(payload, self.packed_format, white_balance=None)
            else:
                mosaic = self.load_bytes(bytes)
            if self.chromatic is not None:
                mosaic = self.chromatic.correct(mosaic)
            if self.highlights is not None:
                mosaic = self.highlights.process(mosaic, self.white_balance)
            elif self.white_balance is not None:
                mosaic = apply_white_balance(mosaic, self.white_balance, self.bayer_pattern)
            return self._demosaic(mosaic).to(self.storage_dtype)
        if self.raw_correction is not None:
            if bytes.numel() != self.expected_bytes:
                raise self._mismatch(f'Image size mismatch: expected {self.expected_bytes} bytes for {self.image_size} {self.packed_format.name} '
                                     f'with {self.padding} padding, got {bytes.numel()} bytes. ')
            payload = bytes[: bytes.numel() - self.padding] if self.padding > 0 else bytes
            mosaic = self.raw_correction.process_packed(payload, self.packed_format, white_balance=self.white_balance)
            return self._demosaic(mosaic).to(self.storage_dtype)   # the white balance is in the mosaic already
        if self.settings.debayer == Debayer.rcd and self._lmmse is None:
            # decode -> white balance -> RCD as one kernel (same result as load_bytes + debayer, two fp32 planes less)
            if bytes.numel() != self.expected_bytes:
                raise self._mismatch(f'Image size mismatch: expected {self.expected_bytes} bytes for {self.image_size} {self.packed_format.name} '
                                     f'with {self.padding} padding, got {bytes.numel()} bytes. ')
            payload = bytes[: bytes.numel() - self.padding] if self.padding > 0 else bytes
            rgb = self.rcd_workspace.process_packed(payload, self.white_balance, self.packed_format, self.storage_dtype)
            # (PostProcess takes the storage type as it is: fp32 between its stages, one rounding at its store -- the same bits as
            # converting to float32 around it, without the two conversion passes)
            return self.postprocess_workspace.process(rgb) if self.settings.postprocess else rgb
        return self.debayer(self.load_bytes(bytes)).to(self.storage_dtype)

    def load_bracket(self, payloads, exposures, ref: int | None = None) -> torch.Tensor:
        """The packed frames of one exposure bracket -> the demosaiced merge: every payload becomes the linear mosaic without gains
        (sensor correction, or the plain decode), `hdr` merges them, and the merged mosaic goes on as load_image's does: highlights or
        white balance -> demosaic."""
        if self.hdr is None:
            raise ValueError('process_bracket needs hdr: build the processor with hdr=HdrMerge(...)')
        if self.temporal is not None:
            raise ValueError('process_bracket and temporal do not combine: the frames of a bracket are no sequence of one exposure')
        mosaics = []
        for bytes in payloads:
            if self.raw_correction is not None:
                if bytes.numel() != self.expected_bytes:
                    raise self._mismatch(f'Image size mismatch: expected {self.expected_bytes} bytes for {self.image_size} {self.packed_format.name} '
                                         f'with {self.padding} padding, got {bytes.numel()} bytes. ')
                payload = bytes[: bytes.numel() - self.padding] if self.padding > 0 else bytes
                mosaics.append(self.raw_correction.process_packed(payload, self.packed_format, white_balance=None))
            else:
                mosaics.append(self.load_bytes(bytes))
        mosaic = self.hdr.process(mosaics, exposures, ref=ref)
        if self.chromatic is not None:
            mosaic = self.chromatic.correct(mosaic)
        if self.highlights is not None:
            mosaic = self.highlights.process(mosaic, self.white_balance)
        elif self.white_balance is not None:
            mosaic = apply_white_balance(mosaic, self.white_balance, self.bayer_pattern)
        return self._demosaic(mosaic).to(self.storage_dtype)

    def debayer(self, bayer_image: torch.Tensor) -> torch.Tensor:
        assert bayer_image.ndim == 2, f'Bayer image must have 2 dimensions, got {bayer_image.shape}'
        if self.white_balance is not None:
            bayer_image = apply_white_balance(bayer_image, self.white_balance, self.bayer_pattern)
        return self._demosaic(bayer_image)

    def _demosaic(self, bayer_image: torch.Tensor) -> torch.Tensor:
        mosaic = bayer_image.unsqueeze(-1)
        method = self.settings.debayer
        if self._lmmse is not None:
            rgb = self._lmmse.process(mosaic, out_dtype=self.storage_dtype)
        elif method == Debayer.bilinear:
            rgb = _debayer.bilinear5x5_demosaic(mosaic, self.bayer_pattern)
        elif method == Debayer.rcd:
            rgb = self.rcd_workspace.process(mosaic)
        elif method == Debayer.ppg:
            rgb = self.ppg_workspace.process(mosaic)
        else:
            raise AssertionError(f'Invalid debayer method: {method}')
        return self.postprocess_workspace.process(rgb) if self.settings.postprocess else rgb

    def process_rgb(self, rgb_raw: torch.Tensor, bounds: torch.Tensor | None = None, metrics: '_tonemap.MetricsAccumulator | None' = None) -> torch.Tensor:
        """normalise -> [denoise] -> [local contrast].  When both stages run, the denoiser hands the lightness plane of
        its result to the bilateral (which would extract it first); with `metrics` the result is also added to that
        accumulator -- same results as the separate calls."""
        s = self.settings
        both = s.enable_denoise and s.enable_bilateral
        if bounds is not None and not both:
            rgb_raw = normalize_image(rgb_raw, bounds)
        if both:
            # both stages replace the Lab lightness of the same pixel (reference denoise.py:54-58, local_contrast.py:109-114): the
            # pixel travels between them as lightness + chroma planes and is converted back to RGB once (include/tdk_hip.h, Lab
            # hand-over; tests/test_gpu_lab_chain.py) instead of as an RGB image through two colour round trips
            hw = (self.image_size[1], self.image_size[0])
            if self._lum_plane is None or self._lum_plane.device != rgb_raw.device:
                self._lum_plane = torch.empty(hw, dtype=torch.float32, device=rgb_raw.device)
                self._ab_plane = torch.empty((*hw, 2), dtype=torch.float32, device=rgb_raw.device)
            # (normalize_image rides in the first kernel of the chain: the normalised image is never stored)
            self.wiener_workspace.process_log_luminance_lab(rgb_raw, s.denoise, luminance_out=self._lum_plane, chroma_out=self._ab_plane, bounds=bounds)
            return self.bil_workspace.process_lab(self._lum_plane, self._ab_plane, s.bilateral, out_dtype=rgb_raw.dtype, metrics=metrics)
        if s.enable_denoise:
            rgb_raw = self.wiener_workspace.process_log_luminance(rgb_raw, s.denoise)
        if s.enable_bilateral:
            rgb_raw = self.bil_workspace.process_rgb(rgb_raw, s.bilateral, metrics=metrics)
        elif metrics is not None:
            metrics.add(rgb_raw)
        return rgb_raw

    def tonemap(self, rgb_raw: torch.Tensor, metrics: torch.Tensor | None = None) -> torch.Tensor:
        s = self.settings
        params = _tonemap.TonemapParameters(s.tone_gamma, s.tone_intensity, s.light_adapt, s.vibrance)
        if metrics is None:
            metrics = _tonemap.compute_image_metrics([rgb_raw], stride=4, min_gray=1e-4)
        mapper = s.tone_mapping
        if mapper == ToneMapper.reinhard:
            return _tonemap.reinhard_tonemap(rgb_raw, metrics, params)
        if mapper == ToneMapper.linear:
            return _tonemap.linear_tonemap(rgb_raw, metrics, params)
        if mapper == ToneMapper.aces:
            return _tonemap.aces_tonemap(rgb_raw, params)
        return _tonemap.aces_tonemap(rgb_raw, params, metrics)

    def transform(self, image: torch.Tensor, image_name: str) -> torch.Tensor:
        t = self.transforms[image_name] if isinstance(self.transforms, dict) else self.transforms
        return transform(image, t)

    # ---- whole pipeline
    def process(self, bytes: torch.Tensor, image_name: str) -> torch.Tensor:
        return self.process_image_set({image_name: bytes})[image_name]

    def process_bracket(self, payloads, exposures, image_name: str, ref: int | None = None) -> torch.Tensor:
        """`process` of one exposure bracket: the packed frames are merged on the raw mosaic by `hdr` (exposures, ref: HdrMerge.process)
        and the merge continues as `process` does from the mosaic on, bounds and metrics included."""
        rgb = self.load_bracket(payloads, exposures, ref)
        return self._process_frames([image_name], [rgb], resized=False)[image_name]

    def process_image_set(self, image_set_bytes: dict[str, torch.Tensor]) -> dict[str, torch.Tensor]:
        """One synchronised set of cameras: shared bounds / metrics (moving-averaged across calls)."""
        return self._process_image_set(image_set_bytes, resized=False)

    def _decompress(self, stream, codec: RawCodec) -> tuple[torch.Tensor, torch.Tensor]:
        """A TDKR stream (a RawCodecResult or a 1-D uint8 device tensor) -> (the buffer `process` takes: expected_bytes long, the frame in
        the processor's packed_format, the padding bytes zero; the decoder's status, a 0-dim int32 device tensor)."""
        if not isinstance(codec, RawCodec):
            raise TypeError(f'codec must be a RawCodec, got {type(codec).__name__}')
        if tuple(codec.image_size) != tuple(self.image_size):
            raise self._mismatch(f'Image size mismatch: the codec is for {codec.image_size}, the processor for {tuple(self.image_size)}. ')
        data = stream.data if isinstance(stream, RawCodecResult) else stream
        buffer = torch.empty(self.expected_bytes, dtype=torch.uint8, device=data.device)
        if self.padding > 0:
            buffer[buffer.numel() - self.padding:].zero_()
        return codec.decode(stream, output=self.packed_format, out=buffer, return_status=True)

    def process_compressed(self, stream, image_name: str, codec: RawCodec) -> torch.Tensor:
        """`process` of a frame that arrives as a lossless TDKR stream (RawCodec.encode): decoded on the device into the packed bytes
        `process` takes, so every configuration behaves bit for bit as on the packed file.  Nothing waits for the decoder: a corrupt or
        truncated stream is processed as the frame the decoder leaves of it (zeros in the segments it refuses).  The decoder's status
        of the call is kept in `compressed_status[image_name]`, a 0-dim int32 device tensor (0, or RawCodec.BAD_* bits), for a caller
        who wants to look."""
        return self.process_image_set_compressed({image_name: stream}, codec)[image_name]

    def process_image_set_compressed(self, image_set_streams: dict, codec: RawCodec) -> dict[str, torch.Tensor]:
        """`process_image_set` of TDKR streams, one codec (one frame size) for the set; `compressed_status` holds the decoder's status
        of every frame of the call, by name (see process_compressed)."""
        decoded = {name: self._decompress(stream, codec) for name, stream in image_set_streams.items()}
        self.compressed_status = {name: status for name, (_, status) in decoded.items()}
        return self.process_image_set({name: buffer for name, (buffer, _) in decoded.items()})

    def process_resized(self, bytes: torch.Tensor, image_name: str) -> torch.Tensor:
        """`process`, scaled to `final_size` (longest edge = settings.resize_width) before the orientation: the result has
        transformed_size(final_size, transform).  resize_width == 0: what `process` returns."""
        return self.process_image_set_resized({image_name: bytes})[image_name]

    def process_image_set_resized(self, image_set_bytes: dict[str, torch.Tensor]) -> dict[str, torch.Tensor]:
        """`process_image_set` with every tone-mapped uint8 frame scaled to `final_size` (antialiased, `Resize`) before its
        orientation; bounds and metrics are those of the full-size frames, updated exactly as `process_image_set` does."""
        return self._process_image_set(image_set_bytes, resized=True)

    def process_preview(self, bytes: torch.Tensor, image_name: str) -> torch.Tensor:
        """`process` at `preview.output_size`: the frame is brought to the mosaic in front of the demosaic exactly as `process` does on
        each of its branches (raw_correction, temporal with the image name as key, chromatic, highlights or the white balance), `preview`
        turns it into the reduced frame, and `preview_processor` continues from there as `process` does from the demosaiced frame on,
        with its own stages, bounds and metrics: this processor's `bounds` and `metrics` are not touched.  With none of those mosaic
        stages set the head is one launch from the packed bytes.  PostProcess is not run: it repairs artefacts of a demosaic, and an
        area average makes none.  The result has the orientation's size of `preview.output_size`."""
        return self.process_image_set_preview({image_name: bytes})[image_name]

    def process_image_set_preview(self, image_set_bytes: dict[str, torch.Tensor]) -> dict[str, torch.Tensor]:
        """`process_image_set` at `preview.output_size`, see process_preview; the set shares the bounds and metrics of `preview_processor`."""
        if self._preview is None:
            raise ValueError('process_preview needs preview: set processor.preview = ScaledDemosaic(...)')
        names = list(image_set_bytes.keys())
        frames = [self._load_preview(b, name) for name, b in image_set_bytes.items()]
        return self.preview_processor._process_frames(names, frames, resized=False)

    def _load_preview(self, bytes: torch.Tensor, image_name: str) -> torch.Tensor:
        """Packed raw bytes -> the reduced frame: load_image's mosaic on each of its branches, then `preview` in the place of the demosaic."""
        if bytes.numel() != self.expected_bytes:
            raise self._mismatch(f'Image size mismatch: expected {self.expected_bytes} bytes for {self.image_size} {self.packed_format.name} '
                                 f'with {self.padding} padding, got {bytes.numel()} bytes. ')
        payload = bytes[: bytes.numel() - self.padding] if self.padding > 0 else bytes
        preview, gains = self._preview, self.white_balance
        if self.temporal is not None or self.highlights is not None or self.chromatic is not None:
            # the stages see the linear mosaic without gains; the gains then ride in the preview's launch, with apply_white_balance's bits
            mosaic = self.raw_correction.process_packed(payload, self.packed_format, white_balance=None) if self.raw_correction is not None else self.load_bytes(bytes)
            if self.temporal is not None:
                mosaic = self.temporal.process(mosaic, key=image_name)
            if self.chromatic is not None:
                mosaic = self.chromatic.correct(mosaic)
            if self.highlights is not None:
                mosaic, gains = self.highlights.process(mosaic, self.white_balance), None
            return preview.process(mosaic, gains, out_dtype=self.storage_dtype)
        if self.raw_correction is not None:   # the white balance is in the mosaic already
            return preview.process(self.raw_correction.process_packed(payload, self.packed_format, white_balance=gains), out_dtype=self.storage_dtype)
        if self.image_size[0] % 2:   # (pixel pairs run across the rows: the fused launch has no place for them)
            return preview.process(self.load_bytes(bytes), gains, out_dtype=self.storage_dtype)
        return preview.process_packed(payload, self.packed_format, gains, self.storage_dtype)

    def _process_image_set(self, image_set_bytes: dict[str, torch.Tensor], resized: bool) -> dict[str, torch.Tensor]:
        if resized and self._resize_error is not None:
            raise self._resize_error
        names = list(image_set_bytes.keys())
        if self.temporal is not None:   # the image name is the key of the frame's history; without the stage the call is what it was
            rgb = [self.load_image(b, name) for name, b in image_set_bytes.items()]
        else:
            rgb = [self.load_image(b) for b in image_set_bytes.values()]
        return self._process_frames(names, rgb, resized)

    def _process_frames(self, names: list[str], rgb: list[torch.Tensor], resized: bool) -> dict[str, torch.Tensor]:
        """From the demosaiced frames of a set on."""
        ema = self.settings.moving_average
        if self.chroma_denoise is not None and self.noise_model is not None:
            m, wb = self.noise_model, self.white_balance
            rgb = [m.unstabilize(self.chroma_denoise.process(m.stabilize(img, gains=wb)), gains=wb, out_dtype=img.dtype) for img in rgb]
        elif self.chroma_denoise is not None:
            rgb = [self.chroma_denoise.process(img) for img in rgb]
        if self._defringe is not None:
            rgb = [self._defringe.process(img) for img in rgb]
        if self._capture_sharpen is not None:
            rgb = [self._capture_sharpen.process(img) for img in rgb]
        if self.color is not None:
            rgb = [self.color.process(img) for img in rgb]
        if self._dehaze is not None:
            rgb = [self._dehaze.process(img) for img in rgb]
        if self._tone_equalizer is not None:
            rgb = [self._tone_equalizer.process(img) for img in rgb]
        if self.exposure is not None and len(rgb) > self.exposure.max_frames:
            raise ValueError(f'exposure takes {self.exposure.max_frames} frames per call (max_frames), the image set has {len(rgb)}')
        bounds = self.exposure.bounds(rgb) if self.exposure is not None else _tonemap.compute_image_bounds(rgb, stride=8)
        self.bounds = lerp(self.bounds if self.bounds is not None else bounds, bounds, ema)
        acc = _tonemap.MetricsAccumulator(self.device, stride=8)  # == compute_image_metrics(rgb, stride=8), fed by the last stage
        rgb = [self.process_rgb(img, self.bounds, acc) for img in rgb]
        metrics = acc.finish()
        self.metrics = lerp(self.metrics if self.metrics is not None else metrics, metrics, ema)
        if self._filmic is not None:
            mapped = [self._filmic.process(img) for img in rgb]
        else:
            mapped = [self.tonemap(img, self.metrics) for img in rgb]
        if self.look is not None:
            mapped = [self.look.process(img) for img in mapped]
        if resized and self.resize_workspace is not None:
            mapped = [self.resize_workspace.process(img) for img in mapped]
        if self.sharpen is not None:
            mapped = [self.sharpen.process(img) for img in mapped]
        return {name: self.transform(img, name) for name, img in zip(names, mapped)}
