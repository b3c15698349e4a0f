"""`filter2d` -- host-side mirror of drtk/filter2d.py: alias-free up/down-sampling and low-pass filtering of NCHW images with
separable FIR filters, one fused HIP kernel (csrc/filter2d.hip) behind all of it."""
from enum import Enum
from typing import Optional

import torch as th
from drtk_amd.utils import load_torch_ops

# the operator library is one file; it is loaded through a name the loader serves (`filter2d_ext` is not one of them: the
# `drtk` drop-in package does not lift filter2d yet -- INTEGRATION.md)
load_torch_ops("drtk.rasterize_ext")

__all__ = [
    "FilterType",
    "FilterOptions",
    "resample_filter",
    "filter",
    "low_pass_filter",
    "downsample",
    "upsample",
    "make_resampling_kernel",
]


def _use_reflection_padding(padding_mode: str) -> bool:
    if padding_mode == "reflection":
        return True
    if padding_mode == "zeros":
        return False
    raise NotImplementedError(f"filter2d: expected padding_mode to be 'zeros' or 'reflection', but got: {padding_mode!r}")


class FilterType(Enum):
    """Filter families supported by :func:`make_resampling_kernel`."""

    Kaiser = 0
    Lanczos = 1


def _validate_filter_type(filter_type: object) -> FilterType:
    if not isinstance(filter_type, FilterType):
        raise TypeError(f"filter2d: filter_type must be a FilterType value, but got {filter_type!r}")
    return filter_type


class FilterOptions:
    """Options used to construct filter2d resampling kernels."""

    __slots__ = ("n_taps", "filter_type", "alias_guard_band")

    def __init__(
        self,
        n_taps: int = 6,
        filter_type: FilterType = FilterType.Kaiser,
        alias_guard_band: Optional[float] = None,
        alias_suppression_level: Optional[float] = None,
    ) -> None:
        """
        Args:
            n_taps: Number of taps, default 6.  Not the length of the filter tensor, which is ``m * n_taps``: when
                upsampling, each output pixel is affected by ``n_taps`` input pixels; when downsampling, each input pixel
                affects ``n_taps`` output pixels.
            filter_type: Filter family, default :attr:`FilterType.Kaiser`.
            alias_guard_band: Where the cutoff of the alias-free-GAN low-pass design is placed; non-negative, recommended
                range ``[0, 1]``, default ``0.0``.  Frequencies are normalised to the input sampling rate.  For a given
                ``freq_div`` the usable band limit is ``bandlimit = 0.5 / freq_div``, the transition half-width is
                ``(sqrt(2) - 1) * bandlimit``, and the cutoff sits at ``bandlimit - alias_guard_band * half_width``:
                ``0.0`` puts it at the band limit (least blur, the transition band reaches past the band limit), ``1.0``
                one half-width below it (the transition band ends at the band limit), values above ``1.0`` leave extra
                guard band and blur more.  It does not set the stop-band attenuation, which also depends on ``n_taps``
                and ``filter_type``.
            alias_suppression_level: Backward-compatible alias of ``alias_guard_band``.
        """
        if alias_guard_band is None:
            value = 0.0 if alias_suppression_level is None else alias_suppression_level
        else:
            if alias_suppression_level is not None and alias_guard_band != alias_suppression_level:
                raise ValueError("FilterOptions: specify only one of alias_guard_band and alias_suppression_level")
            value = alias_guard_band
        self.n_taps = n_taps
        self.filter_type = _validate_filter_type(filter_type)
        self.alias_guard_band = value

    @property
    def alias_suppression_level(self) -> float:
        return self.alias_guard_band

    @alias_suppression_level.setter
    def alias_suppression_level(self, value: float) -> None:
        self.alias_guard_band = value


@th.compiler.disable
def resample_filter(
    x: th.Tensor,
    f: th.Tensor,
    up: int = 1,
    down: int = 1,
    padding_mode: str = "reflection",
) -> th.Tensor:
    """Resample an NCHW tensor with a separable 1D filter.

    The input is upsampled by interleaving zeros, convolved with ``f`` along both spatial dimensions, and downsampled by
    dropping sample points -- in one fused kernel that reads each input and writes each output once.  HIP tensors only:
    float16 (storage only, sums in float32), float32 or float64; any ``up``, ``down`` and filter length for which the
    padding rule of the reference is defined, any ``N * C``.

    Args:
        x: Input tensor with shape ``(N, C, H, W)``.
        f: 1D filter tensor, float32.
        up: Upsampling factor. Default is ``1``, which leaves the input sampling rate unchanged.
        down: Downsampling factor. Default is ``1``, which leaves the output sampling rate unchanged.
        padding_mode: Border handling, ``"zeros"`` or ``"reflection"``. Default is ``"reflection"``.

    Gradients: ``x`` only.  The backward is the same operator with ``up`` and ``down`` exchanged applied to the incoming
    gradient, as in the reference.  With ``"zeros"`` that is the exact adjoint.  With ``"reflection"`` it is
    NOT the derivative of the forward within a filter's reach of the border: the reference reflects the incoming gradient
    instead of folding the border contributions back, and this package reproduces it.  With ``down > 1`` the backward needs ``H``
    and ``W`` to be multiples of ``down`` (the gradient has another shape otherwise) and raises an error if they are not.
    """
    return th.ops.filter2d_ext.resample_filter(x.contiguous(), f.contiguous(), up, down, _use_reflection_padding(padding_mode))


@th.compiler.disable
def filter(
    x: th.Tensor,
    f: th.Tensor,
    padding_mode: str = "reflection",
) -> th.Tensor:
    """Filter an NCHW tensor without changing its spatial size.

    Args:
        x: Input tensor with shape ``(N, C, H, W)``.
        f: 1D filter tensor, float32.
        padding_mode: Border handling, ``"zeros"`` or ``"reflection"``. Default is ``"reflection"``.
    """
    return th.ops.filter2d_ext.resample_filter(x.contiguous(), f.contiguous(), 1, 1, _use_reflection_padding(padding_mode))


@th.compiler.disable
def upsample(
    x: th.Tensor,
    filter_options: FilterOptions,
    upsample_factor: int = 2,
    padding_mode: str = "reflection",
) -> th.Tensor:
    """Upsample an NCHW tensor by ``upsample_factor``.

    The fused equivalent of :func:`make_resampling_kernel` (with gain ``upsample_factor``) followed by
    :func:`resample_filter`.

    Args:
        x: Input tensor with shape ``(N, C, H, W)``.
        filter_options: Interpolation filter options.
        upsample_factor: Upsampling factor. Must be at least ``1``. Default is ``2``.
        padding_mode: Border handling, ``"zeros"`` or ``"reflection"``. Default is ``"reflection"``.
    """
    return th.ops.filter2d_ext.upsample(
        x.contiguous(), filter_options.n_taps, upsample_factor, filter_options.alias_guard_band, filter_options.filter_type.value,
        _use_reflection_padding(padding_mode))


@th.compiler.disable
def downsample(
    x: th.Tensor,
    filter_options: FilterOptions,
    downsample_factor: int = 2,
    padding_mode: str = "reflection",
) -> th.Tensor:
    """Downsample an NCHW tensor by ``downsample_factor``.

    The fused equivalent of :func:`make_resampling_kernel` followed by :func:`resample_filter`.

    Args:
        x: Input tensor with shape ``(N, C, H, W)``.
        filter_options: Interpolation filter options.
        downsample_factor: Downsampling factor. Must be at least ``1``. Default is ``2``.
        padding_mode: Border handling, ``"zeros"`` or ``"reflection"``. Default is ``"reflection"``.
    """
    return th.ops.filter2d_ext.downsample(
        x.contiguous(), filter_options.n_taps, downsample_factor, filter_options.alias_guard_band,
        filter_options.filter_type.value, _use_reflection_padding(padding_mode))


@th.compiler.disable
def low_pass_filter(
    x: th.Tensor,
    filter_options: FilterOptions,
    freq_div: float = 1.0,
    padding_mode: str = "reflection",
) -> th.Tensor:
    """Low-pass filter an NCHW tensor without changing its spatial size.

    Args:
        x: Input tensor with shape ``(N, C, H, W)``.
        filter_options: Interpolation filter options.
        freq_div: Frequency divider. The cutoff frequency is reduced by this factor. Default is ``1.0``.
        padding_mode: Border handling, ``"zeros"`` or ``"reflection"``. Default is ``"reflection"``.
    """
    return th.ops.filter2d_ext.low_pass_filter(
        x.contiguous(), filter_options.n_taps, freq_div, filter_options.alias_guard_band, filter_options.filter_type.value,
        _use_reflection_padding(padding_mode))


@th.compiler.disable
def make_resampling_kernel(
    filter_options: FilterOptions,
    m: int = 1,
    freq_div: float = 1.0,
    gain: float = 1.0,
    device: Optional[th.device] = None,
) -> th.Tensor:
    """Build a 1D low-pass resampling filter: float32, ``m * n_taps`` long.

    The result is cached per (parameters, device): a repeated call returns the same tensor, which is therefore not to be
    modified in place.  The first call for a key on a HIP device copies host memory to the device, so it belongs before a
    graph capture; `upsample`, `downsample` and `low_pass_filter` make this call themselves.

    Args:
        filter_options: Interpolation filter options.
        m: Upsampling or downsampling factor. Default is ``1``.
        freq_div: Frequency divider. The cutoff frequency is reduced by this factor. Default is ``1.0``.
        gain: Kernel values sum to this value. Use ``gain == m`` when upsampling to preserve signal magnitude. Default is
            ``1.0``.
        device: Device for the returned filter tensor. Default is CPU.
    """
    if device is None:
        device = th.device("cpu")
    if not isinstance(device, th.device):
        device = th.device(device)
    return th.ops.filter2d_ext.make_resampling_kernel(
        filter_options.n_taps, m, freq_div, gain, filter_options.alias_guard_band, filter_options.filter_type.value, device)
