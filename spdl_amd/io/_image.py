"""Image operators (drop-in for the reference's spdl.io image surface).

Reference signatures:
  decode_image_nvjpeg      src/spdl/io/_core.py:868-915
  load_image_batch_nvjpeg  src/spdl/io/_composite.py:486-524
  load_image_batch         src/spdl/io/_composite.py:358-465
  load_image               src/spdl/io/_composite.py:254-295
All of them decode on the GPU (gfx950 kernels); there is no CPU path.
"""

from __future__ import annotations

import logging
import os
import warnings
from collections.abc import Mapping, Sequence
from dataclasses import dataclass

import numpy as np
import torch

from .. import _lib
from .._lib import Output
from ._buffer import CPUBuffer, CUDABuffer
from ._config import CUDAConfig
from ._preprocessing import get_video_filter_desc, parse_image_filter

_LG = logging.getLogger(__name__)

_FILTER_DESC_DEFAULT = "__SPDL_DEFAULT__"


def _read(src) -> memoryview:
    if isinstance(src, (bytes, bytearray, memoryview)):
        return memoryview(src)
    if isinstance(src, str):
        with open(src, "rb") as f:
            return memoryview(f.read())
    if isinstance(src, np.ndarray):
        return memoryview(src.tobytes())
    raise TypeError(
        f"Source must be `str` (path), `bytes` (data), or `memoryview`. Found: {type(src)}"
    )


def _stream(cfg: CUDAConfig) -> int:
    return int(cfg.stream)


def _default_config() -> CUDAConfig:
    """The device a call without ``device_config`` decodes on: the current
    HIP device once torch has initialised it (a rank that called
    ``torch.cuda.set_device``), else ``$LOCAL_RANK`` (one process per GPU,
    torch.distributed.run), else 0 -- never a hard-wired device 0 for every
    rank of a job."""
    if torch.cuda.is_initialized():
        return CUDAConfig(torch.cuda.current_device())
    rank = int(os.environ.get("LOCAL_RANK", "0") or 0)
    count = torch.cuda.device_count()
    return CUDAConfig(rank if 0 <= rank < count else 0)


# FFmpeg demux / decoder options of the reference's CPU path.  The GPU
# decoder has no equivalent knobs (its parser and decoder are fixed), so
# they are accepted for drop-in compatibility and, when set, reported once.
_IGNORED_WARNED: set = set()


def _ignore_ffmpeg_configs(kwargs: dict) -> None:
    for k in ("demux_config", "decode_config"):
        v = kwargs.pop(k, None)
        if v is not None and k not in _IGNORED_WARNED:
            _IGNORED_WARNED.add(k)
            warnings.warn(f"`{k}` configures FFmpeg's demuxer/decoder, which the GPU decode "
                          f"stage does not use; it is ignored", RuntimeWarning, stacklevel=3)


@dataclass(frozen=True)
class DecodeConfig:
    """The reference's ``spdl.io.DecodeConfig``, the two fields the image path
    reads: of ``decoder_options`` the GPU decoder honours ``"lowres"``."""

    decoder: str | None = None
    decoder_options: dict | None = None


def decode_config(decoder: str | None = None, decoder_options: dict | None = None) -> DecodeConfig:
    """``spdl.io.decode_config``: ``decode_config(decoder_options={"lowres": "1"})``
    asks for FFmpeg's reduced-size decode, here ``lowres=1``."""
    return DecodeConfig(decoder, decoder_options)


def _ffmpeg_configs(kwargs: dict, lowres):
    """``demux_config`` / ``decode_config`` off ``kwargs``.  Of the decoder's
    options ``"lowres"`` (a str or an int, FFmpeg's 0..3) is honoured and
    returned as ``lowres=`` -- which it must equal when both are given; every
    other option, a decoder name and ``demux_config`` keep the once-only
    warning of :func:`_ignore_ffmpeg_configs`."""
    cfg = kwargs.get("decode_config")
    opts = None if cfg is None else (cfg.get("decoder_options") if isinstance(cfg, Mapping)
                                     else getattr(cfg, "decoder_options", None))
    level = None
    if opts is not None and "lowres" in opts:
        try:
            level = int(opts["lowres"])
        except (TypeError, ValueError):
            raise ValueError(f"decoder_options['lowres'] = {opts['lowres']!r} is no integer") from None
        if lowres is not None and lowres != level:
            raise ValueError(f"lowres={lowres!r} and decode_config's lowres {level} disagree")
        named = cfg.get("decoder") if isinstance(cfg, Mapping) else getattr(cfg, "decoder", None)
        if named is None and len(opts) == 1:
            kwargs.pop("decode_config")  # (nothing in it goes unused: no warning)
    _ignore_ffmpeg_configs(kwargs)
    return lowres if level is None else level


def _no_crops_with_lowres(levels, crops, out: Output) -> None:
    if levels is not None and (crops is not None or out.src_crop is not None):
        raise ValueError("lowres= and a source crop are exclusive")


def _alloc_out(cfg: CUDAConfig, shape, dtype) -> CUDABuffer:
    nbytes = int(np.prod(shape)) * (1 if dtype == torch.uint8 else 2)
    if cfg.allocator is None:
        t = torch.empty(shape, dtype=dtype, device=f"cuda:{cfg.device_index}")
        return CUDABuffer(t, stream=cfg.stream)
    alloc, free = cfg.allocator
    ptr = int(alloc(nbytes, cfg.device_index, cfg.stream))
    if not ptr:
        raise RuntimeError("allocator returned a null pointer")
    return CUDABuffer(None, ptr=ptr, shape=tuple(shape), dtype=dtype,
                      device_index=cfg.device_index, stream=cfg.stream, deleter=free)


def _decode(datas: list, out: Output, cfg: CUDAConfig, shape_per_image, batched: bool,
            dtype=torch.uint8, crops=None, flips=None, orients=None, lowres=None) -> CUDABuffer:
    n = len(datas)
    shape = (n, *shape_per_image) if batched else tuple(shape_per_image)
    buf = _alloc_out(cfg, shape, dtype)
    dec = _lib.thread_decoder(cfg.device_index)
    nbytes = int(np.prod(shape)) * (1 if dtype == torch.uint8 else 2)
    dec.decode_batch(datas, out, buf.data_ptr(), nbytes, stream=_stream(cfg), sync=True,
                     crops=crops, flips=flips, orients=orients, lowres=lowres)
    return buf


def _oriented_size(src, out: Output, code: int):
    """The final ``(ow, oh)`` of a ``src = (w, h)`` frame under orientation
    ``code``: a transposed image is sized from the stored frame's ``(h, w)``."""
    return _lib.output_size(*(src[::-1] if code & 4 else src), out)


def _exif_codes(datas, out: Output, flips):
    """``exif_orientation=True``: each file's EXIF orientation as its code, the
    caller's flip on top -- it acts on the displayed image, so the bits xor --
    and ``out`` without its flip, which the codes now hold."""
    if out.orient is not None:
        raise ValueError("exif_orientation= and transpose in filter_desc are exclusive")
    every = _lib._flip(out.flip)
    codes = [_lib.exif_code(_lib.get_orientation(d)) ^ (every if flips is None else flips[k])
             for k, d in enumerate(datas)]
    if out.flip is not None:
        out = Output(**{**out.__dict__, "flip": None})
    return out, codes


def _src_size(info, rect) -> tuple[int, int]:
    """The frame the chain sees: the image, or its source crop ``rect``
    resolved as the decoder resolves it (``None``: no crop)."""
    if rect is None:
        return info.width, info.height
    rc, r = _lib.crop_rect(info, rect)
    if rc:
        raise RuntimeError(f"Failed to decode an image. (invalid source crop {tuple(rect)} of a "
                           f"{info.width}x{info.height} image)")
    return r[2], r[3]


def _shape(out: Output, w: int, h: int) -> tuple:
    return (3, h, w) if out.planar else (h, w, 3)


def _frame_format(info) -> tuple[int, int, bool]:
    """(hs, vs, gray): the chroma ratios of the planar frame FFmpeg's decoder
    makes of this file, for the ``pix_fmt="yuv"`` output; the frames
    convert_frames has no layout for raise as :func:`_native_planes` does."""
    fmt = _UNSUPPORTED_FRAMES.get(info.color)
    if fmt is not None:
        raise RuntimeError(f"Unsupported pixel format: {fmt}")
    if info.ncomp == 1:
        return 1, 1, True
    h, v = list(info.h_samp[:3]), list(info.v_samp[:3])
    hs, vs = h[0] // max(h[1], 1), v[0] // max(v[1], 1)
    if (h[1], v[1]) != (h[2], v[2]) or h[0] != hs * h[1] or v[0] != vs * v[1] or \
            (hs, vs) not in ((1, 1), (2, 1), (2, 2)):
        raise RuntimeError(
            f"Unsupported pixel format: sampling {h[0]}x{v[0]},{h[1]}x{v[1]},{h[2]}x{v[2]}")
    return hs, vs, False


def _yuv_shape(infos: list, out: Output, size=None) -> tuple:
    """Per-image shape of the ``pix_fmt="yuv"`` result of these images (one
    frame format, one output size), or the reference's error.  ``size``: the
    first image's source crop size when it has one."""
    fmts = [_frame_format(i) for i in infos]
    ow, oh = _lib.output_size(*(size or (infos[0].width, infos[0].height)), out)
    if any(f != fmts[0] for f in fmts):
        raise RuntimeError("The input images must have the same size and pixel format.")
    return _lib.planar_layout(ow, oh, *fmts[0])[0]


def decode_image_nvjpeg(
    src,
    *,
    device_config: CUDAConfig | None = None,
    scale_width: int = -1,
    scale_height: int = -1,
    pix_fmt: str = "rgb",
    sync: bool = True,
    scale_algo: str = "lanczos",
    lowres=None,
) -> CUDABuffer:
    """Decode JPEG(s) on the GPU.  Same contract as the reference: a single
    source gives ``[3,H,W]`` (``"rgb"``/``"bgr"``) or ``[H,W,3]``
    (``"rgb24"``/``"bgr24"``), resized (stretch) when both scale sizes are
    positive; a sequence gives ``[B,...]`` and requires the scale sizes.

    ``scale_algo`` (an addition; the reference has no such argument) picks
    the resampling kernel.  The default ``"lanczos"`` is Lanczos-3, the
    kernel of the reference's ``resize_npp`` (NPPI_INTER_LANCZOS,
    src/libspdl/cuda/npp/detail/resize.cpp:36-116); ``"bicubic"`` /
    ``"bilinear"`` are the CPU path's swscale flags.  ``lowres`` (an addition
    as well): the reduced-size decode of :func:`load_image_batch`."""
    if device_config is None:
        raise ValueError("device_config must be provided.")
    if scale_algo not in _lib.FILTERS:
        raise ValueError(f"Unexpected scale_algo: {scale_algo}. Supported: {list(_lib.FILTERS)}")
    if pix_fmt not in _lib.PIX_FMTS:
        raise RuntimeError(
            f'Unexpected pix_fmt: {pix_fmt}. Supported values are "bgr", "bgr24", "rgb", "rgb24"'
        )
    if isinstance(src, Sequence) and not isinstance(src, (str, bytes, bytearray, memoryview)):
        datas = [_read(s) for s in src]
        if not datas:
            raise RuntimeError("No input is provided.")
        # the reference rejects only when both are missing
        # (nvjpeg/decoding.cpp:219-221); one missing size would size its
        # output buffer with a non-positive dimension and fail there
        if scale_width <= 0 and scale_height <= 0:
            raise RuntimeError("Both `scale_width` and `scale_height` must be specified.")
        if scale_width <= 0 or scale_height <= 0:
            raise RuntimeError(
                f"Failed to allocate the output buffer: invalid size {scale_width}x{scale_height}.")
        out = Output(pix_fmt=pix_fmt, resize=True, fit_w=scale_width, fit_h=scale_height,
                     filter=scale_algo)
        levels = None
        if lowres is not None:
            levels = _lib.lowres_levels(lowres, [_lib.get_image_info(d) for d in datas], out)
        return _decode(datas, out, device_config, _shape(out, scale_width, scale_height), True,
                       lowres=levels)
    data = _read(src)
    info = _lib.get_image_info(data) if lowres is not None else None
    if scale_width > 0 and scale_height > 0:
        out = Output(pix_fmt=pix_fmt, resize=True, fit_w=scale_width, fit_h=scale_height,
                     filter=scale_algo)
        w, h = scale_width, scale_height
    else:
        out = Output(pix_fmt=pix_fmt)
        info = info or _lib.get_image_info(data)
        w, h = info.width, info.height
    levels = None if lowres is None else _lib.lowres_levels(lowres, [info], out)
    if levels is not None and not out.resize:
        w, h = _lib.lowres_size(w, h, levels[0])
    return _decode([data], out, device_config, _shape(out, w, h), False, lowres=levels)


def load_image_batch_nvjpeg(
    srcs,
    *,
    device_config: CUDAConfig,
    width: int,
    height: int,
    pix_fmt: str = "rgb",
    scale_algo: str = "lanczos",
    lowres=None,
) -> CUDABuffer:
    """Batch load + resize (reference _composite.py:486-524): stretch to
    ``width`` x ``height`` with the ``resize_npp`` kernel (Lanczos-3) unless
    ``scale_algo`` says otherwise.  ``lowres``: :func:`load_image_batch`'s."""
    return decode_image_nvjpeg(
        [_read(s) for s in srcs],
        scale_width=width,
        scale_height=height,
        device_config=device_config,
        pix_fmt=pix_fmt,
        scale_algo=scale_algo,
        lowres=lowres,
    )


def _to_host(buf: CUDABuffer, storage=None) -> CPUBuffer:
    """Device result -> host buffer.  With ``storage`` (a :class:`CPUStorage`,
    usually pinned) the bytes land in it, as the reference's convert_frames
    writes the batch into the caller's storage
    (src/spdl/io/_composite.py:368,460 -> src/libspdl/core/buffer.cpp:48-69,
    which raises when the storage is too small)."""
    from ._convert import to_torch
    from ._transfer import transfer_buffer_cpu

    if storage is None:
        t = to_torch(buf).cpu()
        if t.dtype == torch.bfloat16:  # numpy has no bfloat16: keep the bit patterns
            return CPUBuffer(t.view(torch.int16).numpy().view(np.uint16), dtype=torch.bfloat16)
        return CPUBuffer(t.numpy())
    nbytes = int(np.prod(buf.shape)) * (1 if buf.dtype == torch.uint8 else 2)
    if storage.size < nbytes:
        raise RuntimeError(
            f"The provided storage does not have enough capacity. ({storage.size} < {nbytes})")
    return transfer_buffer_cpu(buf, storage=storage)


_LOAD_CSC = ("swscale", "turbo")


def _check_csc(csc: str, *, width=None, height=None, crops=None, flips=None,
               exif_orientation: bool = False, lowres=None, pix_fmt="rgb24") -> None:
    """``csc=`` of the ``load_image*`` functions, held before anything is read
    or submitted.  ``"turbo"`` is the whole frame at its own size
    (include/spdl_hipjpeg.h "Pillow-exact decode"): no scale, crop, flip,
    orientation or reduced-size level (all-zero levels are none), and an RGB
    ``pix_fmt``.  These functions take ``"swscale"`` and ``"turbo"``;
    ``"jfif"`` stays with :class:`Output` and the ``Decoder``."""
    if csc not in _LOAD_CSC:
        raise ValueError(f"csc must be one of {list(_LOAD_CSC)}, not {csc!r}")
    if csc != "turbo":
        return
    bad = None
    if width is not None or height is not None:
        bad = "width= / height= (it does not scale)"
    elif crops is not None:
        bad = "crops="
    elif flips is not None:
        bad = "flips="
    elif exif_orientation:
        bad = "exif_orientation="
    elif isinstance(lowres, str) or np.any(np.asarray(0 if lowres is None else lowres) != 0):
        bad = "lowres="
    elif pix_fmt is None:
        bad = "pix_fmt=None (it converts to RGB)"
    if bad:
        raise ValueError(f"csc='turbo' is the full-resolution decode alone: it takes no {bad}")


def _csc_pix_fmt(filter_desc, pix_fmt):
    """The ``pix_fmt`` :func:`_check_csc` judges: none without a chain; the
    argument with the default chain; with a chain of the caller's the chain
    decides (its format node, else ``pix_fmt``), and :func:`_with_csc` holds
    the parsed result."""
    if filter_desc is None:
        return None
    return pix_fmt if filter_desc == _FILTER_DESC_DEFAULT else "rgb24"


def _with_csc(out: Output, csc: str) -> Output:
    """``out`` converting with ``csc``; a chain ``"turbo"`` cannot run (a scale,
    pad, crop, flip or transpose node, no format) is refused here."""
    if csc == "swscale":
        return out
    if csc == "turbo" and (out.resize or out.src_crop is not None or out.flip is not None or
                           out.orient is not None or out.pix_fmt == "yuv"):
        raise ValueError("csc='turbo' is the full-resolution decode alone: filter_desc may hold "
                         "a format node and nothing else")
    return Output(**{**out.__dict__, "csc": csc})


def load_image_batch(
    srcs,
    *,
    width: int | None,
    height: int | None,
    pix_fmt: str | None = "rgb24",
    filter_desc: str | None = _FILTER_DESC_DEFAULT,
    device_config: CUDAConfig | None = None,
    strict: bool = True,
    normalize: bool = False,
    mean=(0.485, 0.456, 0.406),
    std=(0.229, 0.224, 0.225),
    norm_dtype: str = "float16",
    crops=None,
    flips=None,
    exif_orientation: bool = False,
    lowres=None,
    csc: str = "swscale",
    **kwargs,
):
    """Batch load images into one ``[B,H,W,3]`` buffer with the FFmpeg filter
    semantics of the reference CPU path (scale + centred pad by default).
    ``pix_fmt=None`` leaves the format node out: the chain then runs on the
    decoder's own planar format and the batch holds the scaled planes as the
    reference's convert_frames stacks them (``[B,1,H+H/2,W]`` yuvj420p,
    ``[B,1,2H,W]`` yuvj422p, ``[B,3,H,W]`` yuvj444p, ``[B,H,W,1]`` gray).

    Decoding runs on ``device_config``'s GPU (when absent: the current HIP
    device, or ``$LOCAL_RANK``); without a ``device_config`` the result is
    copied back to a host ``CPUBuffer`` -- into ``storage`` when one is given
    (a :func:`cpu_storage`), like the reference's return type.  ``normalize=True`` fuses the ImageNet
    epilogue ((x/255 - mean)/std in fp32 -> ``norm_dtype`` float16 or
    bfloat16), an extension for config 4.

    ``crops`` (an extension, like ``normalize``): one source crop ``(x, y, w,
    h)`` or ``None`` per image, taken from the decoder's frame before the
    chain -- RandomResizedCrop's per-image rectangles with ``width=224,
    height=224``; ``x`` or ``y`` of ``None`` is centred.  Exclusive with a
    positioned ``crop`` node ahead of ``scale`` in ``filter_desc``, which
    crops every image alike.

    ``flips`` (an extension as well): one output flip per image -- ``0..3``
    (bit 0 horizontal, bit 1 vertical), ``"h"``, ``"v"``, ``"hv"`` or ``None``
    -- applied to the chain's result, as ``hflip`` / ``vflip`` at the end of
    ``filter_desc`` do for every image alike (exclusive with those); a
    RandomHorizontalFlip in the decode's own store.  A full-resolution batch
    with a flip takes the generic output kernel.

    ``exif_orientation=True`` (an extension; torchvision's
    ``apply_exif_orientation``, Pillow's ``exif_transpose``) reads each file's
    EXIF orientation and decodes the image as a viewer shows it: ``width`` and
    ``height`` are those of the displayed image, a rotated file runs the chain
    sideways, and every image of the batch has one shape.  ``flips`` then act
    on the displayed image.  A ``transpose`` at the end of ``filter_desc``
    turns every image alike (exclusive with ``exif_orientation``).

    ``lowres``: FFmpeg's reduced-size decode, which the reference reaches
    through ``decode_config=decode_config(decoder_options={"lowres": "1"})``
    (honoured here as well; the two must agree).  Level ``L`` in ``1..3``
    inverse-transforms only the low ``(8 >> L)`` corner of each block: the
    decoder's frame is ``ceil(w / 2^L) x ceil(h / 2^L)`` and the chain runs on
    it -- other pixels than the full decode's, for a fraction of the IDCT and
    output work.  An int for every image, a list per image, or ``"auto"`` (an
    extension): per image the largest level that keeps the frame no smaller
    than what the chain scales it to.  Exclusive with source crops.

    ``csc="turbo"`` (an extension): Pillow's pixels -- libjpeg-turbo's default
    decoder, ``np.asarray(PIL.Image.open(f).convert("RGB"))`` byte for byte --
    for files of one size at that size: ``width=None, height=None``, an RGB
    ``pix_fmt``, and none of ``crops``, ``flips``, ``exif_orientation``,
    ``lowres`` (files of mixed sizes: :func:`load_image_list`)."""
    if not srcs:
        raise ValueError("`srcs` must not be empty.")
    storage = kwargs.pop("storage", None)
    lowres = _ffmpeg_configs(kwargs, lowres)
    if kwargs:
        raise TypeError(f"unexpected arguments: {sorted(kwargs)}")
    _check_csc(csc, width=width, height=height, crops=crops, flips=flips,
               exif_orientation=exif_orientation, lowres=lowres,
               pix_fmt=_csc_pix_fmt(filter_desc, pix_fmt))
    if filter_desc == _FILTER_DESC_DEFAULT:
        filter_desc = get_video_filter_desc(
            scale_width=width, scale_height=height, pix_fmt=pix_fmt
        )
    cfg = device_config or _default_config()
    if crops is not None:
        crops = list(crops)
        if len(crops) != len(srcs):
            raise ValueError(f"{len(crops)} crops for {len(srcs)} images")
        if filter_desc is None:
            raise ValueError("crops= needs a filter chain (width / height, filter_desc or pix_fmt)")
    if flips is not None:
        flips = [_lib._flip(f) for f in flips]
        if len(flips) != len(srcs):
            raise ValueError(f"{len(flips)} flips for {len(srcs)} images")
        if filter_desc is None:
            raise ValueError("flips= needs a filter chain (width / height, filter_desc or pix_fmt)")
    if exif_orientation and filter_desc is None:
        raise ValueError("exif_orientation= needs a filter chain (width / height, filter_desc or "
                         "pix_fmt)")
    if filter_desc is None:
        # no scale and no output format: the decoder's own planes, batched as
        # the reference's convert_frames stacks them ([B, 3, H, W] yuvj444p,
        # [B, 1, 1.5H, W] yuvj420p, [B, H, W, 1] gray; same size and format)
        dec = _lib.thread_decoder(cfg.device_index)
        arrs = []
        for i, s in enumerate(srcs):
            try:
                data = _read(s)
                lv = _lib.lowres_levels(lowres if isinstance(lowres, (int, str, type(None)))
                                        else [lowres[i]], [_lib.get_image_info(data)], Output())
                arrs.append(_native_planes(dec.decode_planes(data, stream=_stream(cfg),
                                                             lowres=lv[0] if lv else 0), data))
            except Exception as err:  # reference: log, skip, raise later if strict
                _LG.error("Failed to load image %d: %s", i, err)
        if strict and len(arrs) != len(srcs):
            raise RuntimeError("Failed to load some images.")
        if not arrs:
            raise RuntimeError("Failed to load all the images.")
        if any(a.shape != arrs[0].shape for a in arrs):
            raise RuntimeError("The input images must have the same size and pixel format.")
        arr = np.stack(arrs)
        if device_config is not None:
            return CUDABuffer(torch.from_numpy(arr).to(f"cuda:{cfg.device_index}"))
        if storage is not None:
            from ._transfer import convert_array

            return convert_array(arr, storage=storage)
        return CPUBuffer(arr)
    # (no format node and pix_fmt=None: the decoder's own planes, scaled)
    out = _with_csc(parse_image_filter(filter_desc, default_pix_fmt=pix_fmt), csc)
    if crops is not None and out.src_crop is not None:
        raise ValueError("crops= and a source crop in filter_desc are exclusive")
    if flips is not None and out.flip is not None:
        raise ValueError("flips= and hflip / vflip in filter_desc are exclusive")
    if normalize:
        if out.pix_fmt == "yuv":
            raise ValueError("normalize=True needs an RGB pix_fmt; pix_fmt=None keeps the "
                             "decoder's planar format")
        out = Output(**{**out.__dict__, "normalize": True, "mean": tuple(mean),
                        "std": tuple(std), "norm_dtype": norm_dtype})
    datas, keep = [], []
    for i, s in enumerate(srcs):
        try:
            d = _read(s)
            _lib.get_image_info(d)
        except Exception as err:  # reference logs and skips (strict=False)
            _LG.error("Failed to load image %d: %s", i, err)
            continue
        datas.append(d)
        keep.append(i)
    if strict and len(datas) != len(srcs):
        raise RuntimeError("Failed to load some images.")
    if not datas:
        raise RuntimeError("Failed to load all the images.")
    info = _lib.get_image_info(datas[0])
    if crops is not None:
        crops = [crops[i] for i in keep]
    if flips is not None:
        flips = [flips[i] for i in keep]
    orients = None
    if exif_orientation:
        out, orients = _exif_codes(datas, out, flips)
        flips = None
    infos = [_lib.get_image_info(d) for d in datas]
    if lowres is not None and not isinstance(lowres, (int, str)):
        if len(lowres) != len(srcs):
            raise ValueError(f"{len(lowres)} lowres levels for {len(srcs)} images")
        lowres = [lowres[i] for i in keep]
    levels = _lib.lowres_levels(lowres, infos, out, orients)
    _no_crops_with_lowres(levels, crops, out)
    src = _src_size(info, crops[0] if crops is not None else out.src_crop)
    if levels is not None:  # (the chain sees the reduced frame)
        src = _lib.lowres_size(*src, levels[0])
    ow, oh = _oriented_size(src, out, orients[0] if orients else _lib._orient(out.orient))
    dtype = out.torch_dtype
    if out.pix_fmt == "yuv":
        shape = _yuv_shape(infos, out, src)
    else:
        shape = _shape(out, ow, oh)
    try:
        buf = _decode(datas, out, cfg, shape, True, dtype=dtype, crops=crops, flips=flips,
                      orients=orients, lowres=levels)
    except RuntimeError:
        if strict:
            raise
        # decode one by one to find the survivors (rare path)
        good = []
        for k, d in enumerate(datas):
            try:
                good.append(_decode([d], out, cfg, shape, True, dtype=dtype,
                                    crops=None if crops is None else [crops[k]],
                                    flips=None if flips is None else [flips[k]],
                                    orients=None if orients is None else [orients[k]],
                                    lowres=None if levels is None else [levels[k]]))
            except RuntimeError as err:
                _LG.error("Failed to decode an image: %s", err)
        if not good:
            raise RuntimeError("Failed to load all the images.") from None
        from ._convert import to_torch

        buf = CUDABuffer(torch.cat([to_torch(g) for g in good]), stream=cfg.stream)
    if device_config is None:
        # the reference's CPU result, in the caller's storage when given (with
        # a device_config the reference only stages through it on the way to
        # the device; here the batch is decoded on the device directly)
        return _to_host(buf, storage)
    return buf


_VIEW_GROUP_KEYS = ("width", "height", "scale_algo", "scale_mode", "pix_fmt", "normalize", "dtype",
                    "mean", "std", "crops", "flips")


def _view_group_output(g) -> Output:
    """The output chain of one ``load_image_views`` group: its image
    arguments, as ``load_image_batch`` reads them."""
    if not hasattr(g, "keys"):
        raise ValueError("a group is a mapping of image arguments plus crops=")
    unknown = sorted(set(g.keys()) - set(_VIEW_GROUP_KEYS))
    if unknown:
        raise ValueError(f"unknown group keys {unknown}; a group takes {list(_VIEW_GROUP_KEYS)}")
    if "crops" not in g:
        raise ValueError("a group needs crops=[[rect, ...] per image]")
    pix_fmt = g.get("pix_fmt", "rgb24")
    if pix_fmt not in ("rgb", "bgr", "rgb24", "bgr24"):
        raise ValueError(f"a group's pix_fmt is rgb, bgr, rgb24 or bgr24, not {pix_fmt!r}")
    desc = get_video_filter_desc(scale_width=g.get("width"), scale_height=g.get("height"),
                                 scale_algo=g.get("scale_algo", "bicubic"),
                                 scale_mode=g.get("scale_mode", "pad"), pix_fmt=pix_fmt)
    out = parse_image_filter(desc, default_pix_fmt=pix_fmt)
    if g.get("normalize", False):
        dtype = g.get("dtype", "float16")
        if dtype not in _lib.NORM_DTYPES:
            raise ValueError(f"a normalised group's dtype is float16 or bfloat16, not {dtype!r}")
        out = Output(**{**out.__dict__, "normalize": True,
                        "mean": tuple(g.get("mean", Output.mean)),
                        "std": tuple(g.get("std", Output.std)), "norm_dtype": dtype})
    return out


def load_image_views(srcs, groups, *, device_config: CUDAConfig, strict: bool = True,
                     exif_orientation: bool = False):
    """Several crops and sizes of every image from one decode (an extension,
    like ``crops=`` and ``normalize=``): multi-crop augmentation, a thumbnail
    beside a training crop.  Every file is parsed and entropy-decoded once and
    inverse-transformed over the rectangle its views cover; each group then
    scales its views through its own chain into its own buffer.

    ``groups``: mappings of ``load_image_batch``'s image arguments -- ``width``,
    ``height``, ``scale_algo``, ``scale_mode``, ``pix_fmt``, ``normalize``,
    ``dtype`` ("float16" / "bfloat16"), ``mean``, ``std`` -- plus
    ``crops=[[rect, ...] per image]``: the source rectangles ``(x, y, w, h)``
    (``None``: the whole frame) this group takes of each image, any number,
    none included.  At most four groups.  ``flips=[[flip, ...] per image]``,
    parallel to ``crops``, mirrors single views (``0..3``, ``"h"``, ``"v"``,
    ``"hv"`` or ``None``; left out: no view of the group is flipped).
    ``exif_orientation=True`` reads each image's EXIF orientation and applies
    it to every view of that image (the rectangles stay in the stored frame's
    coordinates; ``width`` / ``height`` are the displayed view's; a view's flip
    acts on the displayed view).

    Returns one ``(buffer, image_indices)`` per group: ``buffer`` is
    ``[rows, H, W, 3]`` (``[rows, 3, H, W]`` planar) with rows in (image, rect)
    order and ``image_indices[r]`` the image row r was made of.
    ``strict=False`` drops the rows of failed images and refused rectangles
    (``image_indices`` says what remains); ``strict=True`` raises, as
    ``load_image_batch`` does."""
    if not srcs:
        raise ValueError("`srcs` must not be empty.")
    if device_config is None:
        raise ValueError("device_config must be provided.")
    groups = list(groups)
    if not 1 <= len(groups) <= 4:
        raise ValueError(f"1 to 4 groups, not {len(groups)}")
    outs = [_view_group_output(g) for g in groups]
    for g in groups:
        per_image = list(g["crops"])
        if len(per_image) != len(srcs):
            raise ValueError(f"{len(per_image)} crop lists for {len(srcs)} images")
        for rects in per_image:
            if isinstance(rects, (str, bytes)) or not hasattr(rects, "__iter__"):
                raise ValueError("crops= is a list of rectangles per image")
            for r in rects:
                _lib._view_rect(r)
        if g.get("flips") is not None:
            per_flip = [list(f) for f in g["flips"]]
            if [len(f) for f in per_flip] != [len(list(r)) for r in per_image]:
                raise ValueError("flips= is parallel to crops=: one flip per rectangle")
            for f in per_flip:
                for v in f:
                    _lib._flip(v)
    cfg = device_config
    datas, keep, infos = [], [], []
    for i, s in enumerate(srcs):
        try:
            d = _read(s)
            infos.append(_lib.get_image_info(d))
        except Exception as err:  # reference logs and skips (strict=False)
            _LG.error("Failed to load image %d: %s", i, err)
            continue
        datas.append(d)
        keep.append(i)
    if strict and len(datas) != len(srcs):
        raise RuntimeError("Failed to load some images.")
    if not datas:
        raise RuntimeError("Failed to load all the images.")
    # one submission: every group's views of the surviving images, (image, rect) order
    exif = [_lib.exif_code(_lib.get_orientation(d)) for d in datas] if exif_orientation else None
    vgroups, bufs, rows = [], [], []
    for g, out in zip(groups, outs):
        per_image = list(g["crops"])
        per_flip = None if g.get("flips") is None else [list(f) for f in g["flips"]]
        views, src_of, size = [], [], None
        for k, i in enumerate(keep):
            for j, r in enumerate(per_image[i]):
                f = None if per_flip is None else per_flip[i][j]
                if exif is not None:
                    views.append((k, r, None, exif[k] ^ _lib._flip(f)))
                else:
                    views.append((k, r) if per_flip is None else (k, r, f))
                src_of.append(i)
                if size is None:
                    rc, rr = _lib.crop_rect(infos[k], r)
                    if not rc:
                        size = _oriented_size((rr[2], rr[3]), out, exif[k] if exif else 0)
        if not views:
            raise ValueError("a group without any rectangle")
        if size is None:
            raise RuntimeError("Failed to decode an image. (no rectangle of a group resolves)")
        shape = (len(views), *_shape(out, *size))
        buf = _alloc_out(cfg, shape, out.torch_dtype)
        nbytes = int(np.prod(shape)) * (1 if out.torch_dtype == torch.uint8 else 2)
        vgroups.append(_lib.ViewGroup(out, views, buf.data_ptr(), nbytes))
        bufs.append(buf)
        rows.append(src_of)
    dec = _lib.thread_decoder(cfg.device_index)
    # (of the call's own spec only the IDCT counts; strict: a failed image or a
    # refused view raises here)
    status = dec.decode_batch(datas, Output(pix_fmt="rgb24"), 0, 0, stream=_stream(cfg), sync=True,
                              check=strict, views=vgroups)
    result = []
    from ._convert import to_torch

    for vg, buf, src_of in zip(vgroups, bufs, rows):
        ok = [r for r, ((k, _), st) in enumerate(zip(vg.views, vg.statuses))
              if st == 0 and status[k] == 0]
        if len(ok) != len(src_of):  # (strict=True raised above)
            for r in sorted(set(range(len(src_of))) - set(ok)):
                _LG.error("Failed to decode a view of image %d", src_of[r])
            if not ok:
                raise RuntimeError("Failed to load all the images.")
            idx = torch.tensor(ok, device=f"cuda:{cfg.device_index}")
            buf = CUDABuffer(to_torch(buf).index_select(0, idx), stream=cfg.stream)
        result.append((buf, [src_of[r] for r in ok]))
    return result


_LIST_ASPECT = {None: None, "fit": "decrease", "cover": "increase"}


def _list_filter_desc(width, height, scale_mode, scale_algo: str, pix_fmt: str) -> str:
    """The chain of ``load_image_list``'s image arguments: one ``scale`` node
    (none at native size) and the format.  ``scale_mode=None``: exactly
    ``scale=w:h``, a missing side ``-1`` (vf_scale: keep the aspect).  ``"fit"``
    and ``"cover"``: ``force_original_aspect_ratio=decrease`` / ``increase``
    with neither the pad nor the crop that bring ``load_image_batch``'s images
    to one box -- a missing side is the other one, a square box."""
    if scale_mode not in _LIST_ASPECT:
        raise ValueError(f"scale_mode must be 'fit', 'cover' or None, got {scale_mode!r}")
    if width is None and height is None:
        if scale_mode is not None:
            raise ValueError(f"scale_mode={scale_mode!r} needs a width or a height")
        return get_video_filter_desc(pix_fmt=pix_fmt)
    ratio = _LIST_ASPECT[scale_mode]
    if ratio is None:
        w, h = (-1 if v is None else int(v) for v in (width, height))
        if w < 0 and h < 0:
            raise ValueError("one of width and height must be a size")
        extra = ""
    else:
        w, h = (int(width if width is not None else height),
                int(height if height is not None else width))
        if w <= 0 or h <= 0:
            raise ValueError(f"scale_mode={scale_mode!r} needs a positive box, not {w}x{h}")
        extra = f":force_original_aspect_ratio={ratio}"
    return f"scale=w={w}:h={h}:flags={scale_algo}{extra},format=pix_fmts={pix_fmt}"


def load_image_list(
    srcs,
    *,
    width: int | None = None,
    height: int | None = None,
    scale_mode: str | None = None,
    scale_algo: str = "bicubic",
    pix_fmt: str | None = "rgb24",
    filter_desc: str | None = _FILTER_DESC_DEFAULT,
    device_config: CUDAConfig | None = None,
    strict: bool = True,
    normalize: bool = False,
    mean=(0.485, 0.456, 0.406),
    std=(0.229, 0.224, 0.225),
    norm_dtype: str = "float16",
    crops=None,
    flips=None,
    exif_orientation: bool = False,
    align: int = 256,
    csc: str = "swscale",
    lowres=None,
):
    """Every image at its own size from one submission (an extension, like
    :func:`load_image_views`; include/spdl_hipjpeg.h "ragged batches"): native
    resolution, or an aspect-preserving resize, neither of which
    :func:`load_image_batch` can hold in one ``[B,H,W,3]``.

    ``width = height = None`` keeps every file's size.  Otherwise
    ``scale_mode=None`` is exactly ``scale=w:h`` with a ``None`` or ``-1`` /
    ``-n`` side following the aspect ratio (vf_scale); ``"fit"`` scales the
    image into the box (the longer side meets it) and ``"cover"`` over it (the
    shorter side meets it, torchvision's ``Resize(int)``) -- ``load_image_batch``'s
    ``"pad"`` and ``"crop"`` without the pad and the crop.  A ``filter_desc``
    is any chain ``load_image_batch`` takes.  ``crops``, ``flips``,
    ``exif_orientation``, ``normalize`` and ``lowres`` are
    ``load_image_batch``'s; every box is sized from its image's reduced frame.
    ``csc="turbo"``: Pillow's pixels (libjpeg-turbo's default decoder, byte
    for byte) of every file at its native size -- no ``width`` / ``height``,
    ``crops``, ``flips``, ``exif_orientation`` or ``lowres`` with it.

    Returns ``(buffers, image_indices)``: one allocation, every buffer a view
    of it with its image's own shape (``[H,W,3]``, or ``[3,H,W]`` for ``rgb`` /
    ``bgr``) starting at a multiple of ``align`` bytes, and the index in
    ``srcs`` of each.  ``strict=False`` drops failed images (``image_indices``
    says what remains); ``strict=True`` raises.  Without a ``device_config``
    the buffers are host copies."""
    if not srcs:
        raise ValueError("`srcs` must not be empty.")
    if pix_fmt is None:
        raise ValueError("load_image_list needs an RGB pix_fmt: no ragged planar YUV output")
    if csc not in ("swscale", "turbo"):
        raise ValueError(f"load_image_list converts with csc='swscale' only, or with csc='turbo' "
                         f"at native size, not {csc!r}")
    _check_csc(csc, width=width, height=height, crops=crops, flips=flips,
               exif_orientation=exif_orientation, lowres=lowres, pix_fmt=pix_fmt)
    if filter_desc == _FILTER_DESC_DEFAULT:
        filter_desc = _list_filter_desc(width, height, scale_mode, scale_algo, pix_fmt)
    elif (width, height, scale_mode) != (None, None, None):
        raise ValueError("filter_desc= and width / height / scale_mode are exclusive")
    if filter_desc is None:
        raise ValueError("load_image_list needs a filter chain")
    n_src = len(srcs)
    per_lowres = None if lowres is None or isinstance(lowres, (int, str)) else lowres
    for name, per in (("crops", crops), ("flips", flips), ("lowres levels", per_lowres)):
        if per is not None and len(per) != n_src:
            raise ValueError(f"{len(per)} {name} for {n_src} images")
    if flips is not None:
        flips = [_lib._flip(f) for f in flips]
    out = _with_csc(parse_image_filter(filter_desc, default_pix_fmt=pix_fmt), csc)
    if out.pix_fmt == "yuv":
        raise ValueError("load_image_list needs an RGB pix_fmt: no ragged planar YUV output")
    if crops is not None and out.src_crop is not None:
        raise ValueError("crops= and a source crop in filter_desc are exclusive")
    if flips is not None and (out.flip is not None or out.orient is not None):
        raise ValueError("flips= and hflip / vflip / transpose in filter_desc are exclusive")
    if normalize:
        out = Output(**{**out.__dict__, "normalize": True, "mean": tuple(mean),
                        "std": tuple(std), "norm_dtype": norm_dtype})
    cfg = device_config or _default_config()
    datas, keep, infos = [], [], []
    for i, s in enumerate(srcs):
        try:
            d = _read(s)
            infos.append(_lib.get_image_info(d))
        except Exception as err:  # reference logs and skips (strict=False)
            _LG.error("Failed to load image %d: %s", i, err)
            continue
        datas.append(d)
        keep.append(i)
    if strict and len(datas) != n_src:
        raise RuntimeError("Failed to load some images.")
    if not datas:
        raise RuntimeError("Failed to load all the images.")
    n = len(datas)
    if crops is not None:
        crops = [crops[i] for i in keep]
    elif out.src_crop is not None:
        crops = [out.src_crop] * n
    if flips is not None:
        flips = [flips[i] for i in keep]
    # one code per image: the file's EXIF orientation, the chain's transpose, a flip
    if exif_orientation:
        out, codes = _exif_codes(datas, out, flips)
    else:
        every = _lib._orient(out.orient) if out.orient is not None else _lib._flip(out.flip)
        codes = [every if flips is None else flips[k] for k in range(n)]
    out = Output(**{**out.__dict__, "src_crop": None, "flip": None, "orient": None})
    codes = codes if any(codes) else None
    if per_lowres is not None:
        lowres = [per_lowres[i] for i in keep]
    levels = _lib.lowres_levels(lowres, infos, out, codes)
    _no_crops_with_lowres(levels, crops, out)
    offsets, sizes, planned = _lib.ragged_layout(infos, out, crops, codes, align, lowres=levels)
    esz = 1 if out.torch_dtype == torch.uint8 else 2
    # (every offset and every extent is a multiple of the element size)
    total = _alloc_out(cfg, (max(offsets[n] // esz, 1),), out.torch_dtype)
    dec = _lib.thread_decoder(cfg.device_index)
    status = dec.decode_batch(datas, out, total.data_ptr(), offsets[n], stream=_stream(cfg),
                              sync=True, check=False, crops=crops, orients=codes,
                              ragged=offsets[:n], lowres=levels)
    from ._convert import to_torch

    flat = to_torch(total)
    bufs, idx = [], []
    for k in range(n):
        if status[k] or planned[k]:
            _LG.error("Failed to decode image %d: status %d", keep[k], status[k] or planned[k])
            continue
        shape = _shape(out, *sizes[k])
        first = offsets[k] // esz
        t = flat[first:first + int(np.prod(shape))].view(shape)
        # (every view holds the allocation: with an allocator pair its deleter
        # runs when the last of them is gone)
        view = CUDABuffer(t, stream=cfg.stream, owner=total)
        bufs.append(view if device_config is not None else _to_host(view))
        idx.append(keep[k])
    if strict and len(bufs) != n:
        raise RuntimeError("Failed to load some images.")
    if not bufs:
        raise RuntimeError("Failed to load all the images.")
    return bufs, idx


_UNSUPPORTED_FRAMES = {2: "gbrp", 3: "gbrap", 4: "yuva444p", 5: "yuva444p"}  # by spdl_hj_color


def _native_planes(planes: list, data) -> np.ndarray:
    """The buffer the reference's convert_frames makes of an unfiltered
    frame (src/libspdl/core/detail/ffmpeg/conversion.cpp:172-303,411-454,
    single-frame form conversion.h:45-53): av_image_copy_to_buffer packs Y,
    then all of U, then all of V, each plane tightly, into
      gray8     [H, W, 1]        (convert_interleaved)
      yuvj444p  [3, H, W]        (convert_planer)
      yuvj420p  [1, H + H/2, W]  (convert_yuv420p)
      yuvj422p  [1, 2H, W]       (convert_yuv422p)
    A frame whose planes do not fit that shape (odd 4:2:0 / 4:2:2 sizes)
    fails the copy there ("Failed to copy image data."); other samplings
    (yuvj440p, yuvj411p) are "Unsupported pixel format", and so are the
    frames FFmpeg makes of RGB-coded and Adobe CMYK / YCCK files (gbrp,
    gbrap, yuva444p: not in convert_frames' list, conversion.cpp:420-444)."""
    fmt = _UNSUPPORTED_FRAMES.get(_lib.get_image_info(data).color)
    if fmt is not None:
        raise RuntimeError(f"Unsupported pixel format: {fmt}")
    if len(planes) == 1:
        return np.ascontiguousarray(planes[0])[:, :, None]
    (H, W), (ch, cw) = planes[0].shape, planes[1].shape
    flat = np.concatenate([np.ascontiguousarray(p).reshape(-1) for p in planes])
    if (ch, cw) == (H, W):
        return flat.reshape(3, H, W)
    if cw == (W + 1) // 2 and ch == (H + 1) // 2:
        shape = (1, H + H // 2, W)
    elif cw == (W + 1) // 2 and ch == H:
        shape = (1, 2 * H, W)
    else:
        raise RuntimeError(
            f"Unsupported pixel format: chroma {cw}x{ch} for a {W}x{H} image")
    if flat.size != shape[1] * shape[2]:
        raise RuntimeError("Failed to copy image data.")
    return flat.reshape(shape)


def load_image(
    src,
    *,
    filter_desc: str | None = _FILTER_DESC_DEFAULT,
    device_config: CUDAConfig | None = None,
    pix_fmt: str | None = "rgb24",
    flip=None,
    exif_orientation: bool = False,
    lowres=None,
    csc: str = "swscale",
    **kwargs,
):
    """Single image.  ``filter_desc=None`` returns the decoded planes in the
    layout of the reference's convert_frames of an unfiltered frame (Y, U, V
    back to back: ``[1, 1.5H, W]`` yuvj420p, ``[1, 2H, W]`` yuvj422p,
    ``[3, H, W]`` yuvj444p, ``[H, W, 1]`` gray; see :func:`_native_planes`);
    ``pix_fmt=None`` with a scale / pad / crop chain returns the same layout
    of the scaled planes (the chain runs on the frame's own format);
    otherwise RGB per the filter.  ``flip`` (an extension; ``0..3``, ``"h"``,
    ``"v"``, ``"hv"``) mirrors the chain's result, as ``hflip`` / ``vflip`` at
    the end of ``filter_desc`` do (exclusive with those).
    ``exif_orientation=True`` (an extension) applies the file's EXIF
    orientation, as in :func:`load_image_batch`; ``flip`` then acts on the
    displayed image.  ``lowres`` (``0..3`` or ``"auto"``) and a
    ``decode_config`` with the ``"lowres"`` decoder option: the reduced-size
    decode of :func:`load_image_batch`.  ``csc="turbo"`` (an extension):
    ``np.asarray(PIL.Image.open(f).convert("RGB"))`` byte for byte, in the
    ``pix_fmt``'s layout -- libjpeg-turbo's default decoder; no scaling chain,
    ``flip``, ``exif_orientation`` or ``lowres`` with it."""
    kwargs.pop("name", None)  # only names the source in FFmpeg demux errors
    lowres = _ffmpeg_configs(kwargs, lowres)
    if kwargs:
        raise TypeError(f"unexpected arguments: {sorted(kwargs)}")
    _check_csc(csc, flips=flip or None, exif_orientation=exif_orientation, lowres=lowres,
               pix_fmt=_csc_pix_fmt(filter_desc, pix_fmt))
    cfg = device_config or _default_config()
    data = _read(src)
    flip = _lib._flip(flip)
    if filter_desc is None:
        if flip or exif_orientation:
            raise ValueError("flip= and exif_orientation= need a filter chain (filter_desc or "
                             "pix_fmt)")
        dec = _lib.thread_decoder(cfg.device_index)
        lv = _lib.lowres_levels(lowres, [_lib.get_image_info(data)], Output())
        arr = _native_planes(dec.decode_planes(data, stream=_stream(cfg),
                                               lowres=lv[0] if lv else 0), data)
        if device_config is not None:
            return CUDABuffer(torch.from_numpy(arr).to(f"cuda:{cfg.device_index}"))
        return CPUBuffer(arr)
    if filter_desc == _FILTER_DESC_DEFAULT:
        filter_desc = get_video_filter_desc(pix_fmt=pix_fmt)
    out = _with_csc(parse_image_filter(filter_desc, default_pix_fmt=pix_fmt), csc)
    if flip:
        if out.flip is not None:
            raise ValueError("flip= and hflip / vflip in filter_desc are exclusive")
        out = Output(**{**out.__dict__, "flip": flip})
    if exif_orientation:
        out, (code,) = _exif_codes([data], out, None)
        out = Output(**{**out.__dict__, "orient": code})
    info = _lib.get_image_info(data)
    levels = _lib.lowres_levels(lowres, [info], out)
    _no_crops_with_lowres(levels, None, out)
    src = _src_size(info, out.src_crop)
    if levels is not None:  # (the chain sees the reduced frame)
        src = _lib.lowres_size(*src, levels[0])
    if out.pix_fmt == "yuv":  # pix_fmt=None, no format node: the frame's planes
        shape = _yuv_shape([info], out, src)
    else:
        shape = _shape(out, *_oriented_size(src, out, _lib._orient(out.orient)))
    buf = _decode([data], out, cfg, shape, False, lowres=levels)
    if device_config is None:
        return _to_host(buf)
    return buf
