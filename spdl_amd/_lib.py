"""ctypes binding of the gfx950 decode stage (``include/spdl_hipjpeg.h``).

The product path: every public operator in :mod:`spdl_amd.io` ends here, in
``spdl_amd/lib/libspdl_hipjpeg.so``.  There is no CPU fallback: a missing
library or a missing GPU raises immediately.
"""

from __future__ import annotations

import ctypes
import os
import threading
from dataclasses import dataclass, replace

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SPDL_AMD_LIB") or os.path.join(_HERE, "lib", "libspdl_hipjpeg.so")

ABI_VERSION = 7

# enums (mirror include/spdl_hipjpeg.h)
# "yuv": the frame's own planar format (SPDL_HJ_FMT_YUV, see planar_layout)
PIX_FMTS = {"rgb": 0, "bgr": 1, "rgb24": 2, "bgr24": 3, "yuv": 4}
ASPECT = {None: 0, "none": 0, "decrease": 1, "increase": 2}
FILTERS = {"bicubic": 0, "bilinear": 1, "lanczos": 2}
IDCT = {"simple": 0, "islow": 1}
CSC = {"swscale": 0, "jfif": 1, "turbo": 2}
DTYPE_U8, DTYPE_F16, DTYPE_BF16 = 0, 1, 2
NORM_DTYPES = {"float16": DTYPE_F16, "bfloat16": DTYPE_BF16}

EXPORTED = (
    "spdl_hj_abi_version",
    "spdl_hj_get_image_info",
    "spdl_hj_output_size",
    "spdl_hj_create",
    "spdl_hj_destroy",
    "spdl_hj_decode_batch",
    "spdl_hj_decode_batch_device",
    "spdl_hj_decode_planes",
    "spdl_hj_set_profiling",
    "spdl_hj_last_timings",
    "spdl_hj_stage_name",
    "spdl_hj_set_param",
    "spdl_hj_get_param",
    "spdl_hj_debug_entropy",
    "spdl_hj_debug_sws_plan",
    "spdl_hj_last_ticket",
    "spdl_hj_wait",
    "spdl_hj_staging_acquire",
    "spdl_hj_stream_wait",
    "spdl_hj_staging_fill",
    "spdl_hj_staging_read",
    "spdl_hj_decode_staged",
    "spdl_hj_tar_index",
    "spdl_hj_nv12_to_planar_rgb",
    "spdl_hj_copy",
    "spdl_hj_crop_rect",
    "spdl_hj_set_crops",
    "spdl_hj_set_views",
    "spdl_hj_set_flips",
    "spdl_hj_set_orients",
    "spdl_hj_get_orientation",
    "spdl_hj_orient_code",
    "spdl_hj_ragged_layout",
    "spdl_hj_set_ragged",
    "spdl_hj_set_lowres",
)


class ImageInfo(ctypes.Structure):
    _fields_ = [
        ("width", ctypes.c_int32),
        ("height", ctypes.c_int32),
        ("ncomp", ctypes.c_int32),
        ("h_samp", ctypes.c_int32 * 4),
        ("v_samp", ctypes.c_int32 * 4),
        ("color", ctypes.c_int32),  # spdl_hj_color: GRAY YCBCR RGB CMYK YCCK YCBCRK
        ("multiscan", ctypes.c_int32),  # progressive or non-interleaved (ABI 5)
    ]


CROP_CENTER = -(1 << 31)  # SPDL_HJ_CROP_CENTER: x or y of a source crop, "centred"


class Rect(ctypes.Structure):  # spdl_hj_rect
    _fields_ = [("x", ctypes.c_int32), ("y", ctypes.c_int32), ("w", ctypes.c_int32),
                ("h", ctypes.c_int32)]


def _rect(r) -> Rect:
    """``(x, y, w, h)`` -> spdl_hj_rect; ``None`` is no crop, an ``x`` or ``y``
    of ``None`` is centred."""
    if r is None:
        return Rect(0, 0, 0, 0)
    x, y, w, h = r
    return Rect(CROP_CENTER if x is None else int(x), CROP_CENTER if y is None else int(y),
                int(w), int(h))


FLIP_H, FLIP_V = 1, 2  # SPDL_HJ_FLIP_H, SPDL_HJ_FLIP_V
_FLIP_NAMES = {None: 0, "": 0, "h": FLIP_H, "v": FLIP_V, "hv": FLIP_H | FLIP_V,
               "vh": FLIP_H | FLIP_V}


def _flip(f) -> int:
    """An output flip, ``0..3`` (bit 0 horizontal, bit 1 vertical), ``"h"``,
    ``"v"``, ``"hv"`` or ``None`` -> SPDL_HJ_FLIP_* bits."""
    if isinstance(f, (str, type(None))):
        if f not in _FLIP_NAMES:
            raise ValueError(f"a flip is 0..3, 'h', 'v', 'hv' or None, not {f!r}")
        return _FLIP_NAMES[f]
    if isinstance(f, bool) or not isinstance(f, int) or not 0 <= f <= 3:
        raise ValueError(f"a flip is 0..3, 'h', 'v', 'hv' or None, not {f!r}")
    return int(f)


ORIENT_H, ORIENT_V, ORIENT_T = 1, 2, 4  # SPDL_HJ_ORIENT_*
# (the transposes by libavfilter's names for transpose=dir)
_ORIENT_NAMES = {**_FLIP_NAMES, "t": 4, "cclock_flip": 4, "clock": 5, "cclock": 6, "clock_flip": 7}
_ORIENT_WHAT = ("an orientation is 0..7, 'h', 'v', 'hv', 't', 'cclock_flip', 'clock', 'cclock', "
                "'clock_flip' or None")
# EXIF orientation (tag 0x0112) -> orientation code: the output is the image
# as a viewer shows it (spdl_hj_orient_code states the same table)
_EXIF_CODES = {1: 0, 2: 1, 3: 3, 4: 2, 5: 4, 6: 5, 7: 7, 8: 6}


def _orient(o) -> int:
    """An output orientation: ``0..7`` (bit 0 horizontal flip, bit 1 vertical,
    bit 2 a transpose ahead of them), a flip spelling, ``"t"`` or one of
    ``transpose``'s direction names -> SPDL_HJ_ORIENT_* bits."""
    if isinstance(o, (str, type(None))):
        if o not in _ORIENT_NAMES:
            raise ValueError(f"{_ORIENT_WHAT}, not {o!r}")
        return _ORIENT_NAMES[o]
    if isinstance(o, bool) or not isinstance(o, int) or not 0 <= o <= 7:
        raise ValueError(f"{_ORIENT_WHAT}, not {o!r}")
    return int(o)


def exif_code(exif: int) -> int:
    """The orientation code of EXIF orientation ``1..8``."""
    if isinstance(exif, bool) or not isinstance(exif, int) or exif not in _EXIF_CODES:
        raise ValueError(f"an EXIF orientation is 1..8, not {exif!r}")
    return _EXIF_CODES[exif]


def _view_rect(r) -> Rect:
    """A view's rectangle: as :func:`_rect`, and checked -- four numbers."""
    if r is None:
        return Rect(0, 0, 0, 0)
    try:
        ok = len(r) == 4
    except TypeError:
        ok = False
    if not ok:
        raise ValueError(f"a view's rect is (x, y, w, h) or None, not {r!r}")
    return _rect(r)


class OutputSpec(ctypes.Structure):
    _fields_ = [
        ("pix_fmt", ctypes.c_int32),
        ("dtype", ctypes.c_int32),
        ("idct", ctypes.c_int32),
        ("resize", ctypes.c_int32),
        ("fit_w", ctypes.c_int32),
        ("fit_h", ctypes.c_int32),
        ("aspect", ctypes.c_int32),
        ("pad_w", ctypes.c_int32),
        ("pad_h", ctypes.c_int32),
        ("crop_w", ctypes.c_int32),
        ("crop_h", ctypes.c_int32),
        ("filter", ctypes.c_int32),
        ("mean", ctypes.c_float * 3),
        ("std", ctypes.c_float * 3),
        ("csc", ctypes.c_int32),
    ]


@dataclass(frozen=True)
class Output:
    """What the decoder produces for every image of a batch.

    ``resize=False`` keeps the full resolution.  Otherwise the FFmpeg filter
    chain SPDL builds is applied (src/spdl/io/_preprocessing.py:214-234)::

        scale=w=fit_w:h=fit_h[:force_original_aspect_ratio=aspect]
        [,pad=w=pad_w:h=pad_h:x=-1:y=-1:color=black][,crop=w=crop_w:h=crop_h]

    Negative ``fit_w`` / ``fit_h`` have vf_scale's meaning (``-1`` keeps the
    aspect ratio, ``-n`` also makes the size divisible by n).
    ``pix_fmt="yuv"`` keeps the frame's own planar format: the chain with no
    format node (u8, ``csc="swscale"`` only; layout: :func:`planar_layout`).

    ``src_crop=(x, y, w, h)`` crops the decoder's own frame before the chain,
    for every image (libavfilter's ``crop=w:h:x:y`` ahead of ``scale``; ``x``
    or ``y`` of ``None`` is centred; include/spdl_hipjpeg.h "source crop").
    It is no field of the C output spec: the decoder passes it on through
    ``spdl_hj_set_crops``.

    ``flip`` (``0..3``, ``"h"``, ``"v"``, ``"hv"``) mirrors every image's
    output: the last node of the chain, ``...,hflip`` / ``vflip`` after scale,
    pad and crop (include/spdl_hipjpeg.h "output flips").  It travels through
    ``spdl_hj_set_flips`` as well.

    ``orient`` (``0..7`` or a spelling of :func:`_orient`) is the whole
    orientation, a transpose included (include/spdl_hipjpeg.h "output
    orientation"): the spec then describes the FINAL output, and an image with
    the transpose bit runs the chain with ``fit``, ``pad`` and ``crop`` swapped.
    It travels through ``spdl_hj_set_orients`` and excludes ``flip``.
    """

    pix_fmt: str = "rgb"
    normalize: bool = False  # -> (x/255 - mean)/std in fp32, stored as norm_dtype
    idct: str = "simple"
    resize: bool = False
    fit_w: int = 0
    fit_h: int = 0
    aspect: str | None = None
    pad_w: int = 0
    pad_h: int = 0
    crop_w: int = 0
    crop_h: int = 0
    filter: str = "bicubic"
    mean: tuple = (0.485, 0.456, 0.406)
    std: tuple = (0.229, 0.224, 0.225)
    norm_dtype: str = "float16"  # or "bfloat16"
    # "swscale": the reference CPU path's libswscale arithmetic (scale +
    # yuvj -> rgb24); "jfif": IJG libjpeg tables, nearest chroma (full-res);
    # "turbo": libjpeg-turbo's default decoder -- islow, triangle chroma
    # upsampling, 6b colour tables: Pillow's pixels (full-res; ``idct`` is not
    # consulted; include/spdl_hipjpeg.h "Pillow-exact decode")
    csc: str = "swscale"
    src_crop: tuple | None = None
    flip: int | str | None = None
    orient: int | str | None = None

    def to_c(self) -> OutputSpec:
        if self.pix_fmt not in PIX_FMTS:
            raise RuntimeError(f"Unexpected pix_fmt: {self.pix_fmt}")
        return OutputSpec(
            PIX_FMTS[self.pix_fmt],
            NORM_DTYPES[self.norm_dtype] if self.normalize else DTYPE_U8,
            IDCT[self.idct],
            int(bool(self.resize)),
            int(self.fit_w),
            int(self.fit_h),
            ASPECT[self.aspect],
            int(self.pad_w),
            int(self.pad_h),
            int(self.crop_w),
            int(self.crop_h),
            FILTERS[self.filter],
            (ctypes.c_float * 3)(*self.mean),
            (ctypes.c_float * 3)(*self.std),
            CSC[self.csc],
        )

    @property
    def planar(self) -> bool:
        return self.pix_fmt in ("rgb", "bgr")

    @property
    def torch_dtype(self):
        import torch

        if not self.normalize:
            return torch.uint8
        return torch.bfloat16 if self.norm_dtype == "bfloat16" else torch.float16


def planar_layout(ow: int, oh: int, hs: int, vs: int, gray: bool) -> tuple[tuple, int]:
    """(shape, bytes) of one ``pix_fmt="yuv"`` image of ``ow`` x ``oh`` whose
    frame has chroma ratios ``hs``, ``vs`` (include/spdl_hipjpeg.h: Y, then U,
    then V of ceil(ow / hs) x ceil(oh / vs), tightly packed), in the layout
    the reference's convert_frames gives such a frame
    (src/libspdl/core/detail/ffmpeg/conversion.cpp:196-281): ``[oh, ow, 1]``
    gray8, ``[3, oh, ow]`` yuvj444p, ``[1, 2 oh, ow]`` yuvj422p, ``[1, oh +
    oh / 2, ow]`` yuvj420p.  A 4:2:2 / 4:2:0 size that is odd on a subsampled
    axis does not fill such rows: the reference fails the copy there."""
    if gray:
        return (oh, ow, 1), ow * oh
    if (hs, vs) not in ((1, 1), (2, 1), (2, 2)):
        raise RuntimeError(f"Unsupported pixel format: chroma ratios {hs}x{vs}")
    nbytes = ow * oh + 2 * (-(-ow // hs)) * (-(-oh // vs))
    if (hs, vs) == (1, 1):
        return (3, oh, ow), nbytes
    if ow % hs or oh % vs:
        raise RuntimeError("Failed to copy image data.")
    return (1, 2 * oh if vs == 1 else oh + oh // 2, ow), nbytes


class View(ctypes.Structure):  # spdl_hj_view
    _fields_ = [("image", ctypes.c_int32), ("rect", Rect)]


class ViewGroupSpec(ctypes.Structure):  # spdl_hj_view_group
    _fields_ = [("out", OutputSpec), ("out_dev", ctypes.c_void_p), ("out_bytes", ctypes.c_size_t),
                ("views", ctypes.POINTER(View)), ("nviews", ctypes.c_int32),
                ("status", ctypes.POINTER(ctypes.c_int32))]


class ViewGroup:
    """One group of a views submission (include/spdl_hipjpeg.h "views"): the
    output chain ``out``, the views ``[(image, rect_or_None), ...]`` or
    ``[(image, rect_or_None, flip), ...]`` and the device buffer
    ``[len(views), ...]`` they are written to in view order.  A view without a
    flip of its own has ``out.flip``.  A fourth element is the view's
    orientation, ``(image, rect_or_None, None, orient)`` (``0..7``; its flip
    is then ``None``); a view without one has ``out.orient``.  A submission
    with any orientation goes through ``spdl_hj_set_orients``.
    After the consuming call, ``statuses`` holds the per-view codes (0, or the
    status of a view the host refused alone); a view is valid when its own
    status and its image's are both 0."""

    def __init__(self, out: Output, views, out_ptr: int, out_bytes: int):
        if not isinstance(out, Output):
            raise ValueError("ViewGroup(out=...) takes an Output")
        if out.src_crop is not None:
            raise ValueError("views= and Output.src_crop are exclusive")
        self.out, self.out_ptr, self.out_bytes = out, int(out_ptr), int(out_bytes)
        self.views = []
        self.flips = []  # per view, SPDL_HJ_FLIP_* bits
        self.orients = []  # per view, SPDL_HJ_ORIENT_* bits; None: no orientation of its own
        if out.flip is not None and out.orient is not None:
            raise ValueError("Output.flip and Output.orient are exclusive")
        for v in views:
            what = ("a view is (image, rect_or_None), (image, rect_or_None, flip 0..3) or "
                    f"(image, rect_or_None, None, orient 0..7), not {v!r}")
            try:
                image, rect, *rest = v
                if len(rest) > 2 or (len(rest) == 2 and rest[0] is not None):
                    raise ValueError
                orient = rest[1] if len(rest) == 2 else out.orient
                flip = _flip(rest[0] if len(rest) == 1 else None if orient is not None else out.flip)
                orient = None if orient is None else _orient(orient)
            except (TypeError, ValueError):
                raise ValueError(what) from None
            if isinstance(image, bool) or not isinstance(image, int):
                raise ValueError(what)
            self.views.append((image, _view_rect(rect)))
            self.flips.append(flip)
            self.orients.append(orient)
        n = len(self.views)
        self._views = (View * max(n, 1))(*[View(i, r) for i, r in self.views])
        self._status = (ctypes.c_int32 * max(n, 1))()

    @property
    def statuses(self) -> list[int]:
        return list(self._status)[: len(self.views)]

    def to_c(self) -> ViewGroupSpec:
        return ViewGroupSpec(self.out.to_c(), self.out_ptr, self.out_bytes, self._views,
                             len(self.views), self._status)


def _check_views(views, out: Output, crops, out_ptr, out_bytes) -> None:
    """What a views submission refuses before any library call."""
    if crops is not None:
        raise ValueError("views= and crops= are exclusive")
    if out.src_crop is not None:
        raise ValueError("views= and Output.src_crop are exclusive")
    if isinstance(views, ViewGroup) or not all(isinstance(g, ViewGroup) for g in views):
        raise ValueError("views= takes a sequence of ViewGroup")
    if out_ptr or out_bytes:
        raise ValueError("with views= the call's out_ptr and out_bytes must be 0: "
                         "every group has its own buffer")


def _has_flips(out: Output, flips, views) -> bool:
    """The submission names a flip somewhere (else no flip call is made)."""
    return flips is not None or out.flip is not None or \
        (views is not None and any(any(g.flips) for g in views))


def _has_orients(out: Output, orients, views) -> bool:
    """The submission names an orientation somewhere: it then goes through
    ``spdl_hj_set_orients``, its flips with it (codes 0..3)."""
    return orients is not None or out.orient is not None or \
        (views is not None and any(o is not None for g in views for o in g.orients))


_LIB = None
_LIB_LOCK = threading.Lock()


def lib() -> ctypes.CDLL:
    """Load the native library (raises if it has not been built)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    with _LIB_LOCK:
        if _LIB is not None:
            return _LIB
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"spdl_amd native library not found at {LIB_PATH}; "
                "build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(make -C spdl_amd/csrc)"
            )
        L = ctypes.CDLL(LIB_PATH)
        vp, sz, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int32
        cp = ctypes.c_char_p
        L.spdl_hj_abi_version.restype = ctypes.c_int
        L.spdl_hj_get_image_info.argtypes = [vp, sz, ctypes.POINTER(ImageInfo)]
        L.spdl_hj_output_size.argtypes = [
            i32, i32, ctypes.POINTER(OutputSpec), ctypes.POINTER(i32), ctypes.POINTER(i32)
        ]
        L.spdl_hj_create.argtypes = [ctypes.c_int, cp, sz]
        L.spdl_hj_create.restype = vp
        L.spdl_hj_destroy.argtypes = [vp]
        L.spdl_hj_destroy.restype = None
        L.spdl_hj_decode_batch.argtypes = [
            vp, vp, vp, i32, ctypes.POINTER(OutputSpec), vp, sz, vp, i32, vp, cp, sz
        ]
        L.spdl_hj_decode_batch_device.argtypes = [
            vp, vp, sz, vp, vp, vp, i32, ctypes.POINTER(OutputSpec), vp, sz, vp, i32, vp, cp, sz
        ]
        L.spdl_hj_decode_planes.argtypes = [vp, vp, sz, i32, vp, vp, cp, sz]
        L.spdl_hj_set_profiling.argtypes = [vp, i32]
        L.spdl_hj_last_timings.argtypes = [vp, vp, i32, ctypes.POINTER(i32)]
        L.spdl_hj_stage_name.argtypes = [i32]
        L.spdl_hj_stage_name.restype = ctypes.c_char_p
        L.spdl_hj_set_param.argtypes = [vp, cp, ctypes.c_int64]
        L.spdl_hj_get_param.argtypes = [vp, cp, ctypes.POINTER(ctypes.c_int64)]
        L.spdl_hj_debug_entropy.argtypes = [vp, vp, sz, vp, sz, vp, sz, vp, cp, sz]
        i64 = ctypes.c_int64
        L.spdl_hj_last_ticket.argtypes = [vp]
        L.spdl_hj_last_ticket.restype = i64
        L.spdl_hj_wait.argtypes = [vp, i64, vp, i32, cp, sz]
        L.spdl_hj_staging_acquire.argtypes = [
            vp, sz, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(i64), cp, sz
        ]
        L.spdl_hj_stream_wait.argtypes = [vp, i64, vp, cp, sz]
        L.spdl_hj_staging_fill.argtypes = [vp, i64, sz, vp, sz, cp, sz]
        L.spdl_hj_staging_read.argtypes = [vp, i64, sz, ctypes.c_int, i64, sz, cp, sz]
        L.spdl_hj_decode_staged.argtypes = [
            vp, i64, sz, vp, vp, i32, ctypes.POINTER(OutputSpec), vp, sz, vp, i32, vp, cp, sz
        ]
        L.spdl_hj_tar_index.argtypes = [
            vp, sz, sz, i32, vp, vp, vp, vp, sz, ctypes.POINTER(i32), ctypes.POINTER(sz)
        ]
        L.spdl_hj_nv12_to_planar_rgb.argtypes = [
            vp, i32, i32, i32, i32, i32, vp, sz, ctypes.c_int, vp, i32, cp, sz
        ]
        L.spdl_hj_copy.argtypes = [vp, vp, sz, i32, ctypes.c_int, vp, i32, cp, sz]
        if hasattr(L, "spdl_hj_set_crops"):  # (additive in ABI 7; an older A/B build has neither)
            L.spdl_hj_crop_rect.argtypes = [
                ctypes.POINTER(ImageInfo), ctypes.POINTER(Rect), ctypes.POINTER(Rect)
            ]
            L.spdl_hj_set_crops.argtypes = [vp, vp, i32]
        if hasattr(L, "spdl_hj_set_views"):  # (additive in ABI 7 as well)
            L.spdl_hj_set_views.argtypes = [vp, ctypes.POINTER(ViewGroupSpec), i32]
        if hasattr(L, "spdl_hj_set_flips"):  # (likewise)
            L.spdl_hj_set_flips.argtypes = [vp, vp, i32]
        if hasattr(L, "spdl_hj_set_orients"):  # (likewise)
            L.spdl_hj_set_orients.argtypes = [vp, vp, i32]
            L.spdl_hj_get_orientation.argtypes = [vp, ctypes.c_size_t, ctypes.POINTER(i32)]
            L.spdl_hj_orient_code.argtypes = [i32]
        if hasattr(L, "spdl_hj_set_ragged"):  # (likewise)
            L.spdl_hj_ragged_layout.argtypes = [vp, i32, ctypes.POINTER(OutputSpec), vp, vp, i64,
                                                vp, vp, vp, vp]
            L.spdl_hj_set_ragged.argtypes = [vp, vp, i32]
        if hasattr(L, "spdl_hj_set_lowres"):  # (likewise)
            L.spdl_hj_set_lowres.argtypes = [vp, vp, i32]
        ver = L.spdl_hj_abi_version()
        # (an explicitly chosen older build, ABI >= 5, loads for A/B runs)
        if ver != ABI_VERSION and not (os.environ.get("SPDL_AMD_LIB") and 5 <= ver < ABI_VERSION):
            raise RuntimeError(f"libspdl_hipjpeg ABI {ver} != expected {ABI_VERSION}")
        _LIB = L
    return _LIB


def get_image_info(data) -> ImageInfo:
    """Host SOF probe (width, height, components, sampling factors, colour model)."""
    addr, size, keep = buffer_address(data)
    info = ImageInfo()
    rc = lib().spdl_hj_get_image_info(addr, size, ctypes.byref(info))
    del keep
    if rc:
        raise RuntimeError(f"Failed to decode an image. (header probe: status {rc})")
    return info


def get_orientation(data) -> int:
    """The EXIF orientation ``1..8`` of a JPEG (spdl_hj_get_orientation; host
    only): 1 for whatever is absent or malformed -- EXIF never fails an image;
    what fails :func:`get_image_info` fails here."""
    addr, size, keep = buffer_address(data)
    exif = ctypes.c_int32(1)
    rc = lib().spdl_hj_get_orientation(addr, size, ctypes.byref(exif))
    del keep
    if rc:
        raise RuntimeError(f"Failed to decode an image. (header probe: status {rc})")
    return int(exif.value)


def crop_rect(info: ImageInfo, rect) -> tuple[int, tuple | None]:
    """``(status, (x, y, w, h))`` of the source crop ``rect`` on a frame with
    the probe ``info``, resolved as the decode calls resolve it
    (spdl_hj_crop_rect; host only).  The tuple is ``None`` when refused."""
    r, o = _rect(rect), Rect()
    rc = lib().spdl_hj_crop_rect(ctypes.byref(info), ctypes.byref(r), ctypes.byref(o))
    return int(rc), (None if rc else (o.x, o.y, o.w, o.h))


def output_size(width: int, height: int, out: Output) -> tuple[int, int]:
    ow, oh = ctypes.c_int32(), ctypes.c_int32()
    spec = out.to_c()
    rc = lib().spdl_hj_output_size(width, height, ctypes.byref(spec), ctypes.byref(ow),
                                   ctypes.byref(oh))
    if rc:
        raise RuntimeError(f"invalid output geometry for {width}x{height} ({rc})")
    return ow.value, oh.value


def lowres_size(width: int, height: int, level: int) -> tuple[int, int]:
    """The frame the decoder emits at reduced-size level ``level`` (FFmpeg's
    ``lowres``): ``ceil(width / 2^level) x ceil(height / 2^level)``."""
    return -(-width >> level), -(-height >> level)


def auto_lowres(width: int, height: int, out: Output) -> int:
    """``lowres="auto"`` for a ``width x height`` frame through ``out``: the
    largest level ``<= 3`` whose frame is, on both sides, no smaller than the
    scaled content the chain makes of the full frame (its size before pad and
    crop) -- the decode never goes below the size it scales to.  0 for a
    native-size decode."""
    if not out.resize:
        return 0
    sw, sh = output_size(width, height, replace(out, pad_w=0, pad_h=0, crop_w=0, crop_h=0))
    level = 0
    while level < 3 and all(a >= b for a, b in zip(lowres_size(width, height, level + 1), (sw, sh))):
        level += 1
    return level


def lowres_levels(lowres, infos, out: Output, orients=None) -> list[int] | None:
    """``lowres=`` as one level per image: an int ``0..3`` for every image, a
    sequence with one entry per image, or ``"auto"`` (:func:`auto_lowres` from
    each probe of ``infos``; a transposed image against the swapped chain).
    ``None`` when it asks for nothing: ``None`` itself or all zeros."""
    n = len(infos)
    if lowres is None:
        return None
    if isinstance(lowres, str) and lowres != "auto":
        raise ValueError(f'lowres= takes 0..3, a sequence of them or "auto", not {lowres!r}')

    def one(v, k):
        if v == "auto":
            i, code = infos[k], (_orient(orients[k]) if orients is not None else _orient(out.orient))
            return auto_lowres(*((i.height, i.width) if code & 4 else (i.width, i.height)), out)
        if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= 3:
            raise ValueError(f"lowres level {v!r} is not in 0..3")
        return v
    if isinstance(lowres, (str, int)):
        levels = [one(lowres, k) for k in range(n)]
    else:
        try:
            levels = list(lowres)
        except TypeError:
            raise ValueError(f"lowres level {lowres!r} is not in 0..3") from None
        if len(levels) != n:
            raise ValueError(f"{len(levels)} lowres levels for a batch of {n} images")
        levels = [one(v, k) for k, v in enumerate(levels)]
    return levels if any(levels) else None


def ragged_layout(infos, out: Output, crops=None, orients=None, align: int = 256,
                  lowres=None) -> tuple[list[int], list[tuple[int, int]], list[int]]:
    """``(offsets, sizes, statuses)`` of a ragged batch (spdl_hj_ragged_layout;
    host only): every image's final ``(ow, oh)`` resolved alone -- its source
    crop, the chain of ``out``, its orientation -- and packed at multiples of
    ``align`` bytes.  ``offsets`` has ``n + 1`` entries, the last the buffer's
    size.  An image whose crop or geometry does not resolve has its status, a
    ``(0, 0)`` size and no bytes.  ``infos``: a sequence of ImageInfo.
    ``lowres`` (:func:`lowres_levels`): the boxes are those of the reduced
    frames."""
    n = len(infos)
    levels = lowres_levels(lowres, infos, out, orients)
    if levels is not None:  # (the library sizes boxes from the probes: hand it reduced ones)
        reduced = []
        for i, lv in zip(infos, levels):
            r = ImageInfo.from_buffer_copy(i)
            r.width, r.height = lowres_size(i.width, i.height, lv)
            reduced.append(r)
        infos = reduced
    inf = infos if isinstance(infos, ctypes.Array) else (ImageInfo * max(n, 1))(*infos)
    rects = None
    if crops is not None:
        if len(crops) != n:
            raise ValueError(f"{len(crops)} crops for a batch of {n} images")
        rects = (Rect * max(n, 1))(*[_rect(r) for r in crops])
    codes = None
    if orients is not None:
        if len(orients) != n:
            raise ValueError(f"{len(orients)} orients for a batch of {n} images")
        codes = (ctypes.c_uint8 * max(n, 1))(*[_orient(o) for o in orients])
    offs = (ctypes.c_int64 * (n + 1))()
    ow, oh, st = ((ctypes.c_int32 * max(n, 1))() for _ in range(3))
    spec = out.to_c()
    rc = lib().spdl_hj_ragged_layout(inf, n, ctypes.byref(spec), rects, codes, int(align), offs,
                                     ow, oh, st)
    if rc:
        raise ValueError(f"no ragged layout for this output (pix_fmt {out.pix_fmt!r}, csc "
                         f"{out.csc!r}, align {align}): status {rc}")
    return list(offs), [(ow[i], oh[i]) for i in range(n)], list(st)[:n]


PLAN_MODES = {"yuv": 0, "gray": 1, "gbr": 2}
_PLAN_AXES = ("hl", "hc", "vl", "vc")


def debug_sws_plan(width: int, height: int, hsub: int, vsub: int, mode: str, out: Output,
                   prepass: int = -1, max_cols: int = 256) -> dict:
    """The scale / colour plan the library makes of a ``width`` x ``height``
    frame with chroma shifts ``hsub``, ``vsub`` under ``out`` (tests; needs no
    GPU): ``{"rc": code}`` plus, when the plan is accepted, the flags, the
    tiling and the four filter tables as the device gets them
    (spdl_hj_debug_sws_plan, include/spdl_hipjpeg.h).  ``mode``: "yuv", "gray"
    or "gbr"; ``out.pix_fmt == "yuv"`` selects the planar destination."""
    import numpy as np

    L = lib()
    fn = L.spdl_hj_debug_sws_plan  # bound on first use: an older A/B build has no such symbol
    if fn.argtypes is None:
        i32, vp = ctypes.c_int32, ctypes.c_void_p
        fn.argtypes = [i32] * 6 + [ctypes.POINTER(OutputSpec), i32, i32, vp, vp, vp, vp]
    spec = out.to_c()
    planar = int(out.pix_fmt == "yuv")
    info = np.zeros(40, np.int32)
    args = (int(width), int(height), int(hsub), int(vsub), PLAN_MODES[mode], planar,
            ctypes.byref(spec), int(prepass), int(max_cols), info.ctypes.data)
    rc = fn(*args, None, None, None)
    geo = dict(zip(("sw", "sh", "dx", "dy", "ow", "oh"), (int(v) for v in info[5:11])))
    if rc:
        return {"rc": int(rc), **geo}
    n = [int(v) for v in info[19:23]]
    stride = [int(v) for v in info[15:19]]
    pos = [np.zeros(n[i], np.int32) for i in range(4)]
    coef = [np.zeros((n[i], stride[i]), np.int16) for i in range(4)]
    vmode = np.zeros(0 if planar else geo["sh"], np.int32)
    pp = (ctypes.c_void_p * 4)(*[a.ctypes.data for a in pos])
    cp = (ctypes.c_void_p * 4)(*[a.ctypes.data for a in coef])
    rc = fn(*args, vmode.ctypes.data, pp, cp)
    if rc:
        raise RuntimeError(f"spdl_hj_debug_sws_plan: {rc} on the second call")
    plan = {"rc": 0, **geo}
    plan.update(zip(("special", "full", "gray", "gbr", "pre"), (int(v) for v in info[0:5])))
    plan.update(zip(("rb", "col_chunk", "bands", "chunks", "lds", "pre_rl", "pre_rc", "chr_w",
                     "chr_h"), (int(v) for v in info[23:32])))
    plan["planar"] = planar
    plan["vmode"] = vmode
    for i, a in enumerate(_PLAN_AXES):
        plan[a] = {"taps": int(info[11 + i]), "stride": stride[i], "n": n[i], "pos": pos[i],
                   "coef": coef[i]}
    return plan


def buffer_address(src) -> tuple[int, int, object]:
    """(address, length, keepalive) of a bytes-like object without copying
    when it is writable or a numpy array; read-only bytes are viewed through
    numpy (no copy either)."""
    import numpy as np

    if isinstance(src, np.ndarray):
        a = np.ascontiguousarray(src).view(np.uint8).reshape(-1)
        return a.ctypes.data, a.size, a
    a = np.frombuffer(memoryview(src).cast("B"), np.uint8)
    if a.size == 0:  # numpy gives empty arrays a dangling address
        a = np.zeros(1, np.uint8)
        return a.ctypes.data, 0, a
    return a.ctypes.data, a.size, a


def tar_index(src, start: int = 0, max_entries: int = 1 << 20, with_names: bool = True):
    """Regular-file members of an in-memory tar archive: list of (name,
    offset, size) with payload offsets into `src`, plus the resume position.
    Native walk (spdl_hj_tar_index) with the reference's semantics
    (src/spdl/io/lib/archive/tar_iterator.cpp:125-195)."""
    import numpy as np

    addr, size, keep = buffer_address(src)
    out = []
    pos = start
    while len(out) < max_entries:
        want = min(max_entries - len(out), 4096)
        offs = np.zeros(want, np.int64)
        szs = np.zeros(want, np.int64)
        noffs = np.zeros(want, np.int64)
        names = ctypes.create_string_buffer(want * 128 + 65536) if with_names else None
        n = ctypes.c_int32()
        nxt = ctypes.c_size_t()
        rc = lib().spdl_hj_tar_index(
            addr, size, pos, want, offs.ctypes.data, szs.ctypes.data,
            noffs.ctypes.data if with_names else None, names, len(names) if names else 0,
            ctypes.byref(n), ctypes.byref(nxt))
        if rc:
            raise RuntimeError(f"tar index failed ({rc})")
        raw = names.raw if with_names else b""
        for i in range(n.value):
            if with_names:
                o = int(noffs[i])
                name = raw[o: raw.index(b"\0", o)].decode("utf-8", "surrogateescape")
            else:
                name = ""
            out.append((name, int(offs[i]), int(szs[i])))
        pos = nxt.value
        if n.value == 0 or pos >= size:
            break
    del keep
    return out, pos


def _refused(views, rc: int) -> bool:
    """The call failed (``rc``) because the host refused a view alone."""
    return views is not None and any(rc == st for g in views for st in g.statuses if st)


def _stream_handle(stream) -> int | None:
    if stream is None:
        return None
    if isinstance(stream, int):
        return stream
    return int(stream.cuda_stream)


class Decoder:
    """One native context (device workspace + pinned staging) bound to a
    device.  Not thread-safe: use :func:`thread_decoder` for a per-thread one
    (the reference keeps its nvJPEG state thread_local,
    src/libspdl/cuda/nvjpeg/decoding.cpp:107-112)."""

    def __init__(self, device_index: int = 0):
        err = ctypes.create_string_buffer(512)
        h = lib().spdl_hj_create(int(device_index), err, 512)
        if not h:
            raise RuntimeError(f"spdl_amd: cannot create decoder: {err.value.decode()}")
        self._h = h
        self.device_index = int(device_index)

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().spdl_hj_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_param(self, name: str, value: int) -> None:
        rc = lib().spdl_hj_set_param(self._h, name.encode(), int(value))
        if rc:
            raise ValueError(f"invalid decoder parameter {name}={value}")

    def get_param(self, name: str) -> int:
        v = ctypes.c_int64()
        if lib().spdl_hj_get_param(self._h, name.encode(), ctypes.byref(v)):
            raise ValueError(f"unknown decoder parameter {name}")
        return int(v.value)

    def set_profiling(self, enable: bool, stages=None) -> None:
        """HIP-event timing of every stage, or only of the named ones."""
        if stages is not None:
            names = [lib().spdl_hj_stage_name(i).decode() for i in range(16)]
            self.set_param("profile_stages", sum(1 << names.index(s) for s in stages))
        elif enable:
            try:
                self.set_param("profile_stages", 0xFF)
            except ValueError:  # an A/B build from before ABI 6 times every stage anyway
                pass
        lib().spdl_hj_set_profiling(self._h, int(bool(enable)))

    def last_timings(self) -> dict:
        buf = (ctypes.c_float * 16)()
        n = ctypes.c_int32()
        lib().spdl_hj_last_timings(self._h, buf, 16, ctypes.byref(n))
        # (stages outside "profile_stages" report -1: left out)
        return {lib().spdl_hj_stage_name(i).decode(): buf[i] for i in range(n.value)
                if buf[i] >= 0.0}

    def set_crops(self, crops, n: int | None = None) -> None:
        """The source crops of the next batch submission (spdl_hj_set_crops):
        a sequence of ``(x, y, w, h)`` or ``None`` per image; ``None`` or an
        empty one clears them.  A prebuilt ``(Rect * n)`` array is passed as it
        is (no marshalling per call)."""
        if isinstance(crops, ctypes.Array):
            if lib().spdl_hj_set_crops(self._h, crops, len(crops) if n is None else n):
                raise ValueError("invalid source crops")
            return
        crops = list(crops) if crops is not None else []
        arr = (Rect * max(len(crops), 1))(*[_rect(r) for r in crops])
        if lib().spdl_hj_set_crops(self._h, arr if crops else None, len(crops) if n is None else n):
            raise ValueError("invalid source crops")

    def set_views(self, groups) -> None:
        """The views of the next batch submission (spdl_hj_set_views): a
        sequence of :class:`ViewGroup`; ``None`` or an empty one clears them.
        The groups must stay alive until the batch has been waited for (their
        status arrays are written by the consuming call)."""
        groups = list(groups) if groups is not None else []
        if not all(isinstance(g, ViewGroup) for g in groups):
            raise ValueError("set_views takes a sequence of ViewGroup")
        arr = (ViewGroupSpec * max(len(groups), 1))(*[g.to_c() for g in groups])
        self._held_views = groups  # (the library copied the view arrays; the statuses are ours)
        if lib().spdl_hj_set_views(self._h, arr if groups else None, len(groups)):
            raise ValueError("invalid views")

    def set_flips(self, flips) -> None:
        """The output flips of the next batch submission (spdl_hj_set_flips):
        a sequence of ``0..3`` / ``"h"`` / ``"v"`` / ``"hv"`` / ``None``, one
        per image, or per view with views; ``None`` or an empty one clears
        them.  ``bytes`` go to the library as they are."""
        if not isinstance(flips, (bytes, bytearray)):
            flips = bytes(_flip(f) for f in flips) if flips is not None else b""
        arr = (ctypes.c_uint8 * max(len(flips), 1))(*flips)
        if lib().spdl_hj_set_flips(self._h, arr if flips else None, len(flips)):
            raise ValueError("invalid flips")

    def _flips(self, out: Output, flips, n: int, views=None) -> None:
        """Hand the submission's flips to the context: ``flips`` per image, or
        ``out.flip`` for every image; with views, each view's own.  A
        submission without a flip makes no call."""
        if views is not None:
            if flips is not None:
                raise ValueError("with views= a flip belongs to its view: (image, rect, flip)")
            per = [f for g in views for f in g.flips]
            if any(per):
                self.set_flips(bytes(per))
            return
        if flips is not None and out.flip is not None:
            raise ValueError("flips= and Output.flip are exclusive")
        if flips is None and _flip(out.flip):
            flips = [out.flip] * n
        if flips is not None:
            if len(flips) != n:
                raise ValueError(f"{len(flips)} flips for a batch of {n} images")
            self.set_flips(flips)

    def set_orients(self, orients) -> None:
        """The output orientations of the next batch submission
        (spdl_hj_set_orients): a sequence of ``0..7`` or spellings of
        :func:`_orient`, one per image, or per view with views; ``None`` or an
        empty one clears them.  ``bytes`` go to the library as they are."""
        if not isinstance(orients, (bytes, bytearray)):
            orients = bytes(_orient(o) for o in orients) if orients is not None else b""
        arr = (ctypes.c_uint8 * max(len(orients), 1))(*orients)
        if lib().spdl_hj_set_orients(self._h, arr if orients else None, len(orients)):
            raise ValueError("invalid orientations")

    def _orients(self, out: Output, orients, n: int, views=None, flips=None) -> None:
        """Hand the submission's orientations to the context: ``orients`` per
        image, or ``out.orient`` for every image; with views, each view's own
        (a view that has only a flip goes as that flip's code)."""
        if flips is not None:
            raise ValueError("flips= and orients= are exclusive: an orientation code holds the "
                             "flip bits")
        if views is not None:
            if orients is not None:
                raise ValueError("with views= an orientation belongs to its view: "
                                 "(image, rect, None, orient)")
            self.set_orients(bytes(f if o is None else o
                                   for g in views for f, o in zip(g.flips, g.orients)))
            return
        if out.flip is not None:
            raise ValueError("Output.flip and an orientation are exclusive")
        if orients is not None and out.orient is not None:
            raise ValueError("orients= and Output.orient are exclusive")
        if orients is None:
            orients = [out.orient] * n
        if len(orients) != n:
            raise ValueError(f"{len(orients)} orients for a batch of {n} images")
        self.set_orients(orients)

    def set_lowres(self, levels) -> None:
        """The reduced-size levels of the next batch submission
        (spdl_hj_set_lowres): one ``0..3`` per image; ``None`` or an empty
        sequence clears them.  :meth:`decode_planes` consumes one level too."""
        levels = bytes(int(v) for v in levels) if levels is not None else b""
        arr = (ctypes.c_uint8 * max(len(levels), 1))(*levels)
        if lib().spdl_hj_set_lowres(self._h, arr if levels else None, len(levels)):
            raise ValueError("invalid lowres levels")

    def set_ragged(self, offsets) -> None:
        """The byte offsets of the next batch submission's images in its
        output (spdl_hj_set_ragged): that submission is a ragged one, every
        image in the layout of its own size.  ``None`` or an empty sequence
        clears them.  A prebuilt ``(c_int64 * n)`` array is passed as it is (no
        marshalling per call)."""
        if isinstance(offsets, ctypes.Array):
            if lib().spdl_hj_set_ragged(self._h, offsets, len(offsets)):
                raise ValueError("invalid ragged offsets")
            return
        offsets = [int(o) for o in offsets] if offsets is not None else []
        arr = (ctypes.c_int64 * max(len(offsets), 1))(*offsets)
        if lib().spdl_hj_set_ragged(self._h, arr if offsets else None, len(offsets)):
            raise ValueError("invalid ragged offsets")

    def _crops(self, out: Output, crops, n: int) -> None:
        """Hand the submission's rectangles to the context: ``crops`` per
        image, or ``out.src_crop`` for every image."""
        if crops is not None and out.src_crop is not None:
            raise ValueError("crops= and Output.src_crop are exclusive")
        if crops is None and out.src_crop is not None:
            crops = [out.src_crop] * n
        if crops is not None:
            if len(crops) != n:
                raise ValueError(f"{len(crops)} crops for a batch of {n} images")
            self.set_crops(crops)

    def decode_batch(self, datas, out: Output, out_ptr: int, out_bytes: int, stream=None,
                     sync: bool = True, check: bool = True, crops=None, views=None,
                     flips=None, orients=None, ragged=None, lowres=None) -> list[int]:
        """Per-image statuses.  A failed image raises RuntimeError unless
        ``check`` is False (synchronous calls), which returns the statuses.
        ``crops``: a source crop ``(x, y, w, h)`` or ``None`` per image.
        ``views``: a sequence of :class:`ViewGroup` -- several outputs per
        image from one decode; ``out_ptr`` and ``out_bytes`` must then be 0 and
        of ``out`` only ``idct`` is used.  The per-view statuses are each
        group's ``statuses``; with ``check=False`` a refused view does not
        raise either.  ``flips``: an output flip (``0..3``, ``"h"``, ``"v"``,
        ``"hv"`` or ``None``) per image; with views, each view carries its own.
        ``orients``: an orientation (``0..7`` or a spelling of :func:`_orient`)
        per image instead of ``flips`` (spdl_hj_set_orients).  ``ragged``:
        one byte offset per image (the first ``n`` of :func:`ragged_layout`'s)
        -- every image its own size, written at its offset of ``out_ptr``
        (include/spdl_hipjpeg.h "ragged batches").  ``lowres``: a reduced-size
        level ``0..3`` per image (spdl_hj_set_lowres; resolve ``"auto"`` or a
        single int with :func:`lowres_levels` first)."""
        n = len(datas)
        if n == 0:
            raise RuntimeError("Failed to decode an image. (the batch is empty)")
        status = (ctypes.c_int32 * n)()

        def call(err):
            # borrowed for the duration of the call, no copy (the reference binds
            # memoryviews as string_views, src/spdl/io/lib/cuda/memoryview_utils.h:17-20)
            keep = []
            ptrs = (ctypes.c_void_p * n)()
            sizes = (ctypes.c_size_t * n)()
            for i, d in enumerate(datas):
                addr, size, k = buffer_address(d)
                keep.append(k)
                ptrs[i] = addr
                sizes[i] = size
            spec = out.to_c()
            return lib().spdl_hj_decode_batch(
                self._h, ptrs, sizes, n, ctypes.byref(spec), out_ptr, out_bytes,
                _stream_handle(stream), int(bool(sync)), status, err, 1024,
            )
        return list(Decoder._submit(self, n, out, out_ptr, out_bytes, crops, views, flips, sync,
                                    check, status, call, orients, ragged, lowres))

    def _submit(self, n, out, out_ptr, out_bytes, crops, views, flips, sync, check, status,
                call, orients=None, ragged=None, lowres=None):
        """What the three batch submissions share: the views, crops and flips
        (or orientations) go to the context, ``call(err)`` -- the method's own marshalling and
        its native call -- returns the library's code, and a failure raises
        unless ``check`` is False on a synchronous call that refused an image
        (``status``) or a view.  (The methods reach it through the class: they
        also run unbound, on objects that are no Decoder.)"""
        if views is not None:
            _check_views(views, out, crops, out_ptr, out_bytes)
            self.set_views(views)
        else:
            self._crops(out, crops, n)
        if _has_orients(out, orients, views):
            Decoder._orients(self, out, orients, n, views, flips)
        elif _has_flips(out, flips, views):
            self._flips(out, flips, n, views)
        if ragged is not None:  # (its count is the consuming call's to check)
            Decoder.set_ragged(self, ragged)
        if lowres is not None:  # (count and values likewise)
            Decoder.set_lowres(self, lowres)
        err = ctypes.create_string_buffer(1024)
        rc = call(err)
        if rc and not (not check and sync and (any(status) or _refused(views, rc))):
            raise RuntimeError(err.value.decode() or f"Failed to decode an image. ({rc})")
        return status

    def decode_batch_device(self, dev_ptr: int, dev_bytes: int, offsets, sizes, infos,
                            out: Output, out_ptr: int, out_bytes: int, stream=None,
                            sync: bool = True, crops=None, check: bool = True,
                            views=None, flips=None, orients=None, ragged=None,
                            lowres=None) -> list[int]:
        """``offsets``/``sizes``: sequences or int64 numpy arrays; ``infos``: a
        sequence of ImageInfo or a prebuilt ``(ImageInfo * n)`` array (pass the
        same objects again to skip re-marshalling on every call)."""
        import numpy as np

        n = len(offsets)
        status = np.zeros(n, np.int32)

        def call(err):
            offs = np.ascontiguousarray(offsets, dtype=np.int64)
            szs = np.ascontiguousarray(sizes, dtype=np.int64)
            inf = infos if isinstance(infos, ctypes.Array) else (ImageInfo * n)(*infos)
            spec = self._spec(out)
            return lib().spdl_hj_decode_batch_device(
                self._h, dev_ptr, dev_bytes, offs.ctypes.data, szs.ctypes.data, inf, n,
                ctypes.byref(spec), out_ptr, out_bytes, _stream_handle(stream), int(bool(sync)),
                status.ctypes.data, err, 1024,
            )
        return Decoder._submit(self, n, out, out_ptr, out_bytes, crops, views, flips, sync,
                               check, status, call, orients, ragged, lowres).tolist()

    def _spec(self, out: Output) -> OutputSpec:
        cache = self.__dict__.setdefault("_spec_cache", {})
        spec = cache.get(out)
        if spec is None:
            spec = cache[out] = out.to_c()
        return spec

    # ---- asynchronous submission / staging ring (include/spdl_hipjpeg.h) ----
    def last_ticket(self) -> int:
        return int(lib().spdl_hj_last_ticket(self._h))

    def wait(self, ticket: int, n: int = 0) -> list[int]:
        import numpy as np

        status = np.zeros(max(n, 1), np.int32)
        err = ctypes.create_string_buffer(1024)
        rc = lib().spdl_hj_wait(self._h, int(ticket), status.ctypes.data if n else None, n, err,
                                1024)
        if rc:
            raise RuntimeError(err.value.decode() or f"Failed to decode an image. ({rc})")
        return status[:n].tolist()

    def stream_wait(self, ticket: int, stream) -> None:
        """Make `stream` wait on the device for batch `ticket`."""
        err = ctypes.create_string_buffer(512)
        rc = lib().spdl_hj_stream_wait(self._h, int(ticket), _stream_handle(stream), err, 512)
        if rc:
            raise RuntimeError(err.value.decode())

    def staging_acquire(self, nbytes: int) -> tuple[int, int]:
        """(pinned host address, ticket) of the next ring slot (>= nbytes)."""
        ptr = ctypes.c_void_p()
        ticket = ctypes.c_int64()
        err = ctypes.create_string_buffer(1024)
        rc = lib().spdl_hj_staging_acquire(self._h, int(nbytes), ctypes.byref(ptr),
                                           ctypes.byref(ticket), err, 1024)
        if rc:
            raise RuntimeError(err.value.decode())
        return int(ptr.value), int(ticket.value)

    def staging_fill(self, ticket: int, dst_off: int, src_addr: int, nbytes: int) -> None:
        err = ctypes.create_string_buffer(512)
        rc = lib().spdl_hj_staging_fill(self._h, int(ticket), int(dst_off), src_addr, int(nbytes),
                                        err, 512)
        if rc:
            raise RuntimeError(err.value.decode())

    def staging_read(self, ticket: int, dst_off: int, fd: int, file_off: int,
                     nbytes: int) -> None:
        err = ctypes.create_string_buffer(512)
        rc = lib().spdl_hj_staging_read(self._h, int(ticket), int(dst_off), int(fd),
                                        int(file_off), int(nbytes), err, 512)
        if rc:
            raise RuntimeError(err.value.decode())

    def decode_staged(self, ticket: int, nbytes: int, offsets, sizes, out: Output, out_ptr: int,
                      out_bytes: int, stream=None, sync: bool = True, crops=None,
                      check: bool = True, views=None, flips=None, orients=None,
                      ragged=None, lowres=None) -> list[int]:
        n = len(offsets)
        status = (ctypes.c_int32 * max(n, 1))()

        def call(err):
            offs = (ctypes.c_int64 * n)(*offsets)
            szs = (ctypes.c_int64 * n)(*sizes)
            spec = out.to_c()
            return lib().spdl_hj_decode_staged(
                self._h, int(ticket), int(nbytes), offs, szs, n, ctypes.byref(spec), out_ptr,
                out_bytes, _stream_handle(stream), int(bool(sync)), status, err, 1024)
        return list(Decoder._submit(self, n, out, out_ptr, out_bytes, crops, views, flips, sync,
                                    check, status, call, orients, ragged, lowres))[:n]

    def debug_entropy(self, data, nblocks: int):
        """Coefficients / destuffed bytes / diagnostics of one image (tests)."""
        import numpy as np

        addr, size, keep = buffer_address(data)
        coefs = np.zeros((nblocks, 64), np.int16)
        clean = np.zeros(size, np.uint8)
        diag = np.zeros(60, np.int32)
        err = ctypes.create_string_buffer(1024)
        rc = lib().spdl_hj_debug_entropy(self._h, addr, size, coefs.ctypes.data,
                                         coefs.size, clean.ctypes.data, clean.size,
                                         diag.ctypes.data, err, 1024)
        if rc:
            raise RuntimeError(err.value.decode())
        return coefs, clean[: max(int(diag[1]), 0)], {
            "status": int(diag[0]), "clean_len": int(diag[1]), "nseg": int(diag[2]),
            "sync_rounds": int(diag[3]),
            "phase_us": [round(int(x) / 100.0, 1) for x in diag[4:8]],
            "dbg": [int(x) for x in diag[8:12]],
            "scans": [tuple(int(x) for x in diag[12 + 3 * s:15 + 3 * s]) for s in range(16)]}

    def decode_planes(self, data, idct: str = "simple", stream=None, lowres: int = 0):
        """The decoder's own planes; ``lowres`` 1..3: the reduced planes, at the
        reduced frame's component sizes."""
        import numpy as np

        info = get_image_info(data)
        fw, fh = lowres_size(info.width, info.height, lowres if 0 <= lowres <= 3 else 0)
        hmax = max(info.h_samp[c] for c in range(info.ncomp))
        vmax = max(info.v_samp[c] for c in range(info.ncomp))
        planes = []
        for c in range(info.ncomp):
            if info.ncomp == 1:
                w, h = fw, fh
            else:
                w = -(-fw * info.h_samp[c] // hmax)
                h = -(-fh * info.v_samp[c] // vmax)
            planes.append(np.zeros((h, w), np.uint8))
        ptrs = (ctypes.c_void_p * 4)(*([p.ctypes.data for p in planes] + [None] * (4 - len(planes))))
        addr, size, keep = buffer_address(data)
        err = ctypes.create_string_buffer(1024)
        if lowres:
            Decoder.set_lowres(self, [lowres])
        rc = lib().spdl_hj_decode_planes(self._h, addr, size, IDCT[idct],
                                         ptrs, _stream_handle(stream), err, 1024)
        if rc:
            raise RuntimeError(err.value.decode())
        return planes


_TLS = threading.local()


def thread_decoder(device_index: int) -> Decoder:
    """The calling thread's decoder for `device_index` (created on first use)."""
    d = getattr(_TLS, "decoders", None)
    if d is None:
        d = _TLS.decoders = {}
    dec = d.get(device_index)
    if dec is None:
        dec = d[device_index] = Decoder(device_index)
    return dec
