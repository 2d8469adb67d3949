"""FFmpeg filter-description helpers for the image path.

``get_video_filter_desc`` reproduces the string the reference builds
(src/spdl/io/_preprocessing.py:122-254, image-relevant arguments), and
``parse_image_filter`` turns such a string back into the decoder's output
spec, so callers that pass ``filter_desc=`` strings keep working.  Only the
filters the image path needs are understood: ``scale`` (w, h, flags,
force_original_aspect_ratio), ``pad`` (w, h, x=-1, y=-1, color=black),
``crop`` (w, h, centred; with x and / or y ahead of ``scale``: a source crop
of the decoder's frame, integers only) and ``format=pix_fmts=``.  Anything
else raises.
"""

from __future__ import annotations

from .._lib import Output

_FILTERS = {"bicubic": "bicubic", "bilinear": "bilinear", "lanczos": "lanczos"}
# swscale's SWS_FAST_BILINEAR is its own horizontal scaler (7-bit position
# fractions), not the bilinear filter: rather than silently return other
# pixels, it is refused
_NOT_IMPLEMENTED = {"fast_bilinear": "swscale's fast_bilinear scaler is not implemented; "
                                     "use flags=bilinear (a different, exact bilinear filter)"}


# scale_mode -> scale's force_original_aspect_ratio and the filter that
# brings the fitted image to the requested box
_FIT = {None: (None, None), "pad": ("decrease", "pad"), "crop": ("increase", "crop")}


def _node(name: str, **opts) -> str:
    """One filter of an FFmpeg chain: ``name=k1=v1:k2=v2``."""
    return name + "=" + ":".join(f"{k}={v}" for k, v in opts.items())


def get_video_filter_desc(
    *,
    scale_width: int | None = None,
    scale_height: int | None = None,
    scale_algo: str = "bicubic",
    scale_mode: str | None = "pad",
    crop_width: int | None = None,
    crop_height: int | None = None,
    pix_fmt: str | None = "rgb24",
    pad_mode: str | None = None,
    filter_desc: str | None = None,
    **unsupported: object,
) -> str | None:
    """The filter chain the reference builds for these image arguments
    (src/spdl/io/_preprocessing.py:122-254; byte-for-byte, pinned by
    tests/golden/filter_desc.json): optional scale (+ pad / crop to the box),
    optional centre crop, a caller chain, then the output pixel format."""
    extra = sorted(k for k, v in unsupported.items() if v is not None)
    if extra:
        raise ValueError(f"image filter arguments not supported here: {extra}")
    if scale_mode not in _FIT:
        raise ValueError(f"scale_mode must be 'pad', 'crop' or None, got {scale_mode!r}")
    chain: list[str] = []
    if (scale_width, scale_height) != (None, None):
        box = {"w": scale_width or 0, "h": scale_height or 0}
        ratio, follow = _FIT[scale_mode]
        scale = {**box, "flags": scale_algo}
        if ratio:
            scale["force_original_aspect_ratio"] = ratio
        chain.append(_node("scale", **scale))
        if follow == "pad":
            chain.append(_node("pad", **box, x=-1, y=-1, color=pad_mode or "black"))
        elif follow == "crop":
            chain.append(_node("crop", **box))
    if (crop_width, crop_height) != (None, None):
        chain.append(_node("crop", w=crop_width or 0, h=crop_height or 0))
    if filter_desc is not None:
        chain.append(filter_desc)
    if pix_fmt is not None:
        chain.append(_node("format", pix_fmts=pix_fmt))
    return ",".join(chain) or None


def _kv(args: str) -> dict:
    out = {}
    for i, item in enumerate(a for a in args.split(":") if a):
        if "=" in item:
            k, v = item.split("=", 1)
        else:  # positional w:h
            k, v = ("w", "h", "x", "y", "keep_aspect", "exact")[min(i, 5)], item
        out[k.strip()] = v.strip()
    return out


def _size(kv: dict, key: str, part: str, required: bool = False) -> int:
    v = int(kv[key] if required else kv.get(key, 0))
    if v < 0:
        raise ValueError(f"negative {key} is not valid here: {part}")
    return v


_TRANSPOSE_DIRS = {"0": 4, "cclock_flip": 4, "1": 5, "clock": 5, "2": 6, "cclock": 6,
                   "3": 7, "clock_flip": 7}  # -> orientation code (include/spdl_hipjpeg.h)


def _oriented(code: int, img):
    """Rows ``img`` under orientation ``code``: the transpose, then the flips."""
    if code & 4:
        img = [list(r) for r in zip(*img)]
    if code & 1:
        img = [r[::-1] for r in img]
    if code & 2:
        img = img[::-1]
    return [list(r) for r in img]


def _then(code: int, node: int) -> int:
    """The one code of orientation ``code`` followed by orientation ``node``:
    the eight orientations form a group, and instead of its multiplication
    table both are applied to a 3 x 2 image of distinct labels, on which the
    eight codes give eight different results -- the one that matches names the
    product."""
    base = [[0, 1, 2], [3, 4, 5]]
    want = _oriented(node, _oriented(code, base))
    return next(k for k in range(8) if _oriented(k, base) == want)


def parse_image_filter(filter_desc: str | None, default_pix_fmt: str | None = "rgb24") -> Output:
    """Translate an image filter chain into an :class:`Output` spec.

    ``default_pix_fmt=None``: a chain without a ``format`` node keeps the
    decoder's own planar format (``pix_fmt="yuv"``), as libavfilter does.

    ``hflip`` / ``vflip`` are taken as the chain's last geometry nodes: after
    ``scale`` and after the last ``pad`` / ``crop``, before or after ``format``
    (``Output.flip``; repeated nodes toggle).  Anywhere else their pixels would
    differ from the store-time flip, and they are refused.

    ``transpose=dir`` (``0..3`` or ``cclock_flip`` / ``clock`` / ``cclock`` /
    ``clock_flip``) is taken in the same places and composes with the flips in
    chain order.  A chain whose orientation holds a transpose gives
    ``Output.orient`` and the FINAL-output form of the spec: the ``scale``,
    ``pad`` and ``crop`` sizes parsed ahead of it with each pair swapped."""
    spec = dict(pix_fmt=default_pix_fmt or "yuv", resize=False)
    if not filter_desc:
        return Output(**spec)
    have_scale = have_pad = False
    flip = 0  # the orientation code of the flips and transposes so far
    oriented = False  # a transpose node was among them
    for part in filter_desc.split(","):
        part = part.strip()
        if not part:
            continue
        name, _, args = part.partition("=")
        kv = _kv(args)
        if name == "transpose":
            # transpose=dir=clock, or positional: transpose=clock (its own parse: _kv names
            # positional arguments after scale's w:h)
            items = [a for a in args.split(":") if a]
            kv = dict(a.split("=", 1) if "=" in a else ("dir", a) for a in items[:1])
            kv.update(a.split("=", 1) if "=" in a else ("passthrough", a) for a in items[1:])
            extra = sorted(set(kv) - {"dir"})
            if extra:  # passthrough=portrait / landscape skips the node by the frame's shape
                raise ValueError(f"transpose options not supported: {extra} (a transpose that "
                                 f"depends on the frame's shape cannot be planned ahead): {part}")
            d = kv.get("dir", "0")
            if d not in _TRANSPOSE_DIRS:
                raise ValueError(f"transpose takes dir=0..3, cclock_flip, clock, cclock or "
                                 f"clock_flip: {part}")
            if not have_scale:
                raise ValueError(
                    "transpose ahead of scale is not supported: the pixels would differ from a "
                    "transpose of the scaled image (swscale's horizontal and vertical passes "
                    "round differently); put it after scale, pad and crop, or pass orients= for "
                    "a full-resolution decode")
            flip = _then(flip, _TRANSPOSE_DIRS[d])
            oriented = True
            continue
        if name in ("hflip", "vflip"):
            if args:
                raise ValueError(f"{name} takes no options: {part}")
            if not have_scale:
                raise ValueError(
                    f"{name} ahead of scale is not supported: the pixels would differ from a flip "
                    "of the scaled image (swscale's filter positions are not mirror-symmetric and "
                    "odd-width chroma pairs differently); put it after scale, pad and crop, or "
                    "pass flips= for a full-resolution decode")
            flip = _then(flip, 1 if name == "hflip" else 2)
            continue
        if oriented and name in ("scale", "pad", "crop"):
            raise ValueError(
                f"transpose ahead of {name} is not supported: the pixels would differ from a "
                "transpose of the final image (a later scale rounds its two passes differently, "
                "and a centred pad or crop is placed by the sizes it sees); put the transpose "
                "after the last scale, pad and crop")
        if flip and name in ("scale", "pad", "crop"):
            raise ValueError(
                f"hflip / vflip ahead of {name} is not supported: the pixels would differ from a "
                "flip of the final image (the filter positions of a later scale, and the odd "
                "remainder of a centred pad or crop, are not mirror-symmetric); put the flip "
                "after the last scale, pad and crop")
        if name == "scale":
            # (negative sizes: vf_scale's -1 / -n, resolved by the library)
            w, h = int(kv.get("w", 0)), int(kv.get("h", 0))
            spec.update(resize=True, fit_w=w, fit_h=h)
            flags = kv.get("flags", "bicubic")
            if flags in _NOT_IMPLEMENTED:
                raise ValueError(_NOT_IMPLEMENTED[flags])
            if flags not in _FILTERS:
                raise ValueError(f"unsupported scale flags: {flags}")
            spec["filter"] = _FILTERS[flags]
            ar = kv.get("force_original_aspect_ratio")
            if ar in (None, "disable", "0"):
                spec["aspect"] = None
            elif ar in ("decrease", "1"):
                spec["aspect"] = "decrease"
            elif ar in ("increase", "2"):
                spec["aspect"] = "increase"
            else:
                raise ValueError(f"unsupported force_original_aspect_ratio: {ar}")
            have_scale = True
        elif name == "pad":
            if not have_scale:
                raise ValueError("pad without a preceding scale is not supported")
            if kv.get("x", "-1") != "-1" or kv.get("y", "-1") != "-1":
                raise ValueError("only centred pad (x=-1:y=-1) is supported")
            if kv.get("color", "black") != "black":
                raise ValueError("only color=black is supported")
            spec.update(resize=True, pad_w=_size(kv, "w", part, True), pad_h=_size(kv, "h", part, True))
            have_pad = True
        elif name == "crop" and ("x" in kv or "y" in kv) and not have_scale and not have_pad:
            # a crop with a position ahead of scale / pad: a source crop, taken
            # from the decoder's frame (include/spdl_hipjpeg.h); a missing x or
            # y is centred, as in vf_crop
            if "src_crop" in spec:
                raise ValueError(f"more than one source crop: {part}")
            extra = sorted(set(kv) - {"w", "h", "x", "y"})
            if extra:  # exact=1, keep_aspect, out_w ...
                raise ValueError(f"crop options not supported in a source crop: {extra}")
            try:
                w, h = int(kv["w"]), int(kv["h"])
                x, y = (int(kv[k]) if k in kv else None for k in ("x", "y"))
            except (KeyError, ValueError):
                raise ValueError("a source crop takes integer w, h and x / y (no expressions): "
                                 f"{part}") from None
            spec["src_crop"] = (x, y, w, h)
        elif name == "crop":
            if "x" in kv or "y" in kv:
                raise ValueError("only centred crop is supported")
            spec.update(resize=True, crop_w=_size(kv, "w", part), crop_h=_size(kv, "h", part))
        elif name == "format":
            pf = kv.get("pix_fmts", kv.get("w"))
            if pf not in ("rgb24", "bgr24", "rgb", "bgr"):
                raise ValueError(f"unsupported output pix_fmt: {pf}")
            spec["pix_fmt"] = pf
        else:
            raise ValueError(f"filter `{name}` is not supported by the image decode stage")
    if flip & 4:
        if spec["pix_fmt"] == "yuv":
            raise ValueError("transpose of the decoder's planar format is not supported (a "
                             "transposed 4:2:2 frame is another pixel format); name an RGB pix_fmt")
        # the spec describes the final output: the pairs parsed ahead of the transpose, swapped
        for a, b in (("fit_w", "fit_h"), ("pad_w", "pad_h"), ("crop_w", "crop_h")):
            if a in spec or b in spec:
                spec[a], spec[b] = spec.get(b, 0), spec.get(a, 0)
        spec["orient"] = flip
    elif flip:
        spec["flip"] = flip
    return Output(**spec)
