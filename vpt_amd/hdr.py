"""Radiance .hdr (RGBE) reader — environment maps for MCS / MCM (no reference counterpart: RenderingContext.js:95 leaves HDRI as a TODO).

``read_hdr(bytes or path)`` returns an ``HDRImage``: the file's RGBE bytes [height][width][4] (r, g, b, shared exponent), undecoded.
``setEnvironmentMap`` uploads them as VPT_ENV_RGBE8 and the device decodes them (include/vpt.h), so there is one decoder.

What is read:
  * the magic line ``#?RADIANCE`` or ``#?RGBE``; header lines up to the blank line.  ``FORMAT=32-bit_rle_rgbe`` is required when a FORMAT
    line is present (``32-bit_rle_xyze`` raises).  Every other line (EXPOSURE, PRIMARIES, comments, ...) is ignored: EXPOSURE is NOT applied.
  * the resolution line ``-Y H +X W`` (rows top to bottom, columns left to right); any other orientation raises.
  * scanlines in the new run-length form (``2 2 hi lo`` with ``hi << 8 | lo == W``, then the four channel planes: a count byte > 128 is a
    run of ``count - 128`` copies of the next byte, 1 .. 128 that many literal bytes) or flat (W raw RGBE pixels; the only form allowed when
    W < 8 or W > 32767).  Old-style run-length pixels (1, 1, 1, n), a zero count and truncated data raise.
Row 0 of the result is the file's first scanline, the image's top: the row an RGBA8 image puts first (the reference uploads an <img> without
UNPACK_FLIP_Y).  js/vpt/hdr.js is the same reader for the Node host; both return the same bytes."""
import os
import re

import numpy as np

_RESOLUTION = re.compile(rb"^-Y (\d+) \+X (\d+)$")


class HDRImage:
    """RGBE bytes [height][width][4] as read (format 'rgbe': VPT_ENV_RGBE8)"""
    format = 'rgbe'

    def __init__(self, data, width, height):
        self.data, self.width, self.height = data, int(width), int(height)

    @property
    def shape(self):
        return self.data.shape


def _line(buf, pos):
    end = buf.find(b"\n", pos)
    if end < 0:
        raise ValueError("HDR: truncated header")
    return buf[pos:end], end + 1


def _rle_scanline(buf, pos, width, row):
    n = len(buf)
    for c in range(4):
        x = 0
        while x < width:
            if pos >= n:
                raise ValueError("HDR: truncated scanline data")
            count = buf[pos]; pos += 1
            if count > 128:
                count -= 128
                if x + count > width:
                    raise ValueError("HDR: run overruns the scanline")
                if pos >= n:
                    raise ValueError("HDR: truncated scanline data")
                row[x:x + count, c] = buf[pos]; pos += 1
            elif count == 0:
                raise ValueError("HDR: zero run count in a scanline")
            else:
                if x + count > width:
                    raise ValueError("HDR: run overruns the scanline")
                if pos + count > n:
                    raise ValueError("HDR: truncated scanline data")
                row[x:x + count, c] = np.frombuffer(buf, np.uint8, count, pos); pos += count
            x += count
    return pos


def read_hdr(src):
    """src: bytes-like, or a path.  Returns an HDRImage; raises ValueError on anything it does not read."""
    if isinstance(src, (str, os.PathLike)):
        with open(src, "rb") as f:
            buf = f.read()
    else:
        buf = bytes(src)
    magic, pos = _line(buf, 0)
    if magic not in (b"#?RADIANCE", b"#?RGBE"):
        raise ValueError("HDR: not a Radiance file (no #?RADIANCE / #?RGBE line)")
    while True:
        line, pos = _line(buf, pos)
        if not line:
            break
        if line.startswith(b"FORMAT=") and line != b"FORMAT=32-bit_rle_rgbe":
            raise ValueError("HDR: unsupported format %r (only 32-bit_rle_rgbe)" % line[7:].decode("latin-1"))
    res, pos = _line(buf, pos)
    m = _RESOLUTION.match(res)
    if not m:
        raise ValueError("HDR: unsupported resolution line %r (only -Y H +X W)" % res.decode("latin-1"))
    height, width = int(m.group(1)), int(m.group(2))
    if width < 1 or height < 1:
        raise ValueError("HDR: empty image %dx%d" % (width, height))
    out = np.empty((height, width, 4), np.uint8)
    n = len(buf)
    for y in range(height):
        if 8 <= width <= 32767 and pos + 4 <= n and buf[pos] == 2 and buf[pos + 1] == 2 and buf[pos + 2] < 128:
            w = (buf[pos + 2] << 8) | buf[pos + 3]
            if w != width:
                raise ValueError("HDR: scanline %d has width %d, the image %d" % (y, w, width))
            pos = _rle_scanline(buf, pos + 4, width, out[y])
            continue
        if pos + 4 * width > n:
            raise ValueError("HDR: truncated scanline data")
        row = np.frombuffer(buf, np.uint8, 4 * width, pos).reshape(width, 4)
        if ((row[:, 0] == 1) & (row[:, 1] == 1) & (row[:, 2] == 1)).any():
            raise ValueError("HDR: old-style run-length scanlines (1 1 1 n) are not supported")
        out[y] = row
        pos += 4 * width
    return HDRImage(out, width, height)

