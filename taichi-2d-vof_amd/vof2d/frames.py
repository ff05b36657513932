"""vof_frame / vof_step_frames (include/vof2d.h): the names of the quantities and of the summary's slots, the block size of a
picture of a given longest side, colour tables sampled from matplotlib's maps, and a PNG writer on zlib + struct alone, so
that writing frames needs no matplotlib."""
import struct
import zlib

import numpy as np

from . import _abi

QUANTITIES = {"F": _abi.VOF_FRAME_F, "U": _abi.VOF_FRAME_U, "V": _abi.VOF_FRAME_V, "SPEED": _abi.VOF_FRAME_SPEED, "P": _abi.VOF_FRAME_P,
              "VORT": _abi.VOF_FRAME_VORT, "DYE": _abi.VOF_FRAME_DYE}
SIGNED = ("U", "V", "VORT")   # drawn over a range symmetric about zero unless one is given
DEFAULT_CMAP = {"F": "Blues", "DYE": "Blues", "U": "coolwarm", "V": "coolwarm", "VORT": "coolwarm", "SPEED": "plasma", "P": "plasma"}
SUMMARY = ("PW", "PH", "ISTEP", "LO", "HI", "NAN_PIXELS", "CONTOUR_PIXELS")
_INTEGER = ("PW", "PH", "ISTEP", "NAN_PIXELS", "CONTOUR_PIXELS")


def summary_of(row):
    """The VOF_FRAME_SUM_N doubles of a summary as a dict keyed by SUMMARY (the counts as ints)."""
    return {k: (int(row[i]) if k in _INTEGER else float(row[i])) for i, k in enumerate(SUMMARY)}


def quantity_code(quantity):
    if isinstance(quantity, str):
        return QUANTITIES[quantity.upper()]
    return int(quantity)


def spec(quantity="F", bx=1, by=None, lo=0.0, hi=0.0, contour=False, symmetric=False):
    """A vof2d_frame_spec; lo == hi asks for the range of the picture."""
    s = _abi.FrameSpec()
    s.quantity = quantity_code(quantity)
    s.bx, s.by = int(bx), int(bx if by is None else by)
    s.flags = (_abi.VOF_FRAME_CONTOUR if contour else 0) | (_abi.VOF_FRAME_SYMMETRIC if symmetric else 0)
    s.lo, s.hi = float(lo), float(hi)
    return s


def shape(nx, ny, bx, by):
    """(pw, ph) of a picture of an nx x ny grid with bx x by cells per pixel."""
    return -(-int(nx) // int(bx)), -(-int(ny) // int(by))


def default_block(nx, ny, longest=1024):
    """The smallest square block with which the picture's longer side has at most `longest` pixels."""
    return max(1, -(-max(int(nx), int(ny)) // int(longest)))


def default_lut():
    """The table a handle starts with: the grey ramp, a black contour, magenta for NaN."""
    t = np.empty((_abi.VOF_FRAME_LUT_ROWS, 3), dtype=np.uint8)
    t[:256] = np.arange(256, dtype=np.uint8)[:, None]
    t[256], t[257] = (0, 0, 0), (255, 0, 255)
    return t


def lut(cmap_name, contour=(0, 0, 0), nan=(255, 0, 255)):
    """258 x 3 uint8: matplotlib's map cmap_name sampled at k / 255, k = 0 .. 255, each channel x to (int)(x * 255 + 0.5); the
    contour colour; the NaN colour."""
    import matplotlib
    cmap = matplotlib.colormaps[cmap_name] if hasattr(matplotlib, "colormaps") else matplotlib.cm.get_cmap(cmap_name)
    rgba = np.asarray(cmap(np.arange(256) / 255.0), dtype=np.float64)
    t = np.empty((_abi.VOF_FRAME_LUT_ROWS, 3), dtype=np.uint8)
    t[:256] = (rgba[:, :3] * 255.0 + 0.5).astype(np.int64).astype(np.uint8)
    t[256], t[257] = contour, nan
    return t


def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)


def write_png(path, rgb, level=6):
    """An 8-bit RGB PNG of the (height, width, 3) uint8 array rgb: filter 0 on every row, one IDAT chunk."""
    a = np.ascontiguousarray(rgb, dtype=np.uint8)
    if a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("write_png: expected a (height, width, 3) array, got %s" % (a.shape,))
    h, w = a.shape[:2]
    rows = np.empty((h, 1 + 3 * w), dtype=np.uint8)
    rows[:, 0] = 0
    rows[:, 1:] = a.reshape(h, 3 * w)
    png = (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + _chunk(b"IDAT", zlib.compress(rows.tobytes(), level)) +
           _chunk(b"IEND", b""))
    with open(path, "wb") as f:
        f.write(png)
