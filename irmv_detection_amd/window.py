"""Host reference of the tracking window (irmv_engine_cfg.win_width / win_height, include/irmv_hip.h).

A window engine runs every step on a w x h crop of the frame the producer writes.  The window's corner (x0, y0) is given in
the coordinates detections come back in: the 180-degree rotated frame when rotate180 is set, because that is the frame a
tracker sees.  `crop` cuts the same bytes window_crop_kernel copies; `window_map` is irmv_window_map in numpy."""
from __future__ import annotations

import numpy as np


def buffer_origin(full_size, x0, y0, w, h, rotate180=True):
    """The window's top-left corner in buffer coordinates (the frame as the producer writes it)."""
    fw, fh = int(full_size[0]), int(full_size[1])
    if not (0 <= x0 <= fw - w and 0 <= y0 <= fh - h):
        raise ValueError(f"window {w} x {h} at ({x0}, {y0}) does not lie inside the {fw} x {fh} frame")
    return (fw - x0 - w, fh - y0 - h) if rotate180 else (x0, y0)


def crop(frame: np.ndarray, x0: int, y0: int, w: int, h: int, rotate180: bool = True) -> np.ndarray:
    """The window at result coordinates (x0, y0) of an un-rotated frame [H, W, ...], un-rotated like the frame itself:
    what a plain engine of source size w x h must be fed to see what the window engine sees.  With rotate180,
    crop(f, ...)[::-1, ::-1] == f[::-1, ::-1][y0:y0 + h, x0:x0 + w]."""
    bx0, by0 = buffer_origin((frame.shape[1], frame.shape[0]), x0, y0, w, h, rotate180)
    return np.ascontiguousarray(frame[by0:by0 + h, bx0:bx0 + w])


def window_map(full_size, window, x0, y0, rotate180=True, camera_matrix=None) -> dict:
    """irmv_window_map: buffer corner, the band of full-width HWC rows the window covers (byte offset and length in a
    frame) and the principal point of the window's pixels (cx - x0, cy - y0, in doubles)."""
    w, h = int(window[0]), int(window[1])
    bx0, by0 = buffer_origin(full_size, x0, y0, w, h, rotate180)
    pitch = int(full_size[0]) * 3
    out = dict(bx0=bx0, by0=by0, band_offset=by0 * pitch, band_bytes=h * pitch)
    if camera_matrix is not None:
        k = np.asarray(camera_matrix, np.float64).reshape(9)
        out["cx"], out["cy"] = float(k[2] - np.float64(x0)), float(k[5] - np.float64(y0))
    return out


def shifted_camera(camera_matrix, x0, y0):
    """The camera matrix (9 doubles, row-major) of a plain engine that sees the window's pixels."""
    k = [float(v) for v in np.asarray(camera_matrix, np.float64).reshape(9)]
    k[2], k[5] = k[2] - float(x0), k[5] - float(y0)
    return tuple(k)
