"""Scenes for vof_set_scene (include/vof2d.h): an ordered list of shapes painted into F on the device.

A shape is one record of VOF_SHAPE_N doubles, KIND, PHASE, A0 .. A5; the constructors below return it as a tuple of floats (`polygon`
returns a list of them).  `pack` stacks a list into the (n, VOF_SHAPE_N) float64 array the library takes, with the library's own
checks; `loads` / `load` read a scene written as JSON:

    {"samples": 8,
     "shapes": [{"kind": "disc", "phase": "liquid", "cx": 0.03, "cy": 0.05, "r": 0.01},
                {"kind": "rect", "phase": "gas", "x0": 0.0, "x1": 0.1, "y0": 0.09, "y1": 0.1}]}

The kinds and their keys (every shape also has "phase": "liquid" or "gas"):
    rect       x0, x1, y0, y1
    box        cx, cy, hx, hy, angle (degrees, default 0)
    disc       cx, cy, r
    ellipse    cx, cy, hx, hy, angle (degrees, default 0)
    halfplane  px, py, nx, ny        (the side the normal points away from)
    triangle   points: three [x, y]
    polygon    points: three or more [x, y] of a convex polygon, expanded to a fan of triangles
"""
import json
import math

import numpy as np

from . import _abi

PHASES = {"gas": _abi.VOF_SCENE_GAS, "liquid": _abi.VOF_SCENE_LIQUID}
SUMMARY = ("SHAPES", "SAMPLES", "PAINTED", "MIXED", "ISTEP")
SAMPLES = (1, 2, 4, 8, 16)


def summary_of(row):
    return {name: row[getattr(_abi, "VOF_SCENE_SUM_" + name)] for name in SUMMARY}


def phase_code(phase):
    if isinstance(phase, str):
        if phase not in PHASES:
            raise ValueError("unknown phase %r (liquid or gas)" % (phase,))
        return PHASES[phase]
    return int(phase)


def _cos_sin(angle_deg):
    """The cosine and sine of an angle in degrees; the multiples of 90 degrees exactly."""
    q = math.fmod(float(angle_deg), 360.0)
    exact = {0.0: (1.0, 0.0), 90.0: (0.0, 1.0), 180.0: (-1.0, 0.0), 270.0: (0.0, -1.0),
             -90.0: (0.0, -1.0), -180.0: (-1.0, 0.0), -270.0: (0.0, 1.0)}
    if q in exact:
        return exact[q]
    return math.cos(math.radians(q)), math.sin(math.radians(q))


def _record(kind, phase, *a):
    return (float(kind), float(phase_code(phase))) + tuple(float(x) for x in a) + (0.0,) * (6 - len(a))


def box(cx, cy, hx, hy, angle_deg=0.0, phase="liquid"):
    c, s = _cos_sin(angle_deg)
    return _record(_abi.VOF_SHAPE_BOX, phase, cx, cy, hx, hy, c, s)


def rect(x0, x1, y0, y1, phase="liquid"):
    """The axis-aligned box [x0, x1] x [y0, y1]."""
    x0, x1, y0, y1 = float(x0), float(x1), float(y0), float(y1)
    return box((x0 + x1) * 0.5, (y0 + y1) * 0.5, (x1 - x0) * 0.5, (y1 - y0) * 0.5, 0.0, phase)


def ellipse(cx, cy, hx, hy, angle_deg=0.0, phase="liquid"):
    c, s = _cos_sin(angle_deg)
    return _record(_abi.VOF_SHAPE_ELLIPSE, phase, cx, cy, hx, hy, c, s)


def disc(cx, cy, r, phase="liquid"):
    return ellipse(cx, cy, r, r, 0.0, phase)


def halfplane(px, py, nx, ny, phase="liquid"):
    """The points p with (p - (px, py)) . (nx, ny) <= 0."""
    return _record(_abi.VOF_SHAPE_HALFPLANE, phase, px, py, nx, ny)


def triangle(p0, p1, p2, phase="liquid"):
    return _record(_abi.VOF_SHAPE_TRIANGLE, phase, p0[0], p0[1], p1[0], p1[1], p2[0], p2[1])


def polygon(points, phase="liquid"):
    """A convex polygon as the fan of triangles (p0, pk, pk+1); a list of records."""
    pts = [(float(p[0]), float(p[1])) for p in points]
    if len(pts) < 3:
        raise ValueError("a polygon needs at least three points")
    return [triangle(pts[0], pts[k], pts[k + 1], phase) for k in range(1, len(pts) - 1)]


def check_record(r):
    """What scene_check_record of the library (runtime/scene.h) refuses, as a ValueError."""
    if len(r) != _abi.VOF_SHAPE_N:
        raise ValueError("a shape record has %d numbers, not %d" % (len(r), _abi.VOF_SHAPE_N))
    if not all(math.isfinite(x) for x in r):
        raise ValueError("a shape record holds a number that is not finite: %r" % (tuple(r),))
    kind, phase, a = r[0], r[1], r[2:]
    if kind not in (_abi.VOF_SHAPE_BOX, _abi.VOF_SHAPE_ELLIPSE, _abi.VOF_SHAPE_HALFPLANE, _abi.VOF_SHAPE_TRIANGLE):
        raise ValueError("unknown shape kind %r" % (kind,))
    if phase not in (_abi.VOF_SCENE_GAS, _abi.VOF_SCENE_LIQUID):
        raise ValueError("unknown phase %r" % (phase,))
    if kind in (_abi.VOF_SHAPE_BOX, _abi.VOF_SHAPE_ELLIPSE):
        if a[2] < 0.0 or a[3] < 0.0:
            raise ValueError("a box or an ellipse has a negative half extent: %r" % (tuple(r),))
        if not abs(a[4] * a[4] + a[5] * a[5] - 1.0) <= 1e-9:
            raise ValueError("c, s of a box or an ellipse are not a cosine and a sine: %r" % (tuple(r),))
    elif kind == _abi.VOF_SHAPE_HALFPLANE:
        if a[2] == 0.0 and a[3] == 0.0:
            raise ValueError("a half-plane has a zero normal")


def flatten(shapes):
    """The records of a list whose items are records or lists of records (what `polygon` returns)."""
    out = []
    for s in shapes:
        if len(s) and isinstance(s[0], (tuple, list, np.ndarray)):
            out.extend(tuple(float(x) for x in r) for r in s)
        else:
            out.append(tuple(float(x) for x in s))
    return out


def pack(shapes):
    """The (n, VOF_SHAPE_N) float64 array of a list of shapes (an array of that shape passes through), checked like the library checks it."""
    if isinstance(shapes, np.ndarray) and shapes.ndim == 2:
        recs = [tuple(float(x) for x in r) for r in shapes]
    else:
        recs = flatten(shapes)
    if len(recs) > _abi.VOF_SCENE_MAX_SHAPES:
        raise ValueError("%d shapes: at most %d" % (len(recs), _abi.VOF_SCENE_MAX_SHAPES))
    for r in recs:
        check_record(r)
    return np.array(recs, dtype=np.float64).reshape(len(recs), _abi.VOF_SHAPE_N)


def check_samples(samples):
    if samples not in SAMPLES or isinstance(samples, bool):
        raise ValueError("samples must be one of %s, not %r" % (SAMPLES, samples))
    return int(samples)


# ---- JSON
_KEYS = {
    "rect": ("x0", "x1", "y0", "y1"),
    "box": ("cx", "cy", "hx", "hy"),
    "disc": ("cx", "cy", "r"),
    "ellipse": ("cx", "cy", "hx", "hy"),
    "halfplane": ("px", "py", "nx", "ny"),
    "triangle": ("points",),
    "polygon": ("points",),
}
_OPTIONAL = {"box": ("angle",), "ellipse": ("angle",)}


def shape_of(d):
    """The record(s) of one JSON shape."""
    if not isinstance(d, dict):
        raise ValueError("a shape must be an object, not %r" % (d,))
    kind = d.get("kind")
    if kind not in _KEYS:
        raise ValueError("unknown shape kind %r (one of %s)" % (kind, ", ".join(sorted(_KEYS))))
    allowed = ("kind", "phase") + _KEYS[kind] + _OPTIONAL.get(kind, ())
    for k in d:
        if k not in allowed:
            raise ValueError("unknown key %r in a %s" % (k, kind))
    for k in ("phase",) + _KEYS[kind]:
        if k not in d:
            raise ValueError("a %s needs the key %r" % (kind, k))
    phase = phase_code(d["phase"])
    if kind == "rect":
        return rect(d["x0"], d["x1"], d["y0"], d["y1"], phase)
    if kind == "box":
        return box(d["cx"], d["cy"], d["hx"], d["hy"], d.get("angle", 0.0), phase)
    if kind == "disc":
        return disc(d["cx"], d["cy"], d["r"], phase)
    if kind == "ellipse":
        return ellipse(d["cx"], d["cy"], d["hx"], d["hy"], d.get("angle", 0.0), phase)
    if kind == "halfplane":
        return halfplane(d["px"], d["py"], d["nx"], d["ny"], phase)
    pts = d["points"]
    if kind == "triangle":
        if len(pts) != 3:
            raise ValueError("a triangle needs three points")
        return triangle(pts[0], pts[1], pts[2], phase)
    return polygon(pts, phase)


def loads(text):
    """(records, samples) of a scene written as JSON: the (n, VOF_SHAPE_N) array of `pack` and the file's samples (default 8)."""
    doc = json.loads(text)
    if not isinstance(doc, dict):
        raise ValueError("a scene must be an object with the key 'shapes'")
    for k in doc:
        if k not in ("samples", "shapes"):
            raise ValueError("unknown key %r in a scene" % (k,))
    if "shapes" not in doc:
        raise ValueError("a scene needs the key 'shapes'")
    samples = check_samples(doc.get("samples", 8))
    return pack([shape_of(s) for s in doc["shapes"]]), samples


def load(path):
    with open(path) as f:
        return loads(f.read())
