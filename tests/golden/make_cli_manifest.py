"""What two runs of the command line leave behind, as SHA-256 digests: tests/golden/cli_recorders_64.json.

    python tests/golden/make_cli_manifest.py [--out FILE]

runs vof2d.cli.run at 64 x 64 f64, -ic 3 for the two command lines of CASES -- every recording option between them --
in temporary directories, twice, and keeps the entries whose digests agree between the two runs.  It is run on the
commit BEFORE a change to the command line's main loop; tests/test_cli_manifest_gpu.py then holds the changed loop to
the file.  An entry is

    <case>/<path>          a .csv or .npy file under data/ (its bytes)
    <case>/<path>:<name>   an array inside an .npz under data/ (name, dtype, shape, bytes; never the zip container)
    <case>/<path>          an output/frame_*.png, decoded to pixels (shape, bytes)
    <case>/out             the lines passed to `out`, the run's directory written as `.`

The case `resume` is the first command line again, as 20 steps and a second run resumed from the step-20 checkpoint
in the same directory (a resumed run appends to the CSV files).  It is held to the entries of `recorders`; the file
lists under `resume` only the entries that differ from those on the recording commit: the statistics (they start anew
on a resume: the planes are not part of a checkpoint), the tracers' TIME in data/tracers.csv and tracers_state.npz (a
resumed run adds the checkpoint's time to the handle's own sum: other last bits) and the lines passed to `out`.
"""
import hashlib
import json
import os
import struct
import sys
import tempfile
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
MANIFEST = os.path.join(HERE, "cli_recorders_64.json")
GRID = "-ic 3 --nx 64 --ny 64 --dtype f64 "
CASES = {
    "recorders": "--steps 40 --diag-every 5 --interface-every 10 --blobs-every 10 --tracers 50 --tracers-every 4 --tracers-save-every 20 "
                 "--gauge 0.05,0.01 --gauges-every 8 --depths-every 10 --frames-every 20 --frame VORT --frame-contour --stats-every 4 "
                 "--stats-from 8 --stats-save-every 20 --save-every 20",
    "mg_dye": "--steps 24 --pressure-solver mg --mg-cycles 2 --jacobi-crit rel --dye-box 0,0.1,0.05,0.1 --dye-every 5 --dye-save-every 12 "
              "--frames-every 12 --frame DYE --stats-every 3 --save-every 12",
}
RESUME_AT = 20
# at least one entry of each must be in the file: a recorder whose files all dropped out would go unchecked
MUST_LIST = {
    "recorders": ("data/diagnostics.csv", "data/interface.csv", "data/interface_", "data/blobs.csv", "data/tracers.csv", "data/tracers_0",
                  "data/tracers_state.npz", "data/gauges.csv", "data/gauges_state.npz", "data/depths.csv", "data/depths_", "data/frames.csv",
                  "output/frame_", "data/stats.csv", "data/stats_", "data/00000020.npz", "data/00000040.npz", "out"),
    "mg_dye": ("data/dye.csv", "data/dye_0", "data/dye_state.npz", "data/frames.csv", "output/frame_", "data/stats.csv", "data/stats_",
               "data/00000012.npz", "data/00000024.npz", "out"),
}


def _sha(*parts):
    h = hashlib.sha256()
    for p in parts:
        h.update(p if isinstance(p, bytes) else str(p).encode())
        h.update(b"\0")
    return h.hexdigest()


def png_pixels(path):
    """(height, width, 3) uint8 of an 8-bit RGB PNG whose rows all have filter 0 (what vof2d.frames.write_png writes)."""
    raw = open(path, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n", path
    at, idat, w, h = 8, b"", 0, 0
    while at < len(raw):
        n, tag = struct.unpack(">I", raw[at:at + 4])[0], raw[at + 4:at + 8]
        body = raw[at + 8:at + 8 + n]
        if tag == b"IHDR":
            w, h, depth, colour, _, _, interlace = struct.unpack(">IIBBBBB", body)
            assert (depth, colour, interlace) == (8, 2, 0), path
        elif tag == b"IDAT":
            idat += body
        at += 12 + n
    rows = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(h, 1 + 3 * w)
    assert not rows[:, 0].any(), "%s: a filtered row" % path
    return np.ascontiguousarray(rows[:, 1:]).reshape(h, w, 3)


def digest(directory, lines):
    """{entry: sha256} of what a run left in `directory` and of the lines it passed to `out`."""
    found = {}
    data = os.path.join(directory, "data")
    for name in sorted(os.listdir(data)):
        path = os.path.join(data, name)
        if name.endswith(".csv") or name.endswith(".npy"):
            found["data/" + name] = _sha(open(path, "rb").read())
        elif name.endswith(".npz"):
            with np.load(path, allow_pickle=False) as z:
                for key in sorted(z.files):
                    a = np.ascontiguousarray(z[key])
                    found["data/%s:%s" % (name, key)] = _sha(key, a.dtype.str, a.shape, a.tobytes())
    output = os.path.join(directory, "output")
    for name in sorted(os.listdir(output)):
        if name.startswith("frame_") and name.endswith(".png"):
            px = png_pixels(os.path.join(output, name))
            found["output/" + name] = _sha(px.shape, px.tobytes())
    found["out"] = _sha("\n".join(ln.replace(os.path.realpath(directory), ".").replace(directory, ".") for ln in lines))
    return found


def _cli_run(api, argv, lines):
    from vof2d import cli
    rc = cli.run(cli.parse_args((GRID + argv).split()), api=api, world=1, rank=0, out=lambda *a: lines.append(" ".join(str(x) for x in a)))
    assert rc == 0, argv


def run_case(api, case, directory):
    """One case in `directory` (made the working directory for the run); {entry: sha256}."""
    back = os.getcwd()
    os.chdir(directory)
    try:
        lines = []
        if case == "resume":
            argv = CASES["recorders"]
            _cli_run(api, argv.replace("--steps 40", "--steps %d" % RESUME_AT), lines)
            _cli_run(api, argv + " --resume data/%08d.npz" % RESUME_AT, lines)
        else:
            _cli_run(api, CASES[case], lines)
    finally:
        os.chdir(back)
    return digest(directory, lines)


def run_all(api):
    """{case: {entry: sha256}} of the three cases, each in a fresh temporary directory."""
    found = {}
    for case in tuple(CASES) + ("resume",):
        with tempfile.TemporaryDirectory() as d:
            found[case] = run_case(api, case, d)
    return found


def expected(manifest, case):
    """The entries `case` is held to: those of the file; `resume` those of `recorders` with the file's `resume` entries in their place."""
    if case != "resume":
        return manifest[case]
    return dict(manifest["recorders"], **manifest["resume"])


def main(argv):
    out = argv[argv.index("--out") + 1] if "--out" in argv else MANIFEST
    sys.path[:0] = [os.path.join(ROOT, "taichi-2d-vof_amd")]
    from vof2d._lib import hip_api
    api = hip_api()
    first, second = run_all(api), run_all(api)
    kept, dropped = {}, []
    for case in first:
        assert sorted(first[case]) == sorted(second[case]), "%s: the two runs left different files" % case
        kept[case] = {k: v for k, v in first[case].items() if second[case][k] == v}
        dropped += ["%s/%s" % (case, k) for k in first[case] if k not in kept[case]]
    for case, prefixes in MUST_LIST.items():
        for p in prefixes:
            assert any(k.startswith(p) for k in kept[case]), "%s: no entry of %s agrees between the two runs" % (case, p)
    differs = sorted(k for k, v in kept["resume"].items() if kept["recorders"].get(k) != v)
    gone = sorted(k for k in kept["recorders"] if k not in kept["resume"])
    kept["resume"] = {k: kept["resume"][k] for k in differs}
    with open(out, "w") as f:
        json.dump(kept, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%s: %s entries; dropped (the two runs disagree): %s; resume differs from recorders in: %s; resume lacks: %s" %
          (out, {c: len(v) for c, v in kept.items()}, dropped or "none", differs or "none", gone or "none"))


if __name__ == "__main__":
    main(sys.argv[1:])
