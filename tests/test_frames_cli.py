"""The frame options of the command line (vof2d/cli.py) that need no device: what parse_args accepts, and the refusals made
before anything starts."""
import pytest

from vof2d import cli


def refused(argv, capsys):
    with pytest.raises(SystemExit) as e:
        cli.parse_args(argv)
    assert e.value.code == 2
    return capsys.readouterr().err


def test_the_defaults_and_what_is_accepted():
    a = cli.parse_args([])
    assert (a.frames_every, a.frame, a.frame_block, a.frame_cmap, a.frame_contour) == (None, "F:0:1", None, None, False)
    a = cli.parse_args(["--frames-every", "100", "--frame", "VORT", "--frame-contour", "--frame-block", "4", "--frame-cmap", "grey"])
    assert (a.frames_every, a.frame, a.frame_block, a.frame_cmap, a.frame_contour) == (100, "VORT", 4, "grey", True)
    assert cli.parse_frame("F:0:1") == ("F", 0.0, 1.0) and cli.parse_frame("vort") == ("VORT", 0.0, 0.0) and cli.parse_frame("P:-1.5:2e3") == ("P", -1.5, 2000.0)
    # with the fixed number of V-cycles, and beside the other recording options
    a = cli.parse_args(["--frames-every", "10", "--pressure-solver", "mg", "--mg-cycles", "2", "--diag-every", "5", "--frame", "SPEED:0:0.5"])
    assert a.frames_every == 10 and a.mg_cycles == 2
    a = cli.parse_args(["--frames-every", "10", "--frame", "DYE", "--dye-box", "0,0.05,0,0.05"])
    assert a.frame == "DYE"


def test_refusals_before_anything_starts(capsys):
    assert "--frames-every needs N >= 1" in refused(["--frames-every", "0"], capsys)
    assert "--frames-every needs N >= 1" in refused(["--frames-every", "-3"], capsys)
    assert "is not one of F, U, V, SPEED, P, VORT, DYE" in refused(["--frames-every", "10", "--frame", "W"], capsys)
    assert "needs finite LO < HI" in refused(["--frames-every", "10", "--frame", "F:1:0"], capsys)
    assert "needs finite LO < HI" in refused(["--frames-every", "10", "--frame", "F:1:1"], capsys)
    assert "needs finite LO < HI" in refused(["--frames-every", "10", "--frame", "U:-inf:1"], capsys)
    assert "needs finite LO < HI" in refused(["--frames-every", "10", "--frame", "U:nan:1"], capsys)
    assert "LO and HI must be numbers" in refused(["--frames-every", "10", "--frame", "F:a:b"], capsys)
    assert "QUANTITY or QUANTITY:LO:HI" in refused(["--frames-every", "10", "--frame", "F:1"], capsys)
    assert "--frames-every runs on one GPU" in refused(["--frames-every", "10", "--gpus", "2"], capsys)
    assert "--frame-block needs K >= 1" in refused(["--frames-every", "10", "--frame-block", "0"], capsys)
    assert "--frame DYE shows the dye" in refused(["--frames-every", "10", "--frame", "DYE"], capsys)
