"""The --regrid-from options of the command line (vof2d/cli.py) that need no device: what parse_args accepts, and the refusals
made before anything starts.  Without the option nothing about --resume changes: load_state still refuses another grid."""
import numpy as np
import pytest

from vof2d import cli


def exits_with(argv):
    with pytest.raises(SystemExit) as e:
        cli.parse_args(argv)
    assert isinstance(e.value.code, str), e.value.code          # the message itself: it says why
    return e.value.code


def test_the_defaults_and_what_is_accepted():
    a = cli.parse_args([])
    assert (a.regrid_from, a.regrid_no_plic) == (None, False)
    a = cli.parse_args(["--regrid-from", "data/00000020.npz", "--nx", "128", "--ny", "128", "--dt", "2e-6", "--diag-every", "5"])
    assert a.regrid_from == "data/00000020.npz" and not a.regrid_no_plic and a.dt == 2e-6
    assert cli.parse_args(["--regrid-from", "x.npz", "--regrid-no-plic"]).regrid_no_plic


@pytest.mark.parametrize("extra,name", [(["--resume", "data/00000020.npz"], "--resume"), (["--gpus", "2"], "--gpus N")])
def test_what_it_cannot_be_combined_with(extra, name):
    msg = exits_with(["--regrid-from", "x.npz"] + extra)
    assert "--regrid-from cannot be combined with " + name in msg


def test_a_scene_is_refused_too(tmp_path):
    p = tmp_path / "s.json"
    p.write_text('{"shapes": [{"kind": "disc", "phase": "liquid", "cx": 0.05, "cy": 0.05, "r": 0.01}]}')
    assert "--regrid-from cannot be combined with --scene" in exits_with(["--regrid-from", "x.npz", "--scene", str(p)])


def test_no_plic_belongs_to_regrid_from(capsys):
    with pytest.raises(SystemExit) as e:
        cli.parse_args(["--regrid-no-plic"])
    assert e.value.code == 2 and "--regrid-no-plic belongs to --regrid-from" in capsys.readouterr().err


def test_resume_still_refuses_another_grid(tmp_path):
    path = str(tmp_path / "state.npz")
    z = np.zeros((66, 66))
    cli.save_state(path, {f: z for f in cli.STATE}, 20, 64, 64, "f64", 1)
    with pytest.raises(SystemExit) as e:
        cli.load_state(path, 128, 128, "f64")
    assert "holds a 64x64 f64 run, this one is 128x128 f64" in str(e.value.code)
