"""The scene options of the command line (vof2d/cli.py) that need no device: what parse_args accepts, and the refusals made
before anything starts."""
import json
import os

import pytest

from vof2d import cli, scene

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scenes")
DROPS = os.path.join(GOLDEN, "two_drops.json")


def exits_with(argv):
    with pytest.raises(SystemExit) as e:
        cli.parse_args(argv)
    assert isinstance(e.value.code, str), e.value.code          # the message itself: it says why
    return e.value.code


def test_the_defaults_and_what_is_accepted():
    a = cli.parse_args([])
    assert (a.scene, a.scene_over_ic, a.scene_samples, a.scene_shapes) == (None, False, None, None)
    a = cli.parse_args(["--scene", DROPS])
    assert a.scene_samples == 8 and a.scene_shapes.tobytes() == scene.load(DROPS)[0].tobytes() and not a.scene_over_ic
    a = cli.parse_args(["--scene", os.path.join(GOLDEN, "tilted_pool.json"), "--scene-over-ic", "-ic", "2", "--gpus", "2"])
    assert a.scene_samples == 16 and a.scene_over_ic and a.ic == 2 and len(a.scene_shapes) == 2
    a = cli.parse_args(["--scene", DROPS, "--scene-samples", "2", "--diag-every", "5", "--stats-every", "10"])
    assert a.scene_samples == 2


def test_a_scene_with_resume_exits_and_says_why(tmp_path):
    msg = exits_with(["--scene", DROPS, "--resume", str(tmp_path / "state.npz")])
    assert "--scene cannot be combined with --resume" in msg and "checkpoint" in msg


def test_a_missing_file_is_refused(tmp_path):
    msg = exits_with(["--scene", str(tmp_path / "nothing.json")])
    assert "nothing.json" in msg and "cannot be read" in msg


def test_a_bad_kind_key_phase_or_number_is_refused(tmp_path):
    def scene_file(doc):
        p = tmp_path / "s.json"
        p.write_text(doc if isinstance(doc, str) else json.dumps(doc))
        return str(p)

    disc = {"kind": "disc", "phase": "liquid", "cx": 0.05, "cy": 0.05, "r": 0.01}
    assert "unknown shape kind 'blob'" in exits_with(["--scene", scene_file({"shapes": [dict(disc, kind="blob")]})])
    assert "unknown key 'radius'" in exits_with(["--scene", scene_file({"shapes": [dict(disc, radius=1)]})])
    assert "unknown phase 'ice'" in exits_with(["--scene", scene_file({"shapes": [dict(disc, phase="ice")]})])
    assert "negative half extent" in exits_with(["--scene", scene_file({"shapes": [dict(disc, r=-0.01)]})])
    assert "samples must be one of" in exits_with(["--scene", scene_file({"samples": 5, "shapes": [disc]})])
    assert "samples must be one of" in exits_with(["--scene", scene_file({"shapes": [disc]}), "--scene-samples", "3"])
    assert "s.json" in exits_with(["--scene", scene_file("{not json")])


def test_the_options_that_belong_to_a_scene(capsys):
    for argv in (["--scene-over-ic"], ["--scene-samples", "4"]):
        with pytest.raises(SystemExit) as e:
            cli.parse_args(argv)
        assert e.value.code == 2 and "belong to --scene" in capsys.readouterr().err
