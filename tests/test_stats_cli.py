"""The statistics options of the command line (vof2d/cli.py) that need no device: what parse_args accepts, and the refusals
made before anything starts."""
import pytest

from vof2d import cli


def refused(argv, capsys):
    with pytest.raises(SystemExit) as e:
        cli.parse_args(argv)
    assert e.value.code == 2
    return capsys.readouterr().err


def test_the_defaults_and_what_is_accepted():
    a = cli.parse_args([])
    assert (a.stats_every, a.stats, a.stats_level, a.stats_from, a.stats_save_every) == (None, "MOMENTS,ENVELOPE", 0.5, 0, None)
    a = cli.parse_args(["--stats-every", "8", "--stats", "envelope", "--stats-level", "1", "--stats-from", "400", "--stats-save-every", "1000"])
    assert (a.stats_every, a.stats, a.stats_level, a.stats_from, a.stats_save_every) == (8, "envelope", 1.0, 400, 1000)
    assert cli.parse_args(["--stats-every", "1", "--stats", "MOMENTS"]).stats == "MOMENTS"
    # beside the other recording options and the fixed number of V-cycles
    a = cli.parse_args(["--stats-every", "10", "--pressure-solver", "mg", "--mg-cycles", "2", "--diag-every", "5", "--frames-every", "20"])
    assert a.stats_every == 10 and a.mg_cycles == 2 and a.diag_every == 5
    a = cli.parse_args(["--stats-every", "10", "--dye-box", "0,0.05,0,0.05", "--dye-every", "5"])
    assert a.stats_every == 10 and a.dye_every == 5
    a = cli.parse_args(["--stats-every", "10", "--gauge", "0.01,0.02", "--gauges-every", "5", "--tracers", "100"])
    assert a.stats_every == 10 and a.gauges_every == 5 and a.tracers == 100
    assert "not part of a checkpoint" in " ".join(cli.build_parser().format_help().split())


def test_refusals_before_anything_starts(capsys):
    assert "--stats-every needs N >= 1" in refused(["--stats-every", "0"], capsys)
    assert "--stats-every needs N >= 1" in refused(["--stats-every", "-2"], capsys)
    assert "statistics over row strips are not built" in refused(["--stats-every", "10", "--gpus", "2"], capsys)
    assert "--stats-save-every needs M >= 1" in refused(["--stats-every", "10", "--stats-save-every", "0"], capsys)
    assert "--stats-level needs 0 < L <= 1" in refused(["--stats-every", "10", "--stats-level", "0"], capsys)
    assert "--stats-level needs 0 < L <= 1" in refused(["--stats-every", "10", "--stats-level", "1.5"], capsys)
    assert "--stats-level needs 0 < L <= 1" in refused(["--stats-every", "10", "--stats-level", "nan"], capsys)
    assert "unknown statistics group" in refused(["--stats-every", "10", "--stats", "MOMENTS,PRESSURE"], capsys)
    assert "unknown statistics group" in refused(["--stats-every", "10", "--stats", ""], capsys)
    assert "--stats-from needs STEP >= 0" in refused(["--stats-every", "10", "--stats-from", "-1"], capsys)
    assert "pass that too" in refused(["--stats-save-every", "10"], capsys)
    # with the fixed number of V-cycles too (that branch of parse_args returns early)
    assert "--stats-every needs N >= 1" in refused(["--stats-every", "0", "--pressure-solver", "mg", "--mg-cycles", "2"], capsys)
