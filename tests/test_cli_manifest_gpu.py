"""The command line's main loop against tests/golden/cli_recorders_64.json, which tests/golden/make_cli_manifest.py recorded
on the commit before the loop became a list of recorders (vof2d/recorders.py): two command lines that use every recording
option between them, 64 x 64 f64, and the first again as 20 steps and a resumed run.  Every file under data/ (the arrays inside
the .npz files one by one), every frame (as pixels) and the lines passed to `out` must have the digest recorded there."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def load_maker():
    spec = importlib.util.spec_from_file_location("make_cli_manifest", os.path.join(HERE, "golden", "make_cli_manifest.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


maker = load_maker()
with open(maker.MANIFEST) as f:
    MANIFEST = json.load(f)


def test_the_manifest_lists_every_recorder():
    for case, prefixes in maker.MUST_LIST.items():
        for p in prefixes:
            assert any(k.startswith(p) for k in MANIFEST[case]), (case, p)
    # a resumed run differs from the whole one in the statistics (they start anew), the tracers' TIME and the lines of `out` alone
    assert all(k.startswith(("data/stats", "data/tracers.csv", "data/tracers_state.npz:time")) or k == "out" for k in MANIFEST["resume"])


@pytest.mark.parametrize("case", ["recorders", "mg_dye", "resume"])
def test_the_run_leaves_what_the_recording_commit_left(hip_api, tmp_path, case):
    got = maker.run_case(hip_api, case, str(tmp_path))
    want = maker.expected(MANIFEST, case)
    assert sorted(got) == sorted(want), "other files or arrays: %s" % sorted(set(got) ^ set(want))
    differ = sorted(k for k in want if got[k] != want[k])
    assert not differ, "%s: other contents in %s" % (case, differ)
