"""vof_step_mg without a GPU: the command line (--mg-cycles), the checkpoint entries, the ABI, and the restatement that
chooses the cycle count and the bound of tests/test_step_mg_gpu.py."""
import os
import re

import numpy as np
import pytest

import _step_mg_np as smg
import vof_oracle_np as onp
from vof2d import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_command_line_flag_and_refusals(capsys):
    from vof2d import cli
    a = cli.parse_args(["--pressure-solver", "mg", "--mg-cycles", "3", "--jacobi-crit", "rel"])
    assert a.mg_cycles == 3 and a.mg_coarse == "block" and a.jacobi_tol == 0.0
    num = cli.numerics_of(a, 4e-6)
    assert num["pressure_solver"] == "mg" and num["mg_cycles"] == 3 and num["mg_coarse"] == "block"
    assert cli.parse_args(["--pressure-solver", "mg", "--mg-cycles", "2", "--mg-coarse", "launches"]).mg_coarse == "launches"
    assert "mg_cycles" not in cli.numerics_of(cli.parse_args([]), 4e-6)          # checkpoints of other runs look as they did
    with pytest.raises(SystemExit) as e:                                            # stays the error it was
        cli.parse_args(["--pressure-solver", "mg"])
    assert e.value.code == 2 and "--jacobi-tol" in capsys.readouterr().err
    for bad in (["--mg-cycles", "2"], ["--pressure-solver", "cg", "--mg-cycles", "2"],
                ["--pressure-solver", "mg", "--mg-cycles", "2", "--jacobi-tol", "1e-8"],
                ["--pressure-solver", "mg", "--mg-cycles", "2", "--gpus", "2"],
                ["--pressure-solver", "mg", "--mg-cycles", "-1"]):
        with pytest.raises(SystemExit) as e:
            cli.parse_args(bad)
        assert e.value.code == 2 and "--mg-cycles" in capsys.readouterr().err, bad
    with pytest.raises(SystemExit):       # and before any engine is made when a launcher calls run() itself
        cli.run(cli.build_parser().parse_args(["--gpus", "2", "--pressure-solver", "mg", "--mg-cycles", "2"]),
                api=object(), rank=0, world=2)


def test_checkpoints_record_the_cycle_count_and_the_coarse_mode(tmp_path):
    from vof2d import cli
    f = {k: np.zeros((6, 6)) for k in ("F", "u", "v", "p")}
    runs = {"k2": ["--pressure-solver", "mg", "--mg-cycles", "2"], "k3": ["--pressure-solver", "mg", "--mg-cycles", "3"],
            "k2l": ["--pressure-solver", "mg", "--mg-cycles", "2", "--mg-coarse", "launches"],
            "tol": ["--pressure-solver", "mg", "--jacobi-tol", "1e-8"], "ten": []}
    args = {k: cli.parse_args(v) for k, v in runs.items()}
    for s in args:
        ck = str(tmp_path / (s + ".npz"))
        cli.save_state(ck, f, 5, 4, 4, "f64", 1, 0, cli.numerics_of(args[s], 4e-6))
        z = np.load(ck)
        assert ("num_mg_cycles" in z.files) == s.startswith("k") and ("num_mg_coarse" in z.files) == s.startswith("k")
        for t in args:
            if t == s:
                assert cli.load_state(ck, 4, 4, "f64", cli.numerics_of(args[t], 4e-6))[1] == 5
            else:
                with pytest.raises(SystemExit) as e:
                    cli.load_state(ck, 4, 4, "f64", cli.numerics_of(args[t], 4e-6))
                assert "--resume" in str(e.value) and "pass the same value to continue it" in str(e.value), (s, t)
                if s.startswith("k") and t.startswith("k"):
                    assert "mg-c" in str(e.value), (s, t)            # mg-cycles or mg-coarse, by name


def test_header_and_bindings_agree(hip_api, oracle_api):
    hdr = open(os.path.join(ROOT, "include", "vof2d.h")).read()
    m = re.search(r"int vof_step_mg\(([^;]*)\);", hdr)
    assert m, "include/vof2d.h does not declare vof_step_mg"
    types = [re.sub(r"\s*\w+$", "", a.strip()) for a in m.group(1).replace("\n", " ").split(",")]
    assert types == ["vof2d_handle", "int64_t", "int32_t", "int32_t", "double*", "double*", "int64_t*"]
    import ctypes as C
    res, argt = _abi.SIGNATURES["step_mg"]
    assert res is C.c_int
    assert argt == [_abi.H, C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    assert "step_mg" in _abi.GPU_ONLY
    assert hasattr(hip_api.lib, "vof_step_mg")
    assert not hasattr(oracle_api, "step_mg") and hasattr(oracle_api, "step")      # the oracle library loads without it
    assert "#define VOF_ABI_VERSION 2" in hdr and _abi.VOF_ABI_VERSION == 2


def test_restatement_at_64x64_more_cycles_a_smaller_residual_ten_sweeps_far_behind():
    """The table in tests/_step_mg_np.py, 64x64 rows, recomputed (each figure within 10 % of the docstring's: the sums of
    NumPy may be ordered differently on another machine)."""
    rows = smg.table(64)
    worst = {k: max(v) for k, v in rows.items()}
    print(" ".join("%s %.3e" % kv for kv in worst.items()))
    for k, doc in (("ten", 5.855e-02), (1, 1.249e-03), (2, 1.766e-04), (3, 2.509e-05)):
        assert abs(worst[k] - doc) <= 0.1 * doc, (k, worst[k], doc)
        assert len(rows[k]) == 50 and all(np.isfinite(rows[k]))
    assert worst[1] > worst[2] > worst[3]
    assert 100 * worst[3] <= worst["ten"]                      # the rule that chooses K, met here by K = 2 already
    assert all(m < t for m, t in zip(rows[1], rows["ten"]))     # one cycle beats ten sweeps in every single step


def test_restatement_steps_are_the_reference_steps_around_another_solve():
    """With the solve taken out of both, a restated step and the oracle's leave the same fields: the verbs around the
    cycles are the reference's, in its order."""
    a, b = onp.new_state(24, 20, 2, np.float64, "f32"), onp.new_state(24, 20, 2, np.float64, "f32")
    smg.step_ten(a, 3)
    onp.step(b, 3)
    for n in ("F", "u", "v", "p"):
        assert np.array_equal(getattr(a, n), getattr(b, n)), n
