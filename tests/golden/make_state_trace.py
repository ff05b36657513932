"""Records tests/golden/state_trace.json: the script of tests/_state_trace.py run on the library as built from the commit whose
behaviour is to be kept (an MI355X is needed), one row per call -- counters, istep, launches per kernel of the profiled steps,
digests where the oracle has no entry point.  tests/test_state_trace_gpu.py holds every later build to it.

    python tests/golden/make_state_trace.py [output.json]
"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "taichi-2d-vof_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import _state_trace as st
from vof2d import _abi
from vof2d._lib import hip_api

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "state_trace.json")
    os.environ.setdefault("OMP_NUM_THREADS", "16")
    oracle = _abi.bind(ctypes.CDLL(os.path.join(ROOT, "oracle", "_build", "libvof_oracle.so")), "ovof_", optional=_abi.GPU_ONLY)
    hip = hip_api()
    trace = {case: st.run_case(hip, oracle, case) for case in st.CASES}
    trace["strips"] = st.run_strips(hip)
    with open(out, "w") as f:
        json.dump(trace, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%s: %d cases, %d rows" % (out, len(trace), sum(len(v) for v in trace.values())))
