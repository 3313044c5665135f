"""Writes tests/golden/preprocess_trace.json: the C-ABI call logs of tests/test_hip_preprocess_trace.py's cases, as the
checked-out tree produces them on the GPU.  The committed fixture was written once, on the commit before preprocess_selected
became one plan and one loop, and pins that commit's calls; run this again only when a change of the calls is the purpose of a
pull request.

    python tests/golden/make_preprocess_trace.py [output path]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "preprocess_trace.json")
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE), HERE]

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    from test_hip_preprocess_trace import run_cases
    with open(out, "w") as f:
        json.dump(run_cases(), f, indent=None, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("wrote", out)
