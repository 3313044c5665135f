"""Writes tests/golden/call_order_inputs.json: the engine call logs of tests/test_call_order_inputs.py's cases, as the
checked-out tree produces them.  The committed fixture was written once, on the commit that introduced the test, and pins
that commit's order; it is not regenerated when the orchestration is reorganised - run this again only when a change of the
order is the purpose of a pull request.  Two runs on one tree give the same bytes.

    python tests/golden/make_call_order_inputs.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "call_order_inputs.json")
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

if __name__ == "__main__":
    if not os.path.exists(OUT):                  # the test module reads the fixture when it is imported
        with open(OUT, "w") as f:
            f.write("{}\n")
    from test_call_order_inputs import run_cases
    with open(OUT, "w") as f:
        json.dump(run_cases(), f, indent=None, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("wrote", OUT)
