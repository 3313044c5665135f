"""Writes tests/golden/api_trace.txt: the launch trace of the C++ composites over tests/test_api_trace.py's cases, as the
checked-out csrc/api.cpp produces it.  The committed fixture was written once, on the commit that introduced the test, and pins
that commit's launches; run this again only when a change of the launch sequence is the purpose of a pull request.

    python tests/golden/make_api_trace.py
"""
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "api_trace.txt")
sys.path[:0] = [os.path.dirname(HERE)]

if __name__ == "__main__":
    from test_api_trace import run_trace
    with tempfile.TemporaryDirectory() as d:
        trace = run_trace(d)
    with open(OUT, "wb") as f:
        f.write(trace)
    print("wrote", OUT, "(%d lines)" % trace.count(b"\n"))
