"""The scan stream's host arithmetic without a GPU: tests/cpp/scan_stream_plan_test.cc over csrc/vc_scan_stream_plan.hpp -- the
common-prefix header of a granule (equal keys, adjacent keys, the whole key range, straddles of every power of two), the chain
start as a true lower bound for every key a header covers (exhaustive over small key fields), sizes, padding, the bytes a launch
streams and the memory rule."""
import os
import subprocess


def test_scan_stream_headers_bound_layout_and_memory_rule(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "scan_stream_plan_test"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-o", str(exe), os.path.join(root, "tests", "cpp", "scan_stream_plan_test.cc")])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "all checks hold" in p.stdout, p.stdout + p.stderr
