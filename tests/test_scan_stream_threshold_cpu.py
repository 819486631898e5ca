"""The host arithmetic behind the stream kernel's split threshold test, without a GPU: tests/cpp/scan_stream_threshold_test.cc
over csrc/vc_scan_stream_plan.hpp -- chain base + fire level against the one-piece chain start, exhaustive over small key fields,
every tau and every count of matching streamed bits."""
import os
import subprocess


def test_chain_base_and_fire_level_agree_with_the_chain_start(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "scan_stream_threshold_test"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-o", str(exe), os.path.join(root, "tests", "cpp", "scan_stream_threshold_test.cc")])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "all checks hold" in p.stdout, p.stdout + p.stderr
