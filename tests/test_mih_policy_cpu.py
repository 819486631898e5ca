"""The MIH memory policy without a GPU: tests/cpp/mih_policy_test.cc over csrc/vc_mih_policy.hpp -- which of the optional per-table
structures (bucket-order code copies, {id, code} records, directory lines) an index gets for a shape, a free-memory figure and the
VC_MIH_BCODES / VC_MIH_BENT / VC_MIH_LINES knobs: every threshold at equality and one byte either side, the shapes and knob values
that override it, a failed free-memory query, the ABI's extremes against a 128-bit restatement, and the documented sizes."""
import os
import subprocess


def test_mih_memory_policy_thresholds_knobs_and_extremes(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "mih_policy_test"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-o", str(exe), os.path.join(root, "tests", "cpp", "mih_policy_test.cc")])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "all checks hold" in p.stdout, p.stdout + p.stderr
