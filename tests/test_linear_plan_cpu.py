"""The linear scan driver's host arithmetic without a GPU: tests/cpp/linear_plan_test.cc over csrc/vc_linear_plan.hpp -- the plan of
a call (tile, group, histogram stride, bootstrap sample), the carving of the per-group state, the recovery scratch layout, and the
interval arithmetic of the host-driven ring-overflow recovery against a simulated scan (random and adversarial arrival order)."""
import os
import subprocess


def test_linear_plan_state_layout_and_recovery_interval(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "linear_plan_test"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-o", str(exe), os.path.join(root, "tests", "cpp", "linear_plan_test.cc")])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "all checks hold" in p.stdout, p.stdout + p.stderr
