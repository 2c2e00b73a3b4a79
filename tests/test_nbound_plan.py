"""The noise-target calls' schedule with a neighbour bound (csrc/hip/noise_plan.h, include/trayhip.h: tray_scene_set_noise_ratio), stand-alone:
tests/emu/nbound_plan_check.cpp runs tr_ntplan::run over scripted Ops -- errors from a table, renders that only count -- and checks where the
rounds end. This module builds it with g++ and runs it; the program is also what a host-sanitizer build compiles (its head comment).

Cases (the program's): (i) a strip of 5 x 1 tiles whose first tile never converges, min 2, max 64: ratio 4 must end at exactly
n = [64, 16, 4, 2, 2] and ratio 2 at [64, 32, 16, 8, 4], the least fixed point, so no tile is pulled without need; (ii) a 3 x 3 grid with the
centre noisy: the eight neighbours alike; (iii) a range over part of the grid; (iv) no bound: the unbounded call's groups; (v) the launch and
read counts are the plan's constexpr."""
import os
import subprocess

import numpy as np
import pytest

import _nbound_ref as NB

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("nbound_plan") / "nbound_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(EMU_DIR, "nbound_plan_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.splitlines()


def line(output, head):
    found = [l for l in output if l.startswith(head)]
    assert len(found) == 1, (head, output)
    return found[0]


def test_every_case_passes(output):
    assert output[-1] == "ok" and not any("WRONG" in l for l in output)


@pytest.mark.parametrize("head,n", [("(i) strip 5x1, ratio 4 ", "64 16 4 2 2"), ("(i) strip 5x1, ratio 2 ", "64 32 16 8 4"), ("(i) strip 5x1, no bound", "64 2 2 2 2"),
                                    ("(ii) 3x3, centre noisy, ratio 4", "16 16 16 64 16 16 16 16 16"),
                                    ("(iii) left half of 4x2, tile (1, 0) noisy, ratio 4", "16 64 16 16"), ("(iii) tiles apart in 4x2", "64 2 2")])
def test_the_rounds_end_at_the_least_fixed_point(output, head, n):
    assert f"n = {n}," in line(output, head)


def test_no_bound_is_the_unbounded_schedule_and_the_counts_are_the_plans(output):
    assert "WRONG" not in line(output, "(iv)") and "WRONG" not in line(output, "(v)")
    assert "81 launches, 6 reads, by hand 81" in line(output, "(v)")


@pytest.mark.parametrize("ratio,n", [(4, [64, 16, 4, 2, 2]), (2, [64, 32, 16, 8, 4]), (0, [64, 2, 2, 2, 2])])
def test_the_numpy_statement_ends_where_the_program_does(ratio, n):
    """_nbound_ref.next_set, the statement the emulation and GPU tests compare with, on case (i)"""
    strip = np.array([(x, 0) for x in range(5)], np.uint32)
    assert NB.run_rounds(strip, [1 << 30, 0, 0, 0, 0], 2, 64, ratio).tolist() == n
