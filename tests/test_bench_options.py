"""bench.py's options: a plain run does only what its reported line needs; --full adds the configs[2..4] lines and the CPU
baseline, at N = 1 only, as runs of their own after the reported workload."""
import pytest

import bench


@pytest.mark.parametrize("argv, world, want", [
    ([], 1, (False, False)),
    (["--gpus", "1", "--steps", "5", "--warmup", "2", "--dump-outputs", "out"], 1, (False, False)),
    (["--workload", "tr15_like", "--frames", "2"], 1, (False, False)),
    (["--full"], 1, (True, True)),
    (["--full", "--no-cpu-baseline"], 1, (True, False)),
    (["--full", "--no-other-workloads"], 1, (False, True)),
    (["--full", "--workload", "dragon"], 1, (False, True)),
    (["--full", "--spp", "64"], 1, (False, True)),
    (["--full"], 2, (False, False)),
])
def test_what_a_run_adds_to_the_reported_line(argv, world, want):
    assert bench.extras(bench.parse_args(argv), world) == want
