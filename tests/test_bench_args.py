"""bench.py's command line without a GPU: a plain run skips every measurement and check beyond its headline figure, --full runs them
all unless a --no-* option skips one."""
import bench

SKIPS = ("no_long_runs", "no_parity_check", "no_once_per_step", "no_cpu_baseline", "no_secondary", "no_batch_256")


def test_plain_run_skips_everything_beyond_the_headline():
    a = bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert not a.full and (a.steps, a.warmup, a.filter, a.dtype, a.batch, a.landmarks) == (20, 5, "ekf", "f64", 65536, 50)
    for k in SKIPS:
        assert getattr(a, k), k


def test_full_runs_everything_unless_skipped():
    a = bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5", "--full"])
    assert a.full
    for k in SKIPS:
        assert not getattr(a, k), k
    a = bench.parse_args(["--full", "--no-cpu-baseline", "--no-long-runs"])
    assert a.no_cpu_baseline and a.no_long_runs and not a.no_parity_check and not a.no_once_per_step and not a.no_secondary


def test_pose_graph_defaults_follow_the_given_arguments():
    a = bench.parse_args(["--filter", "pgs"])
    assert (a.landmarks, a.batch, a.steps, a.warmup) == (200, 2048, 5, 1)
    a = bench.parse_args(["--filter", "pgs", "--iterative", "--steps", "2"])
    assert (a.landmarks, a.batch, a.steps, a.warmup) == (200, 256, 2, 1)
