"""The schedule of pgs_solve is the recorded one (live_ekf_slam_amd/csrc/host/pgs_schedule.h holds its rules, pgs_capi.cpp its phases).

A solve's schedule is deterministic: every host read of a trial's counters is a blocking event wait and the solve groups own disjoint
ranges of the batch, so the running slots per trial of every group (last_solve_timeline) are equal as whole integer lists from run to run,
and with them the trials launched and every graph's iteration and trial counts.  tests/golden/pgs_schedule.json holds what the library
reported for the configurations below at commit 6091b81, before pgs_solve was taken apart into phases; it was recorded by running this
module as a script on an MI355X:

    python tests/test_pgs_schedule_gpu.py --record

The recorder notes the commit git reports for the tree and the sha256 of the library it loaded; only in a copy of the tree without its .git
does it take the commit from the command line (--record COMMIT), which is how the present file, from such a copy of 6091b81, came about.

Two recordings in a row were byte-identical.  The fixture is re-recorded ONLY when a change alters the schedule on purpose (another group
rule, lane switch, streaming hand-over ...); a refactor of the host loop must reproduce it.  It holds nothing but this library's own reports."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "pgs_schedule.json")

pytestmark = pytest.mark.gpu

# the scenario of test_parity_pgs_gpu.test_streaming_slots_do_not_change_results
L, T, KP, B, SEED = 20, 150, 8, 45, 4
# (groups, slots, SLAM_PGS_LANES): lockstep with one and two groups, streaming with one group, a share that lets only group 0 stream
# (22 of 23 | 22 of 22), no lambda lanes, three groups streaming with ranges 15, 15, 15
CONFIGS = [(1, 0, 4), (2, 0, 4), (1, 7, 4), (2, 44, 4), (1, 0, 1), (3, 8, 4)]
B_AUTO, T_EVERY = 130, 20   # the automatic group count: two groups from 128 instances, one per tick of an every-iteration run


def _key(cfg):
    return "groups %d slots %d lanes %d" % cfg


def _handle(batch, lanes):
    """A handle of `batch` instances of the scenario after its T ticks, created with SLAM_PGS_LANES = lanes (None: unset)."""
    import live_ekf_slam_amd as S
    from live_ekf_slam_amd.config import default_config
    from live_ekf_slam_amd.scenario import make_scenario
    lm, cmds = make_scenario(9, L, T)
    old = os.environ.pop("SLAM_PGS_LANES", None)
    if lanes is not None:
        os.environ["SLAM_PGS_LANES"] = str(lanes)
    try:
        pg = S.BatchedPoseGraph(batch, num_iterations=T + 1, L_max=L, k_per_pose=KP).readParams(default_config())
    finally:
        os.environ.pop("SLAM_PGS_LANES", None)
        if old is not None:
            os.environ["SLAM_PGS_LANES"] = old
    pg.set_map(lm); pg.set_seed(SEED); pg.init(0.0, 0.0, 0.0)
    return pg, cmds


def _timeline(pg):
    return [a.tolist() for a in pg.last_solve_timeline()]


def observe_config(cfg):
    groups, slots, lanes = cfg
    pg, cmds = _handle(B, lanes)
    pg.set_groups(groups); pg.set_slots(slots)
    pg.run_sim(cmds); pg.solvePoseGraph()
    st = pg.stats()
    out = dict(timeline=_timeline(pg), iterations=st["iterations"].tolist(), trials=st["trials"].tolist(),
               trials_launched=int(pg.last_solve_work()[1]))
    pg.set_profiling(True)      # (last_solve_paths reports the elimination order of a profiled solve)
    pg.solvePoseGraph()
    paths = pg.last_solve_paths()
    out["segmented"] = bool(paths["segmented"]); out["segment_length"] = int(paths["segment_length"])
    pg.close()
    return out


def observe_auto_groups():
    pg, cmds = _handle(B_AUTO, None)
    pg.run_sim(cmds); pg.solvePoseGraph()
    out = dict(timeline=_timeline(pg))
    pg.close()
    pg, cmds = _handle(B_AUTO, None)
    pg.run_sim_every_iteration(cmds[:T_EVERY])
    out["timeline_last_tick"] = _timeline(pg)
    pg.solvePoseGraph()
    out["timeline_after_ticks"] = _timeline(pg)
    pg.close()
    return out


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("cfg", CONFIGS, ids=_key)
def test_solve_schedule_is_the_recorded_one(recorded, cfg):
    want, got = recorded["configs"][_key(cfg)], observe_config(cfg)
    assert len(got["timeline"]) == cfg[0]
    for key in ("timeline", "iterations", "trials", "trials_launched", "segmented", "segment_length"):
        assert got[key] == want[key], (cfg, key, got[key], want[key])


def test_automatic_group_count_and_its_restore_after_an_every_iteration_run(recorded):
    want, got = recorded["auto_groups"], observe_auto_groups()
    assert len(got["timeline"]) == 2                # two groups from 128 instances
    assert len(got["timeline_last_tick"]) == 1      # a tick's solve runs one group unless the caller chose a number ...
    assert len(got["timeline_after_ticks"]) == 2    # ... and the run leaves the handle's own setting behind
    for key in ("timeline", "timeline_last_tick", "timeline_after_ticks"):
        assert got[key] == want[key], (key, got[key], want[key])


def _provenance(argv):
    """What a recording says about where it comes from: the commit git reports for the tree (a tree with changes gets "+dirty"), or, in a copy
    of the tree without its .git, the commit named after --record; and the sha256 of the library file that was loaded."""
    import hashlib
    import subprocess
    from live_ekf_slam_amd import _lib
    git = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True)
    if git.returncode == 0:
        dirty = subprocess.run(["git", "status", "--porcelain", "--untracked-files=no"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
        commit = git.stdout.strip() + ("+dirty" if dirty else "")
    elif len(argv) == 2:
        commit = argv[1] + " (as stated: no git checkout)"
    else:
        sys.exit("not a git checkout: name the commit the tree was copied from, --record COMMIT")
    with open(_lib.LIB_PATH, "rb") as f:
        return commit, hashlib.sha256(f.read()).hexdigest()


if __name__ == "__main__":
    if sys.argv[1:2] != ["--record"] or len(sys.argv) > 3:
        sys.exit("usage: python tests/test_pgs_schedule_gpu.py --record [COMMIT]   (writes tests/golden/pgs_schedule.json, see the docstring)")
    sys.path.insert(0, ROOT)
    commit, lib_sha = _provenance(sys.argv[1:])
    rec = dict(recorded_at=commit, library_sha256=lib_sha, scenario=dict(seed_map=9, L=L, T=T, KP=KP, B=B, seed=SEED, B_auto=B_AUTO, ticks=T_EVERY),
               configs={_key(c): observe_config(c) for c in CONFIGS}, auto_groups=observe_auto_groups())
    with open(FIXTURE, "w") as f:
        json.dump(rec, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes")
