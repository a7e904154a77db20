"""Not -m gpu: builds tools/tracking/session_plan_check.cc and tools/mapmaker/mapmaker_init_plan_check.cc with g++ under
AddressSanitizer and UndefinedBehaviorSanitizer and runs them directly.  Together they answer the whole table of a session's start:
stage x poke x n_good at min_good - 1 and min_good x init state x every init status (ptam_cg_amd/csrc/tracker_plan.h, against the
restatement of src/Tracker.cc:311-347 below), and the mapmaker's side — when a request is taken, when the step runs it, the flags
after every outcome (ptam_cg_amd/csrc/mapmaker_plan.h, src/MapMaker.cc:387-394 and :45-50)."""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOT_STARTED, STARTED, COMPLETE = range(3)
NONE, PENDING, DONE = range(3)
IDLE, START, RESET, KEEP, REQUEST, WAIT, BEGIN, INIT_FAILED, TRACK = range(9)
STATUSES = range(5)          # PTAM_INIT_MAP_OK, NO_HOMOGRAPHY, ZERO_BASELINE, TOO_FEW_POINTS, STOPPED
MIN_GOOD = 10


def build(tmp, source, name):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-I", os.path.join(ROOT, "ptam_cg_amd", "csrc"),
                           os.path.join(ROOT, "tools", source), "-o", exe])

    def run(*cases):
        path = str(tmp / (name + ".txt"))
        with open(path, "w") as f:
            for c in cases:
                f.write(" ".join(str(w) for w in c) + "\n")
        p = subprocess.run([exe, path], capture_output=True, text=True)
        assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr)
        lines = p.stdout.strip().split("\n")
        assert len(lines) == len(cases)
        return [[int(w) for w in ln.split()] for ln in lines]
    return run


@pytest.fixture(scope="module")
def session(tmp_path_factory):
    return build(tmp_path_factory.mktemp("session_plan"), os.path.join("tracking", "session_plan_check.cc"), "session_plan_check")


@pytest.fixture(scope="module")
def mapmaker(tmp_path_factory):
    return build(tmp_path_factory.mktemp("mapmaker_init_plan"), os.path.join("mapmaker", "mapmaker_init_plan_check.cc"), "mapmaker_init_plan_check")


def track_for_initial_map(stage, poke, n_good, init_state, init_status):
    """src/Tracker.cc:127 and :311-347, with the request's outcome where the reference has InitFromStereo's return value"""
    if stage == NOT_STARTED:                                         # :313-324
        return (START, 1) if poke else (IDLE, 0)
    if stage == STARTED:                                             # :326-346
        if n_good < MIN_GOOD:
            return RESET, int(poke)                                  # Reset() clears mbUserPressedSpacebar (:52)
        return (REQUEST, 1) if poke else (KEEP, 0)
    if init_state == NONE:                                           # the handle has no request out: mMap.IsGood() (:127)
        return TRACK, 0
    if init_state == PENDING:
        return WAIT, 0
    return (BEGIN if init_status == 0 else INIT_FAILED), 0


def test_the_whole_stage_table(session):
    cases, want = [], []
    for stage, poke, n_good, st, status in itertools.product((NOT_STARTED, STARTED, COMPLETE), (0, 1), (MIN_GOOD - 1, MIN_GOOD),
                                                             (NONE, PENDING, DONE), STATUSES):
        cases.append(("action", stage, poke, n_good, MIN_GOOD, st, status))
        want.append(list(track_for_initial_map(stage, poke, n_good, st, status)))
    got = session(*cases)
    assert got == want
    assert {g[0] for g in got} == set(range(9))                      # every action is reached
    # min_good 0: never a reset
    assert session(("action", STARTED, 0, 0, 0, NONE, 0), ("action", STARTED, 1, 0, 0, NONE, 0)) == [[KEEP, 0], [REQUEST, 1]]


def test_a_requests_clones_in_the_pool(session):
    FREE, OUT, IN_MAP = 0, 2, 3
    # four clones, 1 and 3 go out under tag 7; the tag comes back: they are the map's; a reset frees all four
    assert session(("pool", 4, 1, 3, 7)) == [[FREE, OUT, FREE, OUT, 2, FREE, IN_MAP, FREE, IN_MAP, 4]]


def test_the_mapmakers_side(mapmaker):
    got = mapmaker(*[("allowed", st, kf) for st in (NONE, PENDING, DONE) for kf in (0, 1)])
    assert got == [[1], [0], [0], [0], [1], [0]]                     # one at a time, and only for a map without a keyframe
    assert mapmaker(("want", NONE), ("want", PENDING), ("want", DONE)) == [[0], [1], [0]]
    cases = [("end",) + c for c in itertools.product((0, 1), repeat=5)]
    # a map was made: both converged (:387-394); none: Reset() (:45-50) — nothing runs, no abort is pending, either way
    assert mapmaker(*cases) == [[1, 1, 0, 0]] * len(cases)
