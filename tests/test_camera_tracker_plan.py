"""Not -m gpu: builds tools/tracking/tracker_plan_check.cc with g++ under AddressSanitizer and UndefinedBehaviorSanitizer and asks
ptam_cg_amd/csrc/tracker_plan.h the whole table of what the tracker's thread decides behind a frame (src/Tracker.cc:146-166): branch x
quality x (frame - last dropped) at gap and gap + 1 x queue at max_queue - 1 and max_queue x records 0 or > 0 -> add / note / neither
and mnLastKeyFrameDropped afterwards; and walks the pools: take, hand over, release in any order, a clone that entered the map,
exhaustion, reset.  The program is run directly."""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEITHER, ADD, NOTE = 0, 1, 2
TRACKED, RECOVERED, FAILED = 0, 1, 2
BAD, GOOD = 0, 1


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("tracker_plan_check")
    exe = str(d / "tracker_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-I", os.path.join(ROOT, "ptam_cg_amd", "csrc"),
                           os.path.join(ROOT, "tools", "tracking", "tracker_plan_check.cc"), "-o", exe])

    def run(*cases):
        path = str(d / "cases.txt")
        with open(path, "w") as f:
            for c in cases:
                f.write(" ".join(str(w) for w in c) + "\n")
        p = subprocess.run([exe, path], capture_output=True, text=True)
        assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr)
        lines = p.stdout.strip().split("\n")
        assert len(lines) == len(cases)
        return [[int(w) for w in ln.split()] for ln in lines]
    return run


def decide(branch, quality, frame, last, gap, queue, max_queue, records):
    """src/Tracker.cc:146-166 restated: isTrackGood && isFarEnough && isQueueNeed on the tracking branch (isNeedFrame is commented out
    there); a frame that found nothing hands nothing over; a tracked or recovered frame that found points is noted otherwise"""
    if branch == FAILED or records == 0:
        return NEITHER, last
    if branch == TRACKED and quality == GOOD and frame - last > gap and queue < max_queue:
        return ADD, frame
    return NOTE, last


def test_the_whole_decision_table(ask):
    cases, want = [], []
    for gap, max_queue in ((20, 3), (1, 3), (0, 1)):
        for branch, quality, far, queue, records, frame in itertools.product((TRACKED, RECOVERED, FAILED), (BAD, GOOD), (gap, gap + 1),
                                                                             (max_queue - 1, max_queue), (0, 37), (5, 1000)):
            last = frame - far
            cases.append(("decide", branch, quality, frame, last, gap, queue, max_queue, records))
            want.append(list(decide(branch, quality, frame, last, gap, queue, max_queue, records)))
    got = ask(*cases)
    assert got == want
    assert {w[0] for w in want} == {NEITHER, ADD, NOTE}
    # the reference's numbers: the first frame after a reset (last = -20) adds at once; 20 frames after an add it does not, 21 after it does
    assert ask(("decide", TRACKED, GOOD, 1, -20, 20, 0, 3, 50), ("decide", TRACKED, GOOD, 40, 20, 20, 0, 3, 50),
               ("decide", TRACKED, GOOD, 41, 20, 20, 0, 3, 50), ("decide", TRACKED, GOOD, 41, 20, 20, 3, 3, 50)) == \
        [[ADD, 1], [NOTE, 20], [ADD, 41], [NOTE, 20]]


def test_a_clone_is_needed_only_where_the_frame_could_add(ask):
    cases = [("mayadd", lost, frame, last, gap) for lost in (0, 2, 3) for frame in (0, 19, 20, 21) for last in (-20, 0, 1) for gap in (20, 1)]
    assert ask(*cases) == [[int(lost < 3 and frame + 1 - last > gap)] for _, lost, frame, last, gap in cases]


def test_the_pools(ask):
    got = ask(("pool", 3, 2),
              ("hold",), ("add", 0, 100),            # frame 100: report 0 and clone 0 go out
              ("hold",), ("note", 1, 101),           # frame 101: report 1 goes out
              ("hold",), ("back", 2),                # frame 102 hands nothing over: its report is free again at once
              ("hold",), ("add", 2, 103),            # frame 103: report 2, clone 1
              ("hold",),                             # no report is free
              ("release", 101),                      # in any order: the note first
              ("hold",), ("add", 1, 104),            # report 1 again — and no clone is free: nothing is handed over
              ("back", 1),
              ("release", 103), ("release", 100),    # the keyframes entered the map: their reports are free, their clones stay
              ("release", 555),                      # not ours
              ("release", 100),                      # ... and a tag comes back once
              ("hold",), ("add", 0, 105),            # still no clone
              ("reset",))
    assert got == [[3, 2],
                   [0], [0],
                   [1], [-1],
                   [2], [1, 1],
                   [2], [1],
                   [-1],
                   [1, 1, 0, 0],
                   [1], [-1],
                   [1, 0],
                   [2, 2, 0, 1], [2, 3, 0, 2],
                   [0, 3, 0, 2],
                   [0, 3, 0, 2],
                   [0], [-1],
                   [3, 2]]
