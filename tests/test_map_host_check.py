"""Not -m gpu: builds tools/mapmaker/map_host_check.cc with g++ under AddressSanitizer and UndefinedBehaviorSanitizer (the line in its
head comment) and runs it on small cases: the re-find planning of ptam_cg_amd/csrc/maprefind_plan.h against numpy and
tests/map_refind_ref.pairs_for, the queue walk of a stopped ReFindNewlyMade against src/MapMaker.cc:1053-1059 restated here, and one
refusing and one passing input for every rule of map_tables_check.h.  The program is run directly; nothing is preloaded."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from ptam_cg_amd import _abi
from tests import map_refind_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYFRAME, NEW_POINTS, QUEUE = _abi.MAP_REFIND_KEYFRAME, _abi.MAP_REFIND_NEW_POINTS, _abi.MAP_REFIND_FAILURE_QUEUE
K, N = 3, 9                                                    # 3 keyframes, 9 points
NEW = np.array([7, 2, 5, 0, 8], np.int32)                      # a new-points list of 5 ...
BAD_POINTS = (2, 8)                                            # ... with 2 bad
FAILURE = [(2, 4), (0, 7), (1, 1), (2, 4), (0, 3), (0, 7)]     # a failure queue of 6 with two duplicates


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("map_host_check")
    exe = str(d / "map_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-I", os.path.join(ROOT, "ptam_cg_amd", "csrc"),
                           os.path.join(ROOT, "tools", "mapmaker", "map_host_check.cc"), "-o", exe])

    def run(*cases):
        """cases: sequences of words -> one list of output words per case; the sanitizers must have nothing to say"""
        path = str(d / "cases.txt")
        with open(path, "w") as f:
            for c in cases:
                f.write(" ".join(str(int(w)) if not isinstance(w, str) else w for w in c) + "\n")
        p = subprocess.run([exe, path], capture_output=True, text=True)
        assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr)
        lines = p.stdout.strip().split("\n")
        assert len(lines) == len(cases)
        return [ln.split() for ln in lines]
    return run


def flat(pairs):
    return [w for p in pairs for w in p]


def sections(words):
    """"plan 1 pairs bound per_pass consumed bad | wpts | wentry | wrank | wq" -> (the five numbers, four lists of ints)"""
    assert words[:2] == ["plan", "1"], words
    parts, cur = [], []
    for w in words[2:]:
        if w == "|":
            parts.append(cur)
            cur = []
        else:
            cur.append(int(w))
    parts.append(cur)
    assert len(parts) == 5
    return parts[0], parts[1:]


def points_table():
    pts = np.zeros(N, F.POINT_DT)
    pts["bad"][list(BAD_POINTS)] = 1
    return pts


EMPTY_MEAS, EMPTY_NEVER = np.zeros(0, F.MEAS_DT), np.zeros(0, F.PAIR_DT)


def test_plan_of_each_mode_matches_the_visiting_order(check):
    pts = points_table()
    fq = np.zeros(len(FAILURE), F.PAIR_DT)
    fq["kf"], fq["point"] = [k for k, _ in FAILURE], [p for _, p in FAILURE]
    out = check(["plan", KEYFRAME, K, N, 0, 1, 1],
                ["plan", NEW_POINTS, K, N, 0, len(NEW)] + NEW.tolist() + pts["bad"][NEW].tolist(),
                ["plan", QUEUE, K, N, 0, len(FAILURE)] + flat(FAILURE))
    # KEYFRAME: every point of the table once, bBad not looked at
    kf, pt, _, n_bad = F.pairs_for(KEYFRAME, K, pts, EMPTY_MEAS, EMPTY_NEVER, np.array([1], np.int32))
    (pairs, bound, per_pass, consumed, bad), (wpts, wentry, wrank, wq) = sections(out[0])
    assert (pairs, bound, per_pass, consumed, bad) == (len(kf), N, N, 0, 0) and n_bad == 0 and not (wpts or wentry or wrank or wq)
    # NEW_POINTS: the points that make pairs in queue order, their queue entries, their places in index order
    kf, pt, _, n_bad = F.pairs_for(NEW_POINTS, K, pts, EMPTY_MEAS, EMPTY_NEVER, NEW)
    (pairs, bound, per_pass, consumed, bad), (wpts, wentry, wrank, wq) = sections(out[1])
    good = pt[::K].tolist()
    assert np.array_equal(kf, np.tile(np.arange(K), len(good))) and np.array_equal(pt, np.repeat(good, K))
    assert good == [7, 5, 0] and n_bad == 2
    assert wpts == good and wentry == [int(np.flatnonzero(NEW == p)[0]) for p in good]
    assert wrank == np.argsort(np.argsort(good)).tolist() and not wq
    assert (pairs, bound, consumed, bad) == (len(kf), K * len(NEW), len(NEW), n_bad)
    assert per_pass == pairs                                   # the default pass holds the call; whole points either way
    # FAILURE_QUEUE: sorted, duplicates kept (the kernel skips a pair equal to its predecessor)
    kf, pt, _, _ = F.pairs_for(QUEUE, K, pts, EMPTY_MEAS, EMPTY_NEVER, fq)
    (pairs, bound, per_pass, consumed, bad), (wpts, wentry, wrank, wq) = sections(out[2])
    assert wq == flat(zip(kf.tolist(), pt.tolist())) and wq == flat(sorted(FAILURE)) and not (wpts or wentry or wrank)
    assert (pairs, bound, per_pass, consumed, bad) == (len(FAILURE), len(FAILURE), len(FAILURE), 0, 0)


def queue_walk(queue, bad, stop_after_good):
    """src/MapMaker.cc:1053-1059 restated: the loop pops the front while the flag (mvpKeyFrameQueue not empty) is down; the flag
    goes up while good point number `stop_after_good` is being re-found -> (entries popped, nBad)"""
    q, popped, n_bad, good = list(queue), 0, 0, 0
    while q and good < stop_after_good:                        # :1053 (the flag is looked at before each pop)
        p = q.pop(0)                                           # :1054-1055
        popped += 1
        if bad[p]:                                             # :1056-1059
            n_bad += 1
            continue
        good += 1                                              # :1060-1063: the point is re-found in every keyframe
    return popped, n_bad


def test_a_stop_after_every_whole_point(check):
    pts = points_table()
    plan = ["plan", NEW_POINTS, K, N, K, len(NEW)] + NEW.tolist() + pts["bad"][NEW].tolist()   # a pass of one point
    n_good = len(NEW) - len(BAD_POINTS)
    out = check(plan, *[["stop", g * K] for g in range(n_good + 1)])
    (pairs, _, per_pass, _, _), _ = sections(out[0])
    assert per_pass == K and pairs == n_good * K
    for g in range(n_good + 1):
        assert [int(w) for w in out[1 + g][1:]] == list(queue_walk(NEW.tolist(), pts["bad"], g)), g
    assert [int(w) for w in out[1][1:]] == [0, 0] and [int(w) for w in out[2][1:]] == [1, 0] and [int(w) for w in out[3][1:]] == [3, 1]


def test_plan_refuses_bad_work(check):
    out = check(["plan", NEW_POINTS, K, N, 0, 2, 4, 4, 0, 0],                     # a point twice
                ["plan", NEW_POINTS, K, N, 0, 1, N, 0],                           # out of range
                ["plan", KEYFRAME, K, N, 0, 1, K],                                # no such keyframe
                ["plan", KEYFRAME, K, N, 0, 2, 0, 1],                             # two keyframes
                ["plan", QUEUE, K, N, 0, 1, K, 0],                                # a pair's keyframe out of range
                ["plan", QUEUE, K, N, 0, 1, 0, -1],
                ["plan", KEYFRAME, K, N, 0, 0], ["plan", NEW_POINTS, K, N, 0, 0], ["plan", QUEUE, K, N, 0, 0])   # no work is fine
    assert [w[1] for w in out] == ["0"] * 6 + ["1"] * 3
    assert all(sections(w)[0][0] == 0 for w in out[6:])


def test_every_table_rule_refuses_and_passes(check):
    ok_pairs = [(0, 1), (0, 8), (1, 0), (2, 3)]
    meas = lambda rows: ["meas", K, N, len(rows)] + flat(rows)
    outl = lambda host, o: (["outliers", host, len(ok_pairs)] + flat(ok_pairs) + [1, 1, 0, 2, len(o)] + flat(o))   # never = {(1, 0)}, 2 failure pairs
    cases = [
        (["sorted", K, N, 4] + flat(ok_pairs), ["1"]),
        (["sorted", K, N, 4] + flat([(0, 1), (0, 1), (1, 0), (2, 3)]), ["0"]),                    # a pair twice
        (["sorted", K, N, 4] + flat([(0, 8), (0, 1), (1, 0), (2, 3)]), ["0"]),                    # out of order
        (["sorted", K, N, 1, K, 0], ["0"]),
        (["sorted", K, N, 0], ["1"]),
        (meas([(0, 1, 0, 0), (1, 2, 3, 4)]), ["1"]),
        (meas([(0, 1, 4, 0)]), ["0"]), (meas([(0, 1, 0, 5)]), ["0"]), (meas([(0, 1, -1, 0)]), ["0"]), (meas([(1, 0, 0, 0), (0, 0, 0, 0)]), ["0"]),
        (["pairs", K, N, 3] + flat([(2, 8), (0, 0), (2, 8)]), ["1"]),                             # any order, duplicates allowed
        (["pairs", K, N, 1, 0, N], ["0"]), (["pairs", K, N, 1, -1, 0], ["0"]),
        (["queue", N, 3, 8, 0, 4], ["1"]), (["queue", N, 3, 8, 0, 8], ["0"]), (["queue", N, 1, N], ["0"]), (["queue", N, 1, -1], ["0"]),
        (["kf_rows", N, 3] + flat([(0, 0), (4, 3), (8, 1)]), ["1"]),
        (["kf_rows", N, 2] + flat([(4, 0), (4, 1)]), ["0"]), (["kf_rows", N, 2] + flat([(5, 0), (4, 1)]), ["0"]),
        (["kf_rows", N, 1, N, 0], ["0"]), (["kf_rows", N, 1, 0, 4], ["0"]),
        (["sources", K, 2] + flat([(0, 0), (2, 3)]), ["1"]), (["sources", K, 1, K, 0], ["0"]), (["sources", K, 1, 0, 4], ["0"]),
        # the outlier list against 4 rows, 1 never pair, 2 failure pairs
        (outl(1, [(0, 1, 0, _abi.OUT_POINT_BAD), (0, 8, 1, _abi.OUT_FAILURE_QUEUE), (2, 3, 3, _abi.OUT_NEVER_RETRY)]),
         ["-1", "1", "1", "1", "2", "2", "3"]),
        (outl(1, [(0, 1, 0, _abi.OUT_POINT_BAD), (0, 1, 0, _abi.OUT_FAILURE_QUEUE)]), ["1"]),     # a row named twice
        (outl(1, [(0, 8, 0, _abi.OUT_POINT_BAD)]), ["0"]),                                           # not its row
        (outl(1, [(0, 1, 0, _abi.OUT_POINT_BAD), (1, 0, 2, _abi.OUT_NEVER_RETRY)]), ["1"]),       # in never already
        (outl(1, [(0, 1, 4, _abi.OUT_POINT_BAD)]), ["0"]), (outl(1, [(0, 1, 0, 4)]), ["0"]), (outl(1, [(0, 1, 0, 0)]), ["0"]),
        # a resident map's list: only what the list alone decides (the kernels look at the tables)
        (outl(0, [(0, 8, 0, _abi.OUT_POINT_BAD), (1, 0, 2, _abi.OUT_NEVER_RETRY)]), ["-1", "1", "0", "1", "3", "2", "2"]),
        (outl(0, [(0, 1, 4, _abi.OUT_POINT_BAD)]), ["0"]),
    ]
    out = check(*[c for c, _ in cases])
    for (c, want), got in zip(cases, out):
        assert got[0] == c[0] and got[1:1 + len(want)] == want, (c, got)
