"""CPU: the two forms of tests/map_publish_ref.py — point objects with a dict from object to finder, and the serial column with
searchsorted — agree on seeded edit histories: every take's counts, prev and finder identities, every resolve, and the one-to-one
correspondence of point objects and (map_id, serial) throughout."""
import numpy as np
import pytest

from tests import map_publish_ref as P


def run(ops):
    """both forms through one history -> what was compared: (takes with changed, takes without, resolves, publishes between takes)"""
    omaps, nmaps = [P.ObjMap(), P.ObjMap()], [P.NpMap(), P.NpMap()]
    osnap, nsnap, otr, ntr = P.ObjSnapshot(), P.NpSnapshot(), P.ObjTracker(), P.NpTracker()
    name = {}                                   # point object -> (map_id, serial): fixed for the object's life, never shared
    ever = [[], []]                             # every (object, serial) a map has held
    stats = dict(changed=0, unchanged=0, resolves=0, between=[], carried=0)
    since = 0

    def correspond(m):
        assert len(omaps[m].points) == len(nmaps[m].serials)
        assert np.all(np.diff(nmaps[m].serials) > 0)                        # strictly increasing with the index
        for p, s in zip(omaps[m].points, nmaps[m].serials.tolist()):
            key = (nmaps[m].map_id, s)
            if p not in name:
                name[p] = key
                ever[m].append((p, s))
            assert name[p] == key
        assert len(set(name.values())) == len(name)                         # no serial is ever given twice

    for op in ops:
        kind = op[0]
        if kind in ("upload", "append"):
            for maps in (omaps, nmaps):
                getattr(maps[op[1]], kind)(op[2])
            correspond(op[1])
        elif kind == "remove":
            keep = P.keep_flags(len(omaps[op[1]].points), op[2], op[3])
            omaps[op[1]].remove(keep)
            nmaps[op[1]].remove(keep)
            correspond(op[1])
        elif kind == "publish":
            assert osnap.publish(omaps[op[1]]) == nsnap.publish(nmaps[op[1]])
            since += 1
        elif kind == "set_map":
            otr.set_map(op[1])
            ntr.set_map(op[1])
        elif kind == "take":
            a, b = otr.take(osnap), ntr.take(nsnap)
            assert a == b, (a, b)
            if a["changed"]:
                stats["changed"] += 1
                stats["carried"] += a["n_carried"]
                stats["between"].append(since)
                assert sorted(x for x in a["prev"] if x >= 0) == [x for x in a["prev"] if x >= 0]      # no old index twice, in order
                assert ntr.serials.tolist() == [name[p][1] for p in otr.points]
            else:
                stats["unchanged"] += 1
            since = 0
        elif kind == "resolve":
            m, rng = op[1], np.random.default_rng(op[2])
            pool = ever[m]
            pick = [pool[i] for i in rng.permutation(len(pool))[:40]]
            want = omaps[m].resolve([p for p, _ in pick])
            got = nmaps[m].resolve(np.array([s for _, s in pick], np.int64))
            assert got.tolist() == want
            never = np.array([0, -5, nmaps[m].next_serial, nmaps[m].next_serial + 7], np.int64)     # values never given out
            assert nmaps[m].resolve(never).tolist() == [-1] * 4
            stats["resolves"] += 1
    return stats


@pytest.mark.parametrize("seed", range(20))
def test_the_two_forms_agree_on_a_seeded_history(seed):
    st = run(P.history(seed))
    assert st["changed"] >= 6 and st["unchanged"] >= 1 and st["resolves"] >= 1 and st["carried"] > 0
    assert 2 in st["between"] and 3 in st["between"]      # two and three publishes between takes


def test_a_reupload_and_a_second_map_carry_nothing():
    for second in (False, True):
        omaps, nmaps = [P.ObjMap(), P.ObjMap()], [P.NpMap(), P.NpMap()]
        osnap, nsnap, otr, ntr = P.ObjSnapshot(), P.NpSnapshot(), P.ObjTracker(), P.NpTracker()
        for maps in (omaps, nmaps):
            maps[0].upload(10)
        osnap.publish(omaps[0]), nsnap.publish(nmaps[0])
        assert otr.take(osnap) == ntr.take(nsnap)
        for maps in (omaps, nmaps):
            maps[int(second)].upload(10)                  # the same count again: new objects, fresh serials
        osnap.publish(omaps[int(second)]), nsnap.publish(nmaps[int(second)])
        a, b = otr.take(osnap), ntr.take(nsnap)
        assert a == b and a["n_carried"] == 0 and a["n_new"] == 10 and a["n_dropped"] == 10 and a["prev"] == [-1] * 10


def test_find_sorted_at_the_edges():
    col = np.array([3, 4, 9, 20], np.int64)
    assert P.find_sorted(col, [3, 20, 2, 21, 5, 9]).tolist() == [0, 3, -1, -1, -1, 2]
    assert P.find_sorted(np.zeros(0, np.int64), [1, 2]).tolist() == [-1, -1]
    assert P.find_sorted(col, np.zeros(0, np.int64)).tolist() == []
    assert P.prev_of(col, 1, col, 2).tolist() == [-1] * 4 and P.prev_of(col, 1, None, 1).tolist() == [-1] * 4
    assert P.prev_of(col[1:], 1, col, 1).tolist() == [1, 2, 3]
