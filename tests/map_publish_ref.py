"""The hand-over of the map from the mapmaker to the tracker (ptam_rmap_publish / ptam_tracker_take_map / ptam_rmap_resolve_serials),
twice on the CPU.

The literal form says what the calls mean with Python objects: a map point is an object, the map a list of them, a snapshot a copy
of that list, and the tracker keeps a dict from point object to its PatchFinder — `TrackerData` lives as long as the `MapPoint`
(include/Tracker.h:42-67).  Nothing in it has a number.

The vectorised form is what the device does: a serial column (int64, strictly increasing with the index, from a running counter that
is never reused), a map_id per handle, `searchsorted` of the new serials in the tracker's old list for prev, `searchsorted` in the
column for resolve.  tests/test_map_publish_ref.py runs both through the same seeded edit histories."""
import itertools

import numpy as np


# ---- the literal form --------------------------------------------------------------------------------------------------------------
class Point:
    """a MapPoint: its identity is the object (hashed and compared as such)"""
    __slots__ = ()


class ObjMap:
    """Map::vpPoints.  Points are appended at the end and removed in place; an upload replaces every object."""

    def __init__(self):
        self.points = []

    def upload(self, n):
        self.points = [Point() for _ in range(n)]

    def append(self, n):
        self.points += [Point() for _ in range(n)]

    def remove(self, keep):
        """keep: one flag per point (Map::MoveBadPointsToTrash keeps the survivors' order)"""
        assert len(keep) == len(self.points)
        self.points = [p for p, k in zip(self.points, keep) if k]

    def resolve(self, points):
        """the current index of each point object, -1 for one that is no longer in the map"""
        where = {p: i for i, p in enumerate(self.points)}
        return [where.get(p, -1) for p in points]


class ObjSnapshot:
    """what the tracker is handed: the list as it stood at the publish"""

    def __init__(self):
        self.points, self.generation = None, 0

    def publish(self, m):
        self.points, self.generation = list(m.points), self.generation + 1
        return self.generation


class ObjTracker:
    """the tracker's map and, per point object, its PatchFinder (a token that is new whenever the finder is)"""

    def __init__(self):
        self.points, self.finder, self.last = [], {}, None
        self._tokens = itertools.count()

    def set_map(self, n):
        """ptam_tracker_set_map: points the mapmaker does not know as objects — every finder is new"""
        self.points = [Point() for _ in range(n)]
        self.finder = {p: next(self._tokens) for p in self.points}
        self.last = None

    def take(self, snap):
        """-> dict(changed, generation, n_points, n_carried, n_new, n_dropped, prev, finders)"""
        assert snap.points is not None, "never published into"
        if self.last == (snap, snap.generation):
            return dict(changed=0, generation=snap.generation, n_points=len(self.points))
        old_index = {p: i for i, p in enumerate(self.points)}
        prev = [old_index.get(p, -1) for p in snap.points]
        carried = sum(1 for x in prev if x >= 0)
        finder = {p: (self.finder[p] if p in old_index else next(self._tokens)) for p in snap.points}
        out = dict(changed=1, generation=snap.generation, n_points=len(snap.points), n_carried=carried, n_new=len(prev) - carried,
                   n_dropped=len(self.points) - carried, prev=prev)
        self.points, self.finder, self.last = list(snap.points), finder, (snap, snap.generation)
        out["finders"] = [finder[p] for p in self.points]
        return out


# ---- the vectorised form ------------------------------------------------------------------------------------------------------------
_map_ids = itertools.count(1)


class NpMap:
    """the serial column of a ptam_rmap"""

    def __init__(self):
        self.map_id, self.next_serial = next(_map_ids), 1
        self.serials = np.zeros(0, np.int64)

    def _fresh(self, n):
        s = np.arange(self.next_serial, self.next_serial + n, dtype=np.int64)
        self.next_serial += n
        return s

    def upload(self, n):
        self.serials = self._fresh(n)

    def append(self, n):
        self.serials = np.concatenate([self.serials, self._fresh(n)])

    def remove(self, keep):
        self.serials = self.serials[np.asarray(keep, bool)]

    def resolve(self, serials):
        return resolve(self.serials, serials)


def find_sorted(column, keys):
    """index of each key in the strictly increasing column, -1 where it is not there"""
    column, keys = np.asarray(column, np.int64), np.asarray(keys, np.int64)
    at = np.searchsorted(column, keys)
    hit = (at < len(column)) & (column[np.minimum(at, max(len(column) - 1, 0))] == keys if len(column) else np.zeros(len(keys), bool))
    return np.where(hit, at, -1).astype(np.int32)


def resolve(column, serials):
    return find_sorted(column, serials)


def prev_of(new_serials, new_map_id, old_serials, old_map_id):
    """prev[i] of ptam_tracker_take_map: -1 for all when the maps differ or the tracker has no list (old_serials None)"""
    if old_serials is None or old_map_id != new_map_id:
        return np.full(len(new_serials), -1, np.int32)
    return find_sorted(old_serials, new_serials)


class NpSnapshot:
    _uids = itertools.count(1)

    def __init__(self):
        self.uid, self.generation, self.serials, self.map_id = next(self._uids), 0, None, 0

    def publish(self, m):
        self.serials, self.map_id, self.generation = m.serials.copy(), m.map_id, self.generation + 1
        return self.generation


class NpTracker:
    def __init__(self):
        self.n, self.serials, self.map_id, self.last = 0, None, 0, None
        self.finder = np.zeros(0, np.int64)
        self._tokens = itertools.count()

    def _new_finders(self, n):
        return np.array([next(self._tokens) for _ in range(n)], np.int64)

    def set_map(self, n):
        self.n, self.serials, self.map_id, self.last = n, None, 0, None
        self.finder = self._new_finders(n)

    def take(self, snap):
        assert snap.serials is not None, "never published into"
        if self.last == (snap.uid, snap.generation):
            return dict(changed=0, generation=snap.generation, n_points=self.n)
        prev = prev_of(snap.serials, snap.map_id, self.serials, self.map_id)
        carried = int((prev >= 0).sum())
        finder = np.zeros(len(prev), np.int64)
        for i, p in enumerate(prev):                # (in index order, as the literal form hands out its tokens)
            finder[i] = self.finder[p] if p >= 0 else next(self._tokens)
        out = dict(changed=1, generation=snap.generation, n_points=len(prev), n_carried=carried, n_new=len(prev) - carried,
                   n_dropped=self.n - carried, prev=prev.tolist(), finders=finder.tolist())
        self.n, self.serials, self.map_id, self.finder, self.last = len(prev), snap.serials.copy(), snap.map_id, finder, (snap.uid, snap.generation)
        return out


# ---- seeded edit histories ------------------------------------------------------------------------------------------------------------
def history(seed, steps=40):
    """a list of operations on two maps (0, 1), one snapshot and one tracker: ("upload", m, n), ("append", m, n), ("remove", m, keep
    share, seed), ("publish", m), ("take",), ("set_map", n), ("resolve", m, seed).  Every history holds two and three publishes between
    takes, a re-upload, and a take from the second map."""
    rng = np.random.default_rng(seed)
    ops = [("upload", 0, int(rng.integers(20, 70))), ("publish", 0), ("take",), ("take",)]
    fixed = [[("publish", 0), ("take",), ("remove", 0, 0.7, 1), ("publish", 0), ("append", 0, 5), ("publish", 0), ("take",)],
             [("publish", 0), ("take",), ("publish", 0), ("remove", 0, 0.5, 2), ("publish", 0), ("append", 0, 9), ("publish", 0), ("take",), ("resolve", 0, 3)],
             [("upload", 0, int(rng.integers(1, 70))), ("publish", 0), ("take",)],
             [("upload", 1, int(rng.integers(1, 70))), ("publish", 1), ("take",), ("publish", 0), ("take",)],
             [("set_map", int(rng.integers(0, 30))), ("take",)]]
    for k in rng.permutation(len(fixed)):
        ops += fixed[k]
        for _ in range(int(rng.integers(0, steps // 5))):
            kind = rng.choice(["append", "remove", "publish", "take", "resolve"])
            m = int(rng.integers(0, 2)) if any(o[0] == "upload" and o[1] == 1 for o in ops) else 0
            ops.append({"append": ("append", m, int(rng.integers(0, 12))), "remove": ("remove", m, float(rng.choice([0.0, 0.5, 0.9, 1.0])), int(rng.integers(1 << 30))),
                        "publish": ("publish", m), "take": ("take",), "resolve": ("resolve", m, int(rng.integers(1 << 30)))}[str(kind)])
    return ops


def keep_flags(n, share, seed):
    return np.random.default_rng(seed).random(n) < share
