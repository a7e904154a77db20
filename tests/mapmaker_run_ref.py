"""The body of MapMaker::run() (src/MapMaker.cc:86-112) written out in Python over the calls a host composed it from before
ptam_mapmaker_step: host.ResidentMap.bundle_adjust + apply_outliers, refind(work=None), note_reports, handle_bad_points,
InsertKeyFrame(report=...), publish, clear — with the flags of :790-793, :895-913, :516-517, :37-51 and the draw restated here.
RefMapMaker has host.MapMaker's methods and its Step returns the same dict, so a test runs both side by side on two maps."""
import numpy as np

from ptam_cg_amd import _abi, host

M64 = (1 << 64) - 1
BA_COUNTS = tuple(f for f, _ in _abi.MapBaResult._fields_)
ZERO = {"recent": _abi.MapBaResult, "recent_outliers": _abi.MapOutliersResult, "refind_new": _abi.MapRefindResult, "all": _abi.MapBaResult,
        "all_outliers": _abi.MapOutliersResult, "refind_failure": _abi.MapRefindResult, "notes": _abi.RmapNoteResult,
        "bad_points": _abi.MapBadPointsResult}


def splitmix64(seed, n):
    z = (seed + (n + 1) * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


class RefMapMaker:
    def __init__(self, rmap, finder, snapshot=None, failure_period=20, failure_seed=0, max_pairs_per_pass=0, ba=None, **epipolar):
        self.m, self.finder, self.snapshot = rmap, finder, snapshot
        self.period, self.seed, self.per_pass, self.ba, self.epipolar = failure_period, failure_seed, max_pairs_per_pass, dict(ba or {}), epipolar
        self.queue, self.notes, self._released = [], [], []
        self.recent = self.full = True                                # Reset() (:46-47)
        self.draws = 0
        self.reset_requested, self.reset_done = False, True

    # ---- the tracker's side
    def AddKeyFrame(self, kf, pose, fixed, report, depth_mean, depth_sigma, tag, rest_made=True):
        self.queue.append(dict(kf=kf, pose=np.array(pose, np.float64), fixed=fixed, report=report, depth=(depth_mean, depth_sigma), tag=tag,
                               rest_made=rest_made))

    def NoteFrame(self, report, tag):
        self.notes.append((report, tag))

    def QueueSize(self):
        return len(self.queue)

    def RequestReset(self):
        self.reset_done, self.reset_requested = False, True

    def ResetDone(self):
        return self.reset_done

    def flags(self):
        return dict(converged_recent=int(self.recent), converged_full=int(self.full), bundle_running=0)

    def set_flags(self, converged_recent, converged_full):
        self.recent, self.full = bool(converged_recent), bool(converged_full)

    def released(self):
        out, self._released = self._released, []
        return out

    # ---- the loop's body
    def _bundle(self, recent):
        m = self.m
        ba = m.bundle_adjust(_abi.MAP_BA_RECENT if recent else _abi.MAP_BA_ALL, **self.ba)
        out = m.apply_outliers(ba["outliers"])
        if ba["accepted"] > 0:                                        # :895-904
            if recent:
                self.recent = False
            self.full = False
        if ba["converged"]:                                           # :906-910
            self.recent = True
            if not recent:
                self.full = True
        return {k: ba[k] for k in BA_COUNTS}, out

    def _end(self, d, status):
        d.update(status=status, converged_recent=int(self.recent), converged_full=int(self.full), queue_size=len(self.queue), draws=self.draws)
        return d

    def Step(self):
        m = self.m
        d = {k: host._counts(t()) for k, t in ZERO.items()}
        d.update(stages=0, insert=dict(kf=0, target_kf=0, target_dist=0.0, refind=host._counts(_abi.MapRefindResult()), first_point=0, n_made=0,
                                       n_rows=0, n_gone=0), publish=dict(generation=0, map_id=0, n_points=0, n_kf=0, grew=0))
        if self.reset_requested:                                      # CHECK_RESET (one thread here: the request precedes the step)
            m.clear()
            self._released += [k["tag"] for k in self.queue] + [t for _, t in self.notes]
            self.queue, self.notes = [], []
            self.recent = self.full = True
            self.reset_done, self.reset_requested = True, False
            return self._end(d, _abi.MM_RESET)
        if m.counts()["n_kf"] == 0:                                   # :79
            return self._end(d, _abi.MM_IDLE)
        changed = False
        if not self.recent and not self.queue:                        # :88
            if m.counts()["n_kf"] < 8:                                # :790-793
                self.recent = True
            else:
                d["recent"], d["recent_outliers"] = self._bundle(True)
                d["stages"] |= _abi.MM_STAGE_BUNDLE_RECENT
                changed |= d["recent"]["accepted"] > 0
        if self.recent and not self.queue:                            # :93
            d["refind_new"] = m.refind(self.finder, _abi.MAP_REFIND_NEW_POINTS, stop=np.zeros(1, np.uint8), max_pairs_per_pass=self.per_pass,
                                       lists=False)
            d["stages"] |= _abi.MM_STAGE_REFIND_NEW
        if self.recent and not self.full and not self.queue:          # :98
            d["all"], d["all_outliers"] = self._bundle(False)
            d["stages"] |= _abi.MM_STAGE_BUNDLE_ALL
            changed |= d["all"]["accepted"] > 0
        if self.recent and self.full:                                 # :103: rand() is called behind the two flags
            hit = splitmix64(self.seed, self.draws) % self.period == 0
            self.draws += 1
            if hit and not self.queue:
                d["refind_failure"] = m.refind(self.finder, _abi.MAP_REFIND_FAILURE_QUEUE, max_pairs_per_pass=self.per_pass, lists=False)
                d["stages"] |= _abi.MM_STAGE_REFIND_FAILURE
        if self.notes:                                                # the tracked frames' counts, before :107
            d["notes"] = m.note_reports([r for r, _ in self.notes])
            self._released += [t for _, t in self.notes]
            self.notes = []
            d["stages"] |= _abi.MM_STAGE_NOTES
        d["bad_points"] = m.handle_bad_points()                       # :107
        d["stages"] |= _abi.MM_STAGE_BAD_POINTS
        changed |= d["bad_points"]["n_removed"] > 0
        if self.queue:                                                # :111-112
            k = self.queue.pop(0)
            if not k["rest_made"]:
                k["kf"].MakeKeyFrame_Rest()                           # :500
            o = m.insert_opts(max_pairs_per_pass=self.per_pass, depth_mean=k["depth"][0], depth_sigma=k["depth"][1],
                              **dict(dict(levels=(3, 0, 1, 2)), **self.epipolar))
            r = m.InsertKeyFrame(self.finder, k["kf"], k["pose"], k["fixed"], opts=o, report=k["report"])
            self._released.append(k["tag"])
            d["insert"] = {f: r[f] for f in d["insert"]}
            self.recent = self.full = False                           # :516-517
            d["stages"] |= _abi.MM_STAGE_ADD_KEYFRAME
            changed = True
        if self.snapshot is not None and changed:
            r = m.publish(self.snapshot)
            d["publish"] = {f: r[f] for f in d["publish"]}
            d["stages"] |= _abi.MM_STAGE_PUBLISH
        return self._end(d, _abi.MM_RAN)
