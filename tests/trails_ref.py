"""Tracker::TrailTracking_Start / TrailTracking_Advance (src/Tracker.cc:352-432), MiniPatch::FindPatch and SSDAtPoint
(src/ImageProcess.cc:57-80, 196-252), the match table of MapMaker::InitFromStereo (src/MapMaker.cc:272-279) and its point loop
(:310-367), restated in numpy / plain Python floats from the reference, statement by statement — the checker of ptam_trails_* and
ptam_init_points_from_trails.  The sub-pixel step, Triangulate and RefreshPixelVectors of the point loop go through
tests/mapmaker_ref.py (the bound library's ptam_subpix_batch, numpy's SVD)."""
import math

import numpy as np

from ptam_cg_amd import _abi, host

MAX_SSD = 100000       # MiniPatch::FindPatch's default nMaxSSD (include/ImageProcess.h:44)
RANGE = 10             # src/Tracker.cc:400
HALF = 4               # mirPatchSize (9, 9) / 2


def in_image_with_border(shape, x, y, border):
    h, w = shape
    return x >= border and y >= border and x < w - border and y < h - border


def sample_patch(im, x, y):
    """MiniPatch::SampleFromImage: GetImageROI(im, irPos, (9, 9))"""
    return im[y - HALF:y + HALF + 1, x - HALF:x + HALF + 1].copy()


def ssd_at_point(im, x, y, patch, max_ssd=MAX_SSD):
    """ImageProcess::SSDAtPoint (:57-80)"""
    if not in_image_with_border(im.shape, x, y, patch.shape[1] // 2) or not in_image_with_border(im.shape, x, y, patch.shape[0] // 2):
        return max_ssd + 1
    d = im[y - HALF:y + HALF + 1, x - HALF:x + HALF + 1].astype(np.int64) - patch.astype(np.int64)
    return int((d * d).sum())


def find_patch(pos, im, corners, patch, rng=RANGE, max_ssd=MAX_SSD, info=None):
    """MiniPatch::FindPatch (:204-252) without a row LUT -> (found, (x, y)).  corners: (n, 2) [x, y] in raster order.
    info (a dict, optional) counts the corners scored and those SSDAtPoint turned away at the border."""
    px, py = int(pos[0]), int(pos[1])
    best, best_ssd = None, max_ssd + 1
    tl = (px - rng, py - rng)
    br = (px + rng, py + rng)
    i = int(np.searchsorted(corners[:, 1], tl[1], side="left")) if len(corners) else 0   # first corner with y >= irBBoxTL.y
    while i < len(corners):
        cx, cy = int(corners[i, 0]), int(corners[i, 1])
        i += 1
        if cx < tl[0] or cx > br[0]:
            continue
        if cy > br[1]:
            break
        ssd = ssd_at_point(im, cx, cy, patch, max_ssd)
        if info is not None:
            info["scored"] = info.get("scored", 0) + 1
            info["border"] = info.get("border", 0) + int(ssd == max_ssd + 1 and not in_image_with_border(im.shape, cx, cy, HALF))
        if ssd < best_ssd:
            best, best_ssd = (cx, cy), ssd
    if info is not None:
        info["best_ssd"] = best_ssd
    if best_ssd < max_ssd:
        return True, best
    return False, (px, py)


def start_order(max_corners, st_scores, shape, min_shi_tomasi):
    """the candidates of level 0 (src/KeyFrame.cc:66-76) in the order of :356-359: std::sort of pair<-score, ImageRef>, ImageRef
    ordered by y, then x -> indices into max_corners"""
    cand = [i for i in range(len(max_corners))
            if in_image_with_border(shape, int(max_corners[i, 0]), int(max_corners[i, 1]), 10) and st_scores[i] > min_shi_tomasi]
    return sorted(cand, key=lambda i: (-float(st_scores[i]), int(max_corners[i, 1]), int(max_corners[i, 0])))


class Trails:
    """mlTrails + mPreviousFrameKF.  A frame is (im, corners): level 0 of a keyframe."""

    def __init__(self):
        self.trails = []          # [initial (x, y), current (x, y), patch]
        self.prev = None
        self.stats = dict(died_unfound=0, died_unmarried=0, border=0, scored=0, top=0, left=0, bottom=0)

    def start(self, im, corners, max_corners, st_scores, min_shi_tomasi=70.0, max_initial=1000, max_trails=1000):
        order = start_order(max_corners, st_scores, im.shape, min_shi_tomasi)
        self.trails = []
        for i in order[:max(0, min(max_initial, max_trails))]:
            p = (int(max_corners[i, 0]), int(max_corners[i, 1]))
            self.trails.append([p, p, sample_patch(im, *p)])
        self.prev = (im.copy(), corners.copy())
        return len(self.trails)

    def advance(self, im, corners):
        """-> (nGoodTrails, trails alive)"""
        good, keep = 0, []
        for tr in self.trails:
            start = tr[1]
            self.stats["top"] += int(start[1] - RANGE < 0)            # searches whose box leaves the image
            self.stats["left"] += int(start[0] - RANGE < 0)
            self.stats["bottom"] += int(start[1] + RANGE >= im.shape[0])
            info = {}
            found, end = find_patch(start, im, corners, tr[2], info=info)
            self.stats["border"] += info.get("border", 0)
            self.stats["scored"] += info.get("scored", 0)
            if found:
                back_patch = sample_patch(im, *end)
                info = {}
                found, back = find_patch(end, self.prev[0], self.prev[1], back_patch, info=info)
                self.stats["border"] += info.get("border", 0)
                self.stats["scored"] += info.get("scored", 0)
                dx, dy = back[0] - start[0], back[1] - start[1]
                if dx * dx + dy * dy > 2:
                    found = False
                tr[1] = end
                good += 1
                if not found:
                    self.stats["died_unmarried"] += 1
            else:
                self.stats["died_unfound"] += 1
            if found:
                keep.append(tr)
        self.trails = keep
        self.prev = (im.copy(), corners.copy())
        return good, len(keep)

    def table(self):
        out = np.zeros(len(self.trails), dtype=host.TRAIL_DT)
        for k, (a, b, _) in enumerate(self.trails):
            out[k] = (a[0], a[1], b[0], b[1])
        return out

    def patches(self):
        return np.array([t[2] for t in self.trails], dtype=np.uint8).reshape(-1, 9, 9)


class Camera:
    """ATANCamera with its cache of the last projection (src/ATANCamera.cc:27-66, 125-140, 179-209), plain floats"""

    def __init__(self, params=host.DEFAULT_CAMERA, size=(640, 480)):
        fx, fy, cx, cy, w = [float(v) for v in params]
        self.focal = (size[0] * fx, size[1] * fy)
        self.centre = (size[0] * cx - 0.5, size[1] * cy - 0.5)
        self.inv_focal = (1.0 / self.focal[0], 1.0 / self.focal[1])
        self.w = w
        if w != 0.0:
            self.two_tan = 2.0 * math.tan(w / 2.0)
            self.one_over_two_tan = 1.0 / self.two_tan
            self.w_inv = 1.0 / w
            self.distortion_enabled = 1.0
        else:
            self.two_tan = self.w_inv = self.distortion_enabled = 0.0
        self.last_cam, self.last_r, self.last_factor = (0.0, 0.0), 0.0, 1.0

    def unproject(self, u, v):
        dx = (u - self.centre[0]) * self.inv_focal[0]
        dy = (v - self.centre[1]) * self.inv_focal[1]
        dist_r = math.sqrt(dx * dx + dy * dy)
        self.last_r = dist_r if self.w == 0.0 else math.tan(dist_r * self.w) * self.one_over_two_tan
        factor = self.last_r / dist_r if dist_r > 0.01 else 1.0
        self.last_factor = 1.0 / factor
        self.last_cam = (factor * dx, factor * dy)
        return self.last_cam

    def projection_derivs(self):
        """GetProjectionDerivs on the cache -> row-major 2x2"""
        k, (x, y) = self.two_tan, self.last_cam
        r = self.last_r * self.distortion_enabled
        if r < 0.01:
            fx = fy = 0.0
        else:
            fx = self.w_inv * (k * x) / (r * r * (1 + k * k * r * r)) - x * self.last_factor / (r * r)
            fy = self.w_inv * (k * y) / (r * r * (1 + k * k * r * r)) - y * self.last_factor / (r * r)
        return (self.focal[0] * (fx * x + self.last_factor), self.focal[0] * (fy * x),
                self.focal[1] * (fx * y), self.focal[1] * (fy * y + self.last_factor))


def match_table(cam, table):
    """the first loop of InitFromStereo (:272-279) on a TRAIL_DT table"""
    out = np.zeros(len(table), dtype=host.HOMOGRAPHY_MATCH_DT)
    for k, t in enumerate(table):
        out[k]["first"] = cam.unproject(float(t["initial_x"]), float(t["initial_y"]))
        out[k]["second"] = cam.unproject(float(t["current_x"]), float(t["current_y"]))
        out[k]["jac"] = cam.projection_derivs()
    return out


def init_points(ctx, first_kf, second_kf, se3, matches, subpix_its=10):
    """the point loop of InitFromStereo (:310-367) composed on one bound library -> (points NEW_MAP_POINT_DT, status).  A centre
    nearer than 5 pixels to a border is template_bad, and RefreshPixelVectors sees the triangulated position: the meaning
    include/ptam_hip.h gives the two places where the reference reads what it has not written."""
    from tests import mapmaker_ref as M
    cam = M.Cam(ctx)
    pf = host.PatchFinder(ctx)
    matches = np.asarray(matches, dtype=host.TRAIL_DT)
    n = len(matches)
    status = np.full(n, _abi.INIT_MADE, dtype=np.int32)
    im = first_kf.level(0)["im"]
    sub_i, sub_pos, sub_t = [], [], []
    for i, m in enumerate(matches):
        x, y = int(m["initial_x"]), int(m["initial_y"])
        if not in_image_with_border(im.shape, x, y, 5):     # MakeTemplateCoarseNoWarp
            status[i] = _abi.INIT_TEMPLATE_BAD
            continue
        sub_i.append(i)
        sub_pos.append((float(m["current_x"]), float(m["current_y"])))
        sub_t.append(im[y - 4:y + 4, x - 4:x + 4].reshape(64))
    sr = pf.SubPix(second_kf, np.array(sub_pos).reshape(-1, 2), np.zeros(len(sub_i), np.int32),
                   np.array(sub_t, dtype=np.uint8).reshape(-1, 64), max_its=subpix_its) if sub_i else []
    identity = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])
    pts = []
    for k, i in enumerate(sub_i):
        if not sr[k]["converged"]:
            status[i] = _abi.INIT_SUBPIX_FAILED
            continue
        m = matches[i]
        x, y = float(m["initial_x"]), float(m["initial_y"])
        tp = (float(sr[k]["pos"][0]), float(sr[k]["pos"][1]))
        world = M.triangulate(np.asarray(se3, dtype=np.float64), cam.unproject(*tp), cam.unproject(x, y))   # first's pose: identity
        if world[2] < 0.0:
            status[i] = _abi.INIT_BEHIND_CAMERA
            continue
        cen, rgt, dwn = cam.unit_ray(x, y), cam.unit_ray(x + 1.0, y), cam.unit_ray(x, y + 1.0)
        pr, pd = M.refresh_pixel_vectors(identity, list(world), cen, rgt, dwn)
        p = np.zeros(1, dtype=host.NEW_MAP_POINT_DT)[0]
        p["point"]["world"], p["point"]["pixel_right_w"], p["point"]["pixel_down_w"] = world, pr, pd
        p["center_nc"], p["one_right_nc"], p["one_down_nc"] = cen, rgt, dwn
        p["src_root_pos"], p["target_pos"] = (x, y), tp
        p["level"], p["center_x"], p["center_y"], p["candidate"] = 0, int(m["initial_x"]), int(m["initial_y"]), i
        p["target_corner"], p["best_zmssd"] = -1, 0
        pts.append(p)
    out = np.array(pts, dtype=host.NEW_MAP_POINT_DT) if pts else np.zeros(0, dtype=host.NEW_MAP_POINT_DT)
    return out, status
