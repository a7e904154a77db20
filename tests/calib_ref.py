"""The camera calibrator's optimiser restated in numpy, function by function, as the yardstick of ptam_calib_*:
ATANCamera::RefreshParams / Project / UnProject / GetProjectionDerivs / GetCameraParameterDerivs / UpdateParams /
DisableRadialDistortion (src/ATANCamera.cc:27-66, 109-140, 179-252), CalibImage::GuessInitialPose and CalibImage::Project
(src/CalibImage.cc:514-648) and CameraCalibrator::OptimizeOneStep (src/CameraCalibrator.cc:215-269) with its dense
(6 views + 5)^2 matrix and SVD back-substitution.  Work per corner is vectorised over an image's corners; nothing else is changed.

Two things about TooN are ASSUMED here, because TooN is not part of this repository and neither can be read in the reference:
  1. SVD<>::backsub(rhs) uses the condition 1e9: a singular value s_i with s_i * 1e9 <= s_0 is treated as zero (its reciprocal is
     replaced by 0), every other one is inverted.  This is how TooN's SVD.h is remembered; it is not verifiable from the reference.
  2. The sign of svdHomography.get_VT()[8] is LAPACK's.  A singular vector's sign is free, so the restatement (like the device)
     takes the sign for which the guessed translation's z is positive; with the other sign the camera is behind the grid,
     Project skips every corner and mdMeanPixelError is 0 / 0.
The device solves the arrowhead system by block elimination without the cut of (1); the two agree while the condition number
stays far below 1e9, which every comparing test asserts first (optimize_one_step returns the matrix's singular values)."""
import numpy as np

CORNER_DT = np.dtype([("gx", "<i4"), ("gy", "<i4"), ("u", "<f8"), ("v", "<f8")])
DEFAULT_PARAMS = (0.5, 0.75, 0.5, 0.5, 0.1)   # ATANCamera::mvDefaultParams src/ATANCamera.cc:286
GUESS_OK, GUESS_REFUSED = 0, 1


class Camera:
    """the members of ATANCamera that the calibrator reads"""

    def __init__(self, params=DEFAULT_PARAMS, size=(640, 480)):
        self.params = np.array(params, dtype=np.float64)
        self.size = np.array(size, dtype=np.float64)
        self.refresh()

    def refresh(self):   # RefreshParams :27-66
        p = self.params
        self.focal = np.array([self.size[0] * p[0], self.size[1] * p[1]])
        self.centre = np.array([self.size[0] * p[2] - 0.5, self.size[1] * p[3] - 0.5])
        with np.errstate(divide="ignore"):
            self.inv_focal = np.array([1.0 / self.focal[0], 1.0 / self.focal[1]])
        self.w = p[4]
        if self.w != 0.0:
            self.two_tan = 2.0 * np.tan(self.w / 2.0)
            self.one_over_two_tan = 1.0 / self.two_tan
            self.w_inv = 1.0 / self.w
            self.dist_enabled = 1.0
        else:
            self.w_inv = 0.0
            self.two_tan = 0.0
            self.one_over_two_tan = 0.0
            self.dist_enabled = 0.0
        with np.errstate(divide="ignore", invalid="ignore"):
            v0 = max(p[2], 1.0 - p[2]) / p[0]
            v1 = max(p[3], 1.0 - p[3]) / p[1]
            self.largest_radius = self.invrtrans(np.sqrt(v0 * v0 + v1 * v1))
        self.max_r = 1.5 * self.largest_radius

    def invrtrans(self, r):   # include/ATANCamera.h:152-157
        if self.w == 0.0:
            return r
        return np.tan(r * self.w) * self.one_over_two_tan

    def rtrans_factor(self, r):   # include/ATANCamera.h:143-149
        if self.w == 0.0:
            return np.ones_like(r)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(r < 0.001, 1.0, self.w_inv * np.arctan(r * self.two_tan) / r)

    def project(self, cam):   # Project :109-121 -> image (n, 2); leaves the cached members
        cam = np.asarray(cam, dtype=np.float64).reshape(-1, 2)
        self.last_cam = cam
        self.last_r = np.sqrt(cam[:, 0] * cam[:, 0] + cam[:, 1] * cam[:, 1])
        self.invalid = self.last_r > self.max_r
        self.last_factor = self.rtrans_factor(self.last_r)
        dist_cam = self.last_factor[:, None] * cam
        return np.stack([self.centre[0] + self.focal[0] * dist_cam[:, 0], self.centre[1] + self.focal[1] * dist_cam[:, 1]], axis=1)

    def unproject(self, im):   # UnProject :125-140
        im = np.asarray(im, dtype=np.float64).reshape(-1, 2)
        with np.errstate(all="ignore"):
            dc = np.stack([(im[:, 0] - self.centre[0]) * self.inv_focal[0], (im[:, 1] - self.centre[1]) * self.inv_focal[1]], axis=1)
            dist_r = np.sqrt(dc[:, 0] * dc[:, 0] + dc[:, 1] * dc[:, 1])
            r = self.invrtrans(dist_r)
            factor = np.where(dist_r > 0.01, r / dist_r, 1.0)
            return factor[:, None] * dc

    def projection_derivs(self):   # GetProjectionDerivs :179-209 at the last projection -> (n, 2, 2)
        k, x, y = self.two_tan, self.last_cam[:, 0], self.last_cam[:, 1]
        r = self.last_r * self.dist_enabled
        with np.errstate(divide="ignore", invalid="ignore"):
            fx = self.w_inv * (k * x) / (r * r * (1 + k * k * r * r)) - x * self.last_factor / (r * r)
            fy = self.w_inv * (k * y) / (r * r * (1 + k * k * r * r)) - y * self.last_factor / (r * r)
        fx = np.where(r < 0.01, 0.0, fx)
        fy = np.where(r < 0.01, 0.0, fy)
        D = np.zeros((len(x), 2, 2))
        D[:, 0, 0] = self.focal[0] * (fx * x + self.last_factor)
        D[:, 1, 0] = self.focal[1] * (fx * y)
        D[:, 0, 1] = self.focal[0] * (fy * x)
        D[:, 1, 1] = self.focal[1] * (fy * y + self.last_factor)
        return D

    def camera_parameter_derivs(self):   # GetCameraParameterDerivs :211-237 at the last projection -> (n, 2, 5)
        normal = self.params.copy()
        cam = self.last_cam
        out = self.project(cam)
        J = np.zeros((len(cam), 2, 5))
        for i in range(5):
            if i == 4 and self.w == 0.0:
                continue
            upd = np.zeros(5)
            upd[i] += 0.001
            self.update_params(upd)
            out_b = self.project(cam)
            J[:, :, i] = (out_b - out) / 0.001
            self.params = normal.copy()
            self.refresh()
        if self.w == 0.0:
            J[:, :, 4] = 0.0
        return J

    def update_params(self, upd):   # UpdateParams :239-244
        self.params = self.params + upd
        self.refresh()

    def disable_radial_distortion(self):   # :246-252
        self.params[4] = 0.0
        self.refresh()

    def pixel_aspect_ratio(self):   # include/ATANCamera.h:101
        return self.focal[1] / self.focal[0]


# ---- SE3 (TooN) ---------------------------------------------------------------------------------------------------------------
def se3_exp(mu):
    """SE3<>::exp -> pose (12,): R row-major, then t"""
    t, w = np.asarray(mu[:3], float), np.asarray(mu[3:], float)
    th2 = w @ w
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    cr = np.cross(w, t)
    if th2 < 1e-8:
        A, B = 1.0 - th2 / 6.0, 0.5
        trans = t + 0.5 * cr
    else:
        if th2 < 1e-6:
            C = (1.0 - th2 / 20.0) / 6.0
            A = 1.0 - th2 * C
            B = 0.5 - 0.25 * (1.0 / 6.0) * th2
        else:
            th = np.sqrt(th2)
            A = np.sin(th) / th
            B = (1 - np.cos(th)) / th2
            C = (1 - A) / th2
        trans = t + B * cr + C * np.cross(w, cr)
    R = np.eye(3) + A * K + B * (K @ K)
    return np.concatenate([R.ravel(), trans])


def se3_mul(a, b):
    Ra, Rb = a[:9].reshape(3, 3), b[:9].reshape(3, 3)
    return np.concatenate([(Ra @ Rb).ravel(), a[9:] + Ra @ b[9:]])


# ---- CalibImage ---------------------------------------------------------------------------------------------------------------
def guess_initial_pose(cam, corners):
    """GuessInitialPose :514-606 -> (status, pose (12,)).  Assumption 2 of the module's header: the null vector's sign is the one
    that puts the grid in front of the camera; a guess that is not finite or has z == 0 is refused."""
    n = len(corners)
    un = cam.unproject(np.stack([corners["u"], corners["v"]], axis=1))
    x, y = corners["gx"].astype(np.float64), corners["gy"].astype(np.float64)
    u, v = un[:, 0], un[:, 1]
    M = np.zeros((2 * n, 9))
    M[0::2, 0], M[0::2, 1], M[0::2, 2] = x, y, 1
    M[0::2, 6], M[0::2, 7], M[0::2, 8] = -x * u, -y * u, -u
    M[1::2, 3], M[1::2, 4], M[1::2, 5] = x, y, 1
    M[1::2, 6], M[1::2, 7], M[1::2, 8] = -x * v, -y * v, -v
    if not np.isfinite(M).all():
        return GUESS_REFUSED, np.full(12, np.nan)
    vt = np.linalg.svd(M, full_matrices=True)[2]
    vh = vt[8]
    if vh[8] < 0:   # (t_z is h[8] over two positive numbers)
        vh = -vh
    H = vh.reshape(3, 3).copy()
    with np.errstate(divide="ignore", invalid="ignore"):
        # the possibly poorly conditioned top-left bit :563-583
        _, diag, vt2 = np.linalg.svd(H[:2, :2])
        H = H / diag[0]
        diag = diag / diag[0]
        lam2 = diag[1]
        b = np.array([0.0, np.sqrt(1.0 - lam2 * lam2)])
        aprime = b @ vt2
        a = H[2, :2]
        H[2, :2] = aprime if a @ aprime > 0 else -aprime
        # Gram-Schmidt :586-601
        mag1 = np.sqrt(H[:, 0] @ H[:, 0])
        H = H / mag1
        R = np.zeros((3, 3))
        R[:, 0] = H[:, 0]
        R[:, 1] = H[:, 1] - H[:, 0] * (H[:, 0] @ H[:, 1])
        R[:, 1] /= np.sqrt(R[:, 1] @ R[:, 1])
        R[:, 2] = np.cross(R[:, 0], R[:, 1])
        t = H[:, 2]
    pose = np.concatenate([R.ravel(), t])
    if not np.isfinite(pose).all() or t[2] == 0.0:
        return GUESS_REFUSED, pose
    return GUESS_OK, pose


def project_image(cam, pose, corners):
    """CalibImage::Project :608-648 -> (kept indices, v2Error (m, 2), m26PoseJac (m, 2, 6), m2NCameraJac (m, 2, 5), image (n, 2),
    valid (n,)); image / valid are what Draw3DGrid(..., true) projects, for every corner"""
    R, t = pose[:9].reshape(3, 3), pose[9:]
    world = np.stack([corners["gx"].astype(np.float64), corners["gy"].astype(np.float64), np.zeros(len(corners))], axis=1)
    c3 = world @ R.T + t
    front = ~(c3[:, 2] <= 0.001)
    with np.errstate(divide="ignore", invalid="ignore"):
        plane = c3[:, :2] / c3[:, 2:3]
    image_all = cam.project(np.where(front[:, None], plane, 0.0))
    valid = front & ~cam.invalid
    keep = np.nonzero(valid)[0]
    c3k = c3[keep]
    image = cam.project(plane[keep])
    err = np.stack([corners["u"][keep], corners["v"][keep]], axis=1) - image
    iz = 1.0 / c3k[:, 2]
    D = cam.projection_derivs()
    G = np.zeros((len(keep), 6, 3))   # SE3<>::generator_field(dof, unproject(v3Cam))
    G[:, 0, 0] = G[:, 1, 1] = G[:, 2, 2] = 1.0
    X, Y, Z = c3k[:, 0], c3k[:, 1], c3k[:, 2]
    G[:, 3, 1], G[:, 3, 2] = -Z, Y
    G[:, 4, 2], G[:, 4, 0] = -X, Z
    G[:, 5, 0], G[:, 5, 1] = -Y, X
    m0 = (G[:, :, 0] - X[:, None] * G[:, :, 2] * iz[:, None]) * iz[:, None]
    m1 = (G[:, :, 1] - Y[:, None] * G[:, :, 2] * iz[:, None]) * iz[:, None]
    Jp = np.zeros((len(keep), 2, 6))
    Jp[:, 0, :] = D[:, 0, 0:1] * m0 + D[:, 0, 1:2] * m1
    Jp[:, 1, :] = D[:, 1, 0:1] * m0 + D[:, 1, 1:2] * m1
    Jc = cam.camera_parameter_derivs()
    return keep, err, Jp, Jc, image_all, valid


class Calibrator:
    """CameraCalibrator's state: the camera, mgvnDisableDistortion and mvCalibImgs (corners, mse3CamFromWorld)"""

    def __init__(self, size=(640, 480), params=None, disable_distortion=False):
        self.size = size
        self.reset(params, disable_distortion)

    def reset(self, params=None, disable_distortion=False):   # Reset src/CameraCalibrator.cc:156-165
        self.cam = Camera(DEFAULT_PARAMS if params is None else params, self.size)
        self.disable = bool(disable_distortion)
        if self.disable:
            self.cam.disable_radial_distortion()
        self.corners, self.poses = [], []
        self.rms, self.n_meas = float("nan"), 0

    def add_image(self, corners):   # :105-106 -> status
        corners = np.ascontiguousarray(corners, dtype=CORNER_DT)
        st, pose = guess_initial_pose(self.cam, corners)
        if st == GUESS_OK:
            self.corners.append(corners)
            self.poses.append(pose)
        return st

    def build_system(self):
        """the accumulation of OptimizeOneStep :217-260 -> (mJTJ, vJTe, sum of squared errors, measurement count)"""
        nv = len(self.poses)
        dim = 6 * nv + 5
        cb = dim - 5
        JTJ, JTe = np.eye(dim), np.zeros(dim)
        if self.disable:
            self.cam.disable_radial_distortion()
        ssq, nmeas = 0.0, 0
        for n in range(nv):
            mb = n * 6
            _, err, Jp, Jc, _, _ = project_image(self.cam, self.poses[n], self.corners[n])
            for i in range(len(err)):
                JTJ[mb:mb + 6, mb:mb + 6] += Jp[i].T @ Jp[i]
                JTJ[cb:, cb:] += Jc[i].T @ Jc[i]
                JTJ[mb:mb + 6, cb:] += Jp[i].T @ Jc[i]
                JTJ[cb:, mb:mb + 6] += (Jp[i].T @ Jc[i]).T
                JTe[mb:mb + 6] += Jp[i].T @ err[i]
                JTe[cb:] += Jc[i].T @ err[i]
                ssq += err[i] @ err[i]
                nmeas += 1
        return JTJ, JTe, ssq, nmeas

    def optimize_one_step(self):
        """OptimizeOneStep :215-269 -> dict(rms, n_meas, update (the scaled vUpdate), sv (the matrix's singular values), JTJ, JTe).
        Nothing to adjust (the reference divides by zero): returns n_meas 0 and changes nothing."""
        JTJ, JTe, ssq, nmeas = self.build_system()
        if nmeas == 0:
            return dict(rms=float("nan"), n_meas=0, update=None, sv=None, JTJ=JTJ, JTe=JTe)
        self.rms, self.n_meas = float(np.sqrt(ssq / nmeas)), nmeas
        update = 0.1 * svd_backsub(JTJ, JTe)
        sv = np.linalg.svd(JTJ, compute_uv=False)
        for n in range(len(self.poses)):
            self.poses[n] = se3_mul(se3_exp(update[n * 6:n * 6 + 6]), self.poses[n])
        self.cam.update_params(update[-5:])
        return dict(rms=self.rms, n_meas=nmeas, update=update, sv=sv, JTJ=JTJ, JTe=JTe)

    def residuals(self, image):
        """what Draw3DGrid(Camera, true) draws for one image :493-501 -> (projected (n, 2), valid (n,))"""
        _, _, _, _, im, valid = project_image(self.cam, self.poses[image], self.corners[image])
        return im, valid


def svd_backsub(M, rhs):
    """SVD<> svd(M); svd.backsub(rhs) — assumption 1 of the module's header"""
    U, s, Vt = np.linalg.svd(M)
    inv = np.where(s * 1e9 > s[0], 1.0 / s, 0.0)
    return Vt.T @ (inv * (U.T @ rhs))


def condition_number(sv):
    return float(sv[0] / sv[-1])


def block_solve_longdouble(JTJ, JTe):
    """the same system by block elimination of the 6x6 view blocks (the order the device solves in), in numpy longdouble"""
    M, r = JTJ.astype(np.longdouble), JTe.astype(np.longdouble)
    nv = (len(r) - 5) // 6
    cb = 6 * nv
    S, g = M[cb:, cb:].copy(), r[cb:].copy()
    Dinv = []
    for n in range(nv):
        D, B = M[n * 6:n * 6 + 6, n * 6:n * 6 + 6], M[n * 6:n * 6 + 6, cb:]
        Di = _inv_longdouble(D)
        Dinv.append(Di)
        S -= B.T @ Di @ B
        g -= B.T @ Di @ r[n * 6:n * 6 + 6]
    dc = _inv_longdouble(S) @ g
    out = np.zeros(len(r), np.longdouble)
    out[cb:] = dc
    for n in range(nv):
        out[n * 6:n * 6 + 6] = Dinv[n] @ (r[n * 6:n * 6 + 6] - M[n * 6:n * 6 + 6, cb:] @ dc)
    return out


def _inv_longdouble(A):
    """Gauss-Jordan with partial pivoting in longdouble (numpy.linalg has no longdouble)"""
    n = len(A)
    W = np.concatenate([A.astype(np.longdouble), np.eye(n, dtype=np.longdouble)], axis=1)
    for c in range(n):
        p = c + int(np.argmax(np.abs(W[c:, c])))
        W[[c, p]] = W[[p, c]]
        W[c] = W[c] / W[c, c]
        for r in range(n):
            if r != c:
                W[r] = W[r] - W[r, c] * W[c]
    return W[:, n:]
