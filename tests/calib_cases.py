"""The calibrator tests' inputs, shared by the CPU and the GPU tests: grids from synth.make_calib_grids, cut to the corner counts a
test needs.  Nothing here touches the device."""
import numpy as np

from ptam_cg_amd import synth
from tests import calib_ref as CR

SIZE = (640, 480)
TRUTH = (0.62, 0.83, 0.48, 0.53, 0.9)
TRUTH_NO_DISTORTION = (0.62, 0.83, 0.48, 0.53, 0.0)


def recover_case(truth=TRUTH, seed=3):
    """4 images of an 8 x 6 grid at 6-10 grid units, all 48 corners in every image: [(corners, true pose)]"""
    return synth.make_calib_grids(truth, SIZE, 4, 8, 6, seed)


def _spread(c, n):
    """n of an image's corners, spread over the grid and never all on one line: the four outermost first"""
    gx, gy = c["gx"], c["gy"]
    ext = [int(np.argmin(gx + gy)), int(np.argmax(gx + gy)), int(np.argmin(gx - gy)), int(np.argmax(gx - gy))]
    rest = [i for i in range(len(c)) if i not in ext]
    rng = np.random.Generator(np.random.PCG64(len(c) * 1000 + n))
    rng.shuffle(rest)
    idx = (ext + rest)[:n]
    assert len(set(idx)) == n
    return c[np.sort(idx)].copy()


# The camera block's largest entry is (image width)^2 x measurements (the derivative of u by the normalised centre is the width):
# 1200 measurements at 640 x 480 put the condition number at 5e8, far beyond the bar of the comparing tests.  A small image keeps
# the many-view case below it; the arithmetic is the same.
SMALL_SIZE = (64, 48)


def images_with_counts(counts, truth=TRUTH, seed=5, size=SIZE):
    """one image per entry of counts, each with exactly that many corners of an 18 x 15 grid seen from 14-20 grid units"""
    out = []
    grids = synth.make_calib_grids(truth, size, 4 * len(counts), 18, 15, seed, distance=(14.0, 20.0))
    for n in counts:
        c, p = next((c, p) for c, p in grids if len(c) >= n and not any(c is d for d, _ in out))
        out.append((c, p))
    return [(_spread(c, n), p) for (c, p), n in zip(out, counts)]


def small_images(n_images, n_corners, seed, distance=(6.0, 10.0)):
    """n_images views of an 8 x 6 grid, n_corners of each kept"""
    return [(_spread(c, n_corners), p) for c, p in synth.make_calib_grids(TRUTH, SIZE, n_images, 8, 6, seed, distance=distance)]


def mixed_counts_65():
    return [63, 64, 65, 255, 256, 257] + [4 + (5 * k) % 9 for k in range(59)]


def reference_from(images, params=None, disable=False, size=SIZE):
    """the restatement with these images added (its own initial poses)"""
    ref = CR.Calibrator(size, params, disable)
    for c, _ in images:
        assert ref.add_image(c) == CR.GUESS_OK
    return ref


def solver_noise(ref):
    """the relative difference between the restatement's SVD solve and block elimination in longdouble on ref's current system,
    and the system's condition number"""
    JTJ, JTe, _, _ = ref.build_system()
    a = CR.svd_backsub(JTJ, JTe)
    b = CR.block_solve_longdouble(JTJ, JTe)
    sv = np.linalg.svd(JTJ, compute_uv=False)
    return float(np.abs(a - b.astype(np.float64)).max() / np.abs(b).max()), CR.condition_number(sv)
