// motion_device.h — the motion model's prediction with the rotation estimator on (src/Tracker.cc:1013-1029), for host and device:
// the twin of motion.hip's so3_ln and ptam_motion_predict_sbi, the same operations in the same order.  The batch's align workgroup
// runs it behind SE3fromSE2 (sbi.hip), where the rotation is.  The device's asin / acos / sin / cos are not glibc's: against the host
// function the result agrees to a few ulps, not to the bit.
#pragma once
#include "common.h"

// TooN SO3<>::ln: rotation vector of R (row-major).  Three ranges of the angle: asin of the antisymmetric part's norm up to
// pi/4, acos of the trace up to 3 pi/4, and beyond that the axis from the symmetric part (the antisymmetric one vanishes at pi).
PTAM_HD void so3_ln_hd(const double* R, double w[3]) {
#pragma clang fp contract(off)   // (plain products and sums, as the host's compiler emits them)
    const double sqrt1_2 = 0.70710678118654752440, pi = 3.14159265358979323846;   // M_SQRT1_2, M_PI
    const double cos_angle = (R[0] + R[4] + R[8] - 1.0) * 0.5;
    w[0] = (R[7] - R[5]) / 2;
    w[1] = (R[2] - R[6]) / 2;
    w[2] = (R[3] - R[1]) / 2;
    const double sin_angle_abs = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    if (cos_angle > sqrt1_2) {
        if (sin_angle_abs > 0) {
            const double s = asin(sin_angle_abs) / sin_angle_abs;
            for (int i = 0; i < 3; i++) w[i] *= s;
        }
    } else if (cos_angle > -sqrt1_2) {
        const double s = acos(cos_angle) / sin_angle_abs;
        for (int i = 0; i < 3; i++) w[i] *= s;
    } else {
        const double angle = pi - asin(sin_angle_abs);
        const double d0 = R[0] - cos_angle, d1 = R[4] - cos_angle, d2 = R[8] - cos_angle;
        double r2[3];
        if (d0 * d0 > d1 * d1 && d0 * d0 > d2 * d2) {
            r2[0] = d0;
            r2[1] = (R[3] + R[1]) / 2;
            r2[2] = (R[2] + R[6]) / 2;
        } else if (d1 * d1 > d2 * d2) {
            r2[0] = (R[3] + R[1]) / 2;
            r2[1] = d1;
            r2[2] = (R[7] + R[5]) / 2;
        } else {
            r2[0] = (R[2] + R[6]) / 2;
            r2[1] = (R[7] + R[5]) / 2;
            r2[2] = d2;
        }
        if (r2[0] * w[0] + r2[1] * w[1] + r2[2] * w[2] < 0)
            for (int i = 0; i < 3; i++) r2[i] = -r2[i];
        const double inv = 1.0 / sqrt(r2[0] * r2[0] + r2[1] * r2[1] + r2[2] * r2[2]);
        for (int i = 0; i < 3; i++) w[i] = angle * (r2[i] * inv);
    }
}

// TooN SE3<>::exp followed by the left-multiplication (common.h: se3_exp_mul<false>), operation by operation and WITHOUT contraction:
// the host's compiler emits plain products and sums where the device's would fuse a * b + c into one rounding, and a prediction that
// differs from the host's in the last bit grows, frame over frame, through the byte-truncated templates of the patch search.
PTAM_HD void se3_exp_mul_plain(const double* mu, const double* T, double* out) {
#pragma clang fp contract(off)
    const double one_6th = 1.0 / 6.0, one_20th = 1.0 / 20.0;
    const double tx = mu[0], ty = mu[1], tz = mu[2], wx = mu[3], wy = mu[4], wz = mu[5];
    const double theta_sq = wx * wx + wy * wy + wz * wz;
    const double cx = wy * tz - wz * ty, cy = wz * tx - wx * tz, cz = wx * ty - wy * tx;
    double A, B, R[9], et[3];
    if (theta_sq < 1e-8) {
        A = 1.0 - one_6th * theta_sq;
        B = 0.5;
        et[0] = tx + 0.5 * cx;
        et[1] = ty + 0.5 * cy;
        et[2] = tz + 0.5 * cz;
    } else {
        double Cc;
        if (theta_sq < 1e-6) {
            Cc = one_6th * (1.0 - one_20th * theta_sq);
            A = 1.0 - theta_sq * Cc;
            B = 0.5 - 0.25 * one_6th * theta_sq;
        } else {
            const double theta = sqrt(theta_sq);
            const double inv_theta = 1.0 / theta;
            A = sin(theta) * inv_theta;
            B = (1 - cos(theta)) * (inv_theta * inv_theta);
            Cc = (1 - A) * (inv_theta * inv_theta);
        }
        const double dx = wy * cz - wz * cy, dy = wz * cx - wx * cz, dz = wx * cy - wy * cx;
        et[0] = tx + B * cx + Cc * dx;
        et[1] = ty + B * cy + Cc * dy;
        et[2] = tz + B * cz + Cc * dz;
    }
    {
        const double wx2 = wx * wx, wy2 = wy * wy, wz2 = wz * wz;
        R[0] = 1.0 - B * (wy2 + wz2);
        R[4] = 1.0 - B * (wx2 + wz2);
        R[8] = 1.0 - B * (wx2 + wy2);
        double a = A * wz, b = B * (wx * wy);
        R[1] = b - a;
        R[3] = b + a;
        a = A * wy;
        b = B * (wx * wz);
        R[2] = b + a;
        R[6] = b - a;
        a = A * wx;
        b = B * (wy * wz);
        R[5] = b - a;
        R[7] = b + a;
    }
    double o[12];
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++)
            o[r * 3 + c] = R[r * 3 + 0] * T[0 * 3 + c] + R[r * 3 + 1] * T[1 * 3 + c] + R[r * 3 + 2] * T[2 * 3 + c];
        o[9 + r] = et[r] + (R[r * 3 + 0] * T[9] + R[r * 3 + 1] * T[10] + R[r * 3 + 2] * T[11]);
    }
    for (int i = 0; i < 12; i++) out[i] = o[i];
}

// ptam_motion_predict_sbi without the model around it: v = velocity with v[3..5] = ln(rotation), v[0] = v[1] = 0 (v[2] stays);
// pose_out = exp(v) * start_pose
PTAM_HD void motion_predict_sbi_hd(const double velocity[6], const double start_pose[12], const double rotation[9], double pose_out[12]) {
    double v[6];
    for (int i = 0; i < 6; i++) v[i] = velocity[i];
    so3_ln_hd(rotation, v + 3);   // SE3<>::ln of a pose without translation: (0, 0, 0, rotation vector)
    v[0] = v[1] = 0.0;
    se3_exp_mul_plain(v, start_pose, pose_out);
}
