"""ctypes view of include/ptam_hip.h and include/ptam_hip_bench.h, and their only statement in Python: a class for every struct
(ptam_foo_bar or ptam_foo_bar_t -> FooBar, the header's field names), a constant for every enumerator and integer #define (the
header's name without PTAM_), a PROTOTYPES entry for every function.  host.py derives its numpy record types from the classes;
tests/test_abi.py compares all of it with the headers as a C compiler reads them.

`bind(lib, prefix)` attaches argtypes/restypes for every entry point that the given shared library
exports under `prefix` ("ptam_" for libptam_hip.so).  The binding is prefix-generic so that the
test-suite can drive its CPU checker through the very same host classes; the package itself only
ever loads libptam_hip.so (see _lib.py).
"""
import ctypes as C

LEVELS = 4
PATCH = 8
MAX_SSD = 8 * 8 * 500
OK, E_ARG, E_HIP, E_STATE, E_LIMIT, E_COMM = 0, -1, -2, -3, -4, -5
HALFSAMPLE_R, HALFSAMPLE_T = 0, 1
EST_TUKEY, EST_CAUCHY, EST_HUBER = 0, 1, 2
K_PROJECT, K_SELECT, K_JACOBIAN, K_VINV, K_SCHUR, K_SOLVE, K_UPDATE, K_EXCHANGE, K_COUNT = range(9)
KERNEL_NAMES = ["project", "select", "jacobian", "vinv", "schur", "solve", "update", "exchange"]
TRACK_STAGE_NAMES = ["pyramid_pvs", "fast_detect", "compact_select", "search_coarse", "gather_coarse", "pose_coarse",
                     "search_fine", "gather_fine", "pose_fine"]


class Int2(C.Structure):
    _fields_ = [("x", C.c_int32), ("y", C.c_int32)]


class CamParams(C.Structure):
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("w", C.c_double), ("width", C.c_int32), ("height", C.c_int32)]


class PatchQuery(C.Structure):
    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("level", C.c_int32), ("range", C.c_uint32)]


class PatchResult(C.Structure):
    _fields_ = [("found", C.c_int32), ("best_ssd", C.c_int32), ("best_x", C.c_int32),
                ("best_y", C.c_int32), ("n_scored", C.c_int32), ("pad_", C.c_int32),
                ("pos", C.c_double * 2)]


class Projection(C.Structure):
    _fields_ = [("cam", C.c_double * 3), ("image", C.c_double * 2), ("derivs", C.c_double * 4),
                ("in_image", C.c_int32), ("pad_", C.c_int32)]


class SubpixQuery(C.Structure):
    _fields_ = [("coarse_pos", C.c_double * 2), ("level", C.c_int32), ("max_its", C.c_int32)]


class SubpixResult(C.Structure):
    _fields_ = [("converged", C.c_int32), ("iterations", C.c_int32), ("pos", C.c_double * 2), ("mean_diff", C.c_double)]


class TemplateQuery(C.Structure):
    _fields_ = [("src_kf", C.c_void_p), ("src_level", C.c_int32), ("search_level", C.c_int32), ("center_x", C.c_int32),
                ("center_y", C.c_int32), ("warp_inverse", C.c_double * 4)]


class TemplateResult(C.Structure):
    _fields_ = [("bad", C.c_int32), ("n_outside", C.c_int32), ("sum", C.c_int32), ("sum_sq", C.c_int32), ("m2", C.c_double * 4)]


class EpipolarQuery(C.Structure):
    _fields_ = [("level_x", C.c_int32), ("level_y", C.c_int32), ("normal", C.c_double * 2), ("norm_dist", C.c_double),
                ("along", C.c_double * 2), ("min_len", C.c_double), ("max_len", C.c_double), ("max_dist_sq", C.c_double)]


class EpipolarResult(C.Structure):
    _fields_ = [("best", C.c_int32), ("best_zmssd", C.c_int32), ("n_scored", C.c_int32), ("template_bad", C.c_int32)]


class PvsPoint(C.Structure):
    _fields_ = [("world", C.c_double * 3), ("pixel_right_w", C.c_double * 3), ("pixel_down_w", C.c_double * 3)]


class PvsResult(C.Structure):
    _fields_ = [("proj", Projection), ("warp_inverse", C.c_double * 4), ("level", C.c_int32), ("pad_", C.c_int32)]


class RefindResult(C.Structure):
    _fields_ = [("found", C.c_int32), ("level", C.c_int32), ("sub_pix", C.c_int32), ("never_retry", C.c_int32), ("root_pos", C.c_double * 2)]


class RefindPair(C.Structure):
    _fields_ = [("kf", C.c_void_p), ("kf_pose", C.c_double * 12), ("point", PvsPoint), ("source", TemplateQuery), ("point_id", C.c_int64),
                ("skip", C.c_int32), ("pad_", C.c_int32)]


class EpipolarOpts(C.Structure):
    """ptam_epipolar_opts (MapMaker::AddSomeMapPoints, src/MapMaker.cc:448-457)"""
    _fields_ = [("depth_mean", C.c_double), ("depth_sigma", C.c_double), ("wiggle_scale", C.c_double), ("min_shi_tomasi", C.c_double),
                ("subpix_max_its", C.c_int32), ("n_levels", C.c_int32), ("levels", C.c_int32 * 4)]


class NewMapPoint(C.Structure):
    _fields_ = [("point", PvsPoint), ("center_nc", C.c_double * 3), ("one_right_nc", C.c_double * 3), ("one_down_nc", C.c_double * 3),
                ("src_root_pos", C.c_double * 2), ("target_pos", C.c_double * 2), ("level", C.c_int32), ("center_x", C.c_int32),
                ("center_y", C.c_int32), ("candidate", C.c_int32), ("target_corner", C.c_int32), ("best_zmssd", C.c_int32)]


class Trail(C.Structure):
    """ptam_trail (Trail::irInitialPos / irCurrentPos, src/Tracker.cc:352-432)"""
    _fields_ = [("initial_x", C.c_int32), ("initial_y", C.c_int32), ("current_x", C.c_int32), ("current_y", C.c_int32)]


class HomographyMatch(C.Structure):
    """ptam_homography_match (HomographyMatch, include/HomographyInit.h:23-29)"""
    _fields_ = [("first", C.c_double * 2), ("second", C.c_double * 2), ("jac", C.c_double * 4)]


class HomographyOpts(C.Structure):
    """ptam_homography_opts (HomographyInit::Compute, src/HomographyInit.cc)"""
    _fields_ = [("max_pixel_error", C.c_double), ("trials", C.c_int32), ("seed", C.c_uint64), ("samples", C.POINTER(C.c_int32))]


class HomographyInfo(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_matches", C.c_int32), ("n_inliers", C.c_int32), ("best_trial", C.c_int32),
                ("ambiguous", C.c_int32), ("best_score", C.c_double), ("homography", C.c_double * 9), ("sampson", C.c_double * 2)]


HOMOG_OK, HOMOG_DEGENERATE, HOMOG_NO_INLIERS = range(3)
INIT_MADE, INIT_SUBPIX_FAILED, INIT_BEHIND_CAMERA, INIT_TEMPLATE_BAD = range(4)   # ptam_init_points_from_trails status


class EpipolarLevelStats(C.Structure):
    _fields_ = [(f, C.c_int32) for f in ("candidates", "kept_after_thinning", "ray_rejected", "line_rejected", "template_bad",
                                         "no_match", "subpix_failed", "made")]


class PoseMeas(C.Structure):
    _fields_ = [("world", C.c_double * 3), ("found", C.c_double * 2), ("sqrt_inv_noise", C.c_double)]


class GnOpts(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("nonlinear_mask", C.c_uint32),
                ("override_after", C.c_int32), ("override_sigma_sq", C.c_double),
                ("mark_outliers_iter", C.c_int32), ("estimator", C.c_int32), ("prior", C.c_double)]


class PoseUpdateMeas(C.Structure):
    _fields_ = [("found", C.c_double * 2), ("image", C.c_double * 2), ("sqrt_inv_noise", C.c_double),
                ("jac", C.c_double * 12)]


class BaOpts(C.Structure):
    _fields_ = [("max_iterations", C.c_int32), ("update_sq_conv_limit", C.c_double),
                ("min_sigma", C.c_double), ("estimator", C.c_int32), ("verbose", C.c_int32),
                ("deterministic", C.c_int32), ("pad_", C.c_int32)]


class MotionModel(C.Structure):
    """ptam_motion_model (src/Tracker.cc:1008-1056)"""
    _fields_ = [("pose", C.c_double * 12), ("start_pose", C.c_double * 12), ("velocity", C.c_double * 6),
                ("msd_scaled_velocity", C.c_double), ("scene_depth_mean", C.c_double), ("scene_depth_sigma", C.c_double),
                ("coarse_min_velocity", C.c_double), ("use_constant_velocity", C.c_int32), ("disable_coarse", C.c_int32),
                ("just_recovered", C.c_int32), ("pad_", C.c_int32)]


class BaTrial(C.Structure):
    """ptam_ba_trial (`lambda` is read with getattr)"""
    _fields_ = [("lambda", C.c_double), ("sigma_sq", C.c_double), ("err_old", C.c_double),
                ("err_new", C.c_double), ("sum_sq_update", C.c_double), ("n_bad", C.c_int32),
                ("accepted", C.c_int32)]


MAP_BA_ALL, MAP_BA_RECENT = 0, 1
MAP_SRC_TRACKER, MAP_SRC_REFIND, MAP_SRC_ROOT, MAP_SRC_TRAIL, MAP_SRC_EPIPOLAR = range(5)   # Measurement::Source, include/KeyFrame.h:50
MAP_OUT_POINT_BAD, MAP_OUT_FAILURE_QUEUE, MAP_OUT_NEVER_RETRY = 1, 2, 3
# (the shorter names the map code and its tests say)
SRC_TRACKER, SRC_REFIND, SRC_ROOT, SRC_TRAIL, SRC_EPIPOLAR = MAP_SRC_TRACKER, MAP_SRC_REFIND, MAP_SRC_ROOT, MAP_SRC_TRAIL, MAP_SRC_EPIPOLAR
OUT_POINT_BAD, OUT_FAILURE_QUEUE, OUT_NEVER_RETRY = MAP_OUT_POINT_BAD, MAP_OUT_FAILURE_QUEUE, MAP_OUT_NEVER_RETRY


class MapMeas(C.Structure):
    """ptam_map_meas: one row of the table of all keyframes' mMeasurements"""
    _fields_ = [("kf", C.c_int32), ("point", C.c_int32), ("level", C.c_int32), ("source", C.c_int32), ("root_pos", C.c_double * 2)]


class MapOutlier(C.Structure):
    """ptam_map_outlier: one outlier measurement with the action the host applies"""
    _fields_ = [("point", C.c_int32), ("kf", C.c_int32), ("action", C.c_int32), ("meas", C.c_int32)]


class MapBaResult(C.Structure):
    """ptam_map_ba_result (MapMaker::BundleAdjust, src/MapMaker.cc:838-933)"""
    _fields_ = [(f, C.c_int32) for f in ("ran", "accepted", "converged", "n_adjust", "n_fixed", "n_points", "n_meas", "n_outliers")]


PLANE_OK, PLANE_TOO_FEW, PLANE_DEGENERATE = range(3)


class PlaneOpts(C.Structure):
    """ptam_plane_opts (MapMaker::CalcPlaneAligner, src/MapMaker.cc:1100-1195)"""
    _fields_ = [("max_dist", C.c_double), ("trials", C.c_int32), ("seed", C.c_uint64), ("samples", C.POINTER(C.c_int32))]


class PlaneInfo(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_points", C.c_int32), ("n_inliers", C.c_int32), ("best_trial", C.c_int32),
                ("trials_skipped", C.c_int32), ("pad_", C.c_int32), ("best_score", C.c_double), ("mean", C.c_double * 3),
                ("normal", C.c_double * 3), ("eigenvalues", C.c_double * 3)]


class MapPointSource(C.Structure):
    """ptam_map_point_source (MapPoint::pPatchSourceKF and the _NC vectors, include/MapPoint.h)"""
    _fields_ = [("src_kf", C.c_int32), ("pad_", C.c_int32), ("center_nc", C.c_double * 3), ("one_right_nc", C.c_double * 3),
                ("one_down_nc", C.c_double * 3)]


class SceneDepth(C.Structure):
    """ptam_scene_depth (MapMaker::RefreshSceneDepth, src/MapMaker.cc:1202-1219)"""
    _fields_ = [("depth_mean", C.c_double), ("depth_sigma", C.c_double), ("n_meas", C.c_int32), ("pad_", C.c_int32)]


MAP_REFIND_KEYFRAME, MAP_REFIND_NEW_POINTS, MAP_REFIND_FAILURE_QUEUE = range(3)


class MapRefindPoint(C.Structure):
    """ptam_map_refind_point (MapPoint: the pixel vectors, pPatchSourceKF as an index, nSourceLevel, irCenter, bBad)"""
    _fields_ = [("pv", PvsPoint), ("src_kf", C.c_int32), ("src_level", C.c_int32), ("center_x", C.c_int32), ("center_y", C.c_int32),
                ("bad", C.c_int32), ("pad_", C.c_int32)]


class MapPair(C.Structure):
    """ptam_map_pair: one entry of sNeverRetryKFs / mvFailureQueue as table indices"""
    _fields_ = [("kf", C.c_int32), ("point", C.c_int32)]


class MapRefindOpts(C.Structure):
    _fields_ = [("max_pairs_per_pass", C.c_int32), ("pad_", C.c_int32)]


class MapRefindResult(C.Structure):
    """ptam_map_refind_result (MapMaker::ReFind*, src/MapMaker.cc:1028-1081)"""
    _fields_ = [(f, C.c_int32) for f in ("n_pairs", "n_skipped", "n_found", "n_never", "n_bad_points", "n_template_kept",
                                         "points_consumed", "stopped")]


class MapOutliersResult(C.Structure):
    """ptam_map_outliers_result (the outlier loop of MapMaker::BundleAdjust, src/MapMaker.cc:916-932)"""
    _fields_ = [(f, C.c_int32) for f in ("n_point_bad", "n_failure_added", "n_never_added", "n_meas_out", "n_never_out", "n_failure_out")]


MAP_MAX_COLUMNS = 8


class MapColumn(C.Structure):
    """ptam_map_column: one point-side table of ptam_map_handle_bad_points, one row of row_bytes per point"""
    _fields_ = [("data", C.c_void_p), ("row_bytes", C.c_int32), ("pad_", C.c_int32)]


class MapBadPointsResult(C.Structure):
    """ptam_map_bad_points_result (MapMaker::HandleBadPoints, src/MapMaker.cc:131-153)"""
    _fields_ = [(f, C.c_int32) for f in ("n_marked", "n_removed", "n_kept", "n_meas_out", "n_never_out", "n_new_out", "n_new_dropped",
                                         "n_failure_out")]


# the tables of a ptam_rmap, as ptam_rmap_download and ptam_rmap_last_refusal name them
(RMAP_KF_POSES, RMAP_KF_FIXED, RMAP_POINTS3, RMAP_REFIND_POINTS, RMAP_SOURCES, RMAP_BAD, RMAP_OUTLIER_COUNT, RMAP_INLIER_COUNT, RMAP_MEAS,
 RMAP_NEVER, RMAP_NEW_QUEUE, RMAP_FAILURE) = range(12)
RMAP_TABLES = RMAP_OUTLIERS = 12
RMAP_WORD_BYTES = 64
RMAP_KF_RECORD_BYTES = 512


class RmapCounts(C.Structure):
    """ptam_rmap_counts_t"""
    _fields_ = [(f, C.c_int32) for f in ("n_kf", "n_points", "n_meas", "n_never", "n_new", "n_failure")]


class MapKfRow(C.Structure):
    """ptam_map_kf_row: one measurement of a keyframe that ptam_rmap_add_keyframe appends"""
    _fields_ = [("point", C.c_int32), ("level", C.c_int32), ("root_pos", C.c_double * 2)]


class RmapInsertOpts(C.Structure):
    """ptam_rmap_insert_opts"""
    _fields_ = [("epipolar", EpipolarOpts), ("refind", MapRefindOpts), ("target_kf", C.c_int32), ("skip_refind", C.c_int32),
                ("skip_points", C.c_int32)]


class RmapInsertResult(C.Structure):
    """ptam_rmap_insert_result (MapMaker::AddKeyFrameFromTopOfQueue, src/MapMaker.cc:493-518)"""
    _fields_ = [("kf", C.c_int32), ("target_kf", C.c_int32), ("target_dist", C.c_double), ("refind", MapRefindResult),
                ("first_point", C.c_int32), ("n_made", C.c_int32), ("levels", EpipolarLevelStats * 4)]


INIT_MAP_OK, INIT_MAP_NO_HOMOGRAPHY, INIT_MAP_ZERO_BASELINE, INIT_MAP_TOO_FEW_POINTS, INIT_MAP_STOPPED = range(5)


class RmapInitOpts(C.Structure):
    """ptam_rmap_init_opts (MapMaker::InitFromStereo, src/MapMaker.cc:268-405)"""
    _fields_ = [("homography", HomographyOpts), ("wiggle_scale", C.c_double), ("subpix_max_its", C.c_int32), ("first_bundles", C.c_int32),
                ("max_bundles", C.c_int32), ("pad_", C.c_int32), ("ba", BaOpts), ("epipolar", EpipolarOpts), ("plane", PlaneOpts)]


class RmapInitResult(C.Structure):
    """ptam_rmap_init_result"""
    _fields_ = [("status", C.c_int32), ("n_matches", C.c_int32), ("homography", HomographyInfo), ("baseline", C.c_double),
                ("n_made", C.c_int32), ("n_subpix_failed", C.c_int32), ("n_behind_camera", C.c_int32), ("n_template_bad", C.c_int32),
                ("n_bundles", C.c_int32), ("n_accepted", C.c_int32), ("n_outliers", C.c_int32), ("n_outlier_bundles", C.c_int32),
                ("converged", C.c_int32), ("pad_", C.c_int32), ("depth", SceneDepth * 2), ("wiggle_scale_depth_normalized", C.c_double),
                ("first_epipolar_point", C.c_int32), ("n_epipolar", C.c_int32), ("levels", EpipolarLevelStats * 4), ("plane", PlaneInfo),
                ("se3_aligner", C.c_double * 12), ("tracker_pose", C.c_double * 12), ("counts", RmapCounts)]


class MapPublishResult(C.Structure):
    """ptam_map_publish_result"""
    _fields_ = [("generation", C.c_int64), ("map_id", C.c_int64), ("n_points", C.c_int32), ("n_kf", C.c_int32), ("grew", C.c_int32),
                ("pad_", C.c_int32)]


class MapTakeResult(C.Structure):
    """ptam_map_take_result"""
    _fields_ = [("changed", C.c_int32), ("n_points", C.c_int32), ("n_carried", C.c_int32), ("n_new", C.c_int32), ("n_dropped", C.c_int32),
                ("link_bytes", C.c_int32), ("generation", C.c_int64), ("map_id", C.c_int64)]


class MapSnapshotInfo(C.Structure):
    """ptam_map_snapshot_info_t"""
    _fields_ = [("generation", C.c_int64), ("map_id", C.c_int64), ("n_points", C.c_int32), ("pad_", C.c_int32)]


class SnapshotKeyframesInfo(C.Structure):
    """ptam_snapshot_keyframes_info_t"""
    _fields_ = [("generation", C.c_int64), ("map_id", C.c_int64), ("epoch", C.c_int64), ("enabled", C.c_int32), ("max_keyframes", C.c_int32),
                ("n_kf", C.c_int32), ("n_made", C.c_int32), ("sbi_w", C.c_int32), ("sbi_h", C.c_int32), ("blur", C.c_double)]


class KeyframesTakeResult(C.Structure):
    """ptam_keyframes_take_result"""
    _fields_ = [("changed", C.c_int32), ("n_kf", C.c_int32), ("n_new", C.c_int32), ("link_bytes", C.c_int32), ("generation", C.c_int64),
                ("map_id", C.c_int64)]


class FrameRecord(C.Structure):
    """ptam_frame_record: one found entry of a tracked frame's iteration set, named by its point's serial"""
    _fields_ = [("serial", C.c_int64), ("level", C.c_int32), ("outlier", C.c_uint8), ("did_subpix", C.c_uint8), ("pad_", C.c_uint8 * 2),
                ("root_pos", C.c_double * 2)]


class FrameReportInfo(C.Structure):
    """ptam_frame_report_info_t"""
    _fields_ = [("map_id", C.c_int64), ("tag", C.c_int64), ("n_records", C.c_int32), ("n_entries", C.c_int32), ("n_outliers", C.c_int32),
                ("pad_", C.c_int32)]


class TrackReportInfo(C.Structure):
    """ptam_track_report_info (ptam_track_frames_report_batch)"""
    _fields_ = [("report", FrameReportInfo), ("report_in_chain", C.c_int32), ("report_too_small", C.c_int32)]


class TrackmapOpts(C.Structure):
    """ptam_trackmap_opts"""
    _fields_ = [("try_coarse", C.c_int32), ("coarse_min", C.c_uint32), ("coarse_max", C.c_uint32), ("coarse_range", C.c_uint32),
                ("coarse_subpix_its", C.c_int32), ("max_patches", C.c_int32), ("estimator", C.c_int32), ("pad_", C.c_int32)]


class TrackmapResult(C.Structure):
    """ptam_trackmap_result"""
    _fields_ = [("pose", C.c_double * 12), ("did_coarse", C.c_int32), ("n_pvs", C.c_int32 * 4), ("attempted", C.c_int32 * 4),
                ("found", C.c_int32 * 4), ("n_coarse", C.c_int32), ("n_top", C.c_int32), ("n_fine", C.c_int32), ("n_meas", C.c_int32),
                ("depth_n", C.c_int32), ("templates_reused", C.c_int32), ("pad_", C.c_int32), ("depth_sum", C.c_double),
                ("depth_sum_sq", C.c_double)]


class TrackmapMeas(C.Structure):
    """ptam_trackmap_meas"""
    _fields_ = [("point", C.c_int32), ("level", C.c_int32), ("found", C.c_int32), ("did_subpix", C.c_int32), ("outlier", C.c_int32),
                ("pad_", C.c_int32), ("v2_found", C.c_double * 2)]


class RmapNoteResult(C.Structure):
    """ptam_rmap_note_result"""
    _fields_ = [("n_records", C.c_int32), ("n_gone", C.c_int32)]


MM_RAN, MM_IDLE, MM_RESET, MM_INIT = range(4)
(MM_STAGE_BUNDLE_RECENT, MM_STAGE_REFIND_NEW, MM_STAGE_BUNDLE_ALL, MM_STAGE_REFIND_FAILURE, MM_STAGE_NOTES, MM_STAGE_BAD_POINTS,
 MM_STAGE_ADD_KEYFRAME, MM_STAGE_PUBLISH, MM_STAGE_INIT) = (1 << i for i in range(9))
MM_INIT_NONE, MM_INIT_PENDING, MM_INIT_DONE = range(3)   # ptam_mapmaker_init_poll


class MapmakerOpts(C.Structure):
    """ptam_mapmaker_opts"""
    _fields_ = [("ba", BaOpts), ("refind", MapRefindOpts), ("insert", RmapInsertOpts), ("failure_period", C.c_int32),
                ("failure_seed", C.c_uint64)]


class MapmakerStepResult(C.Structure):
    """ptam_mapmaker_step_result (one iteration of MapMaker::run(), src/MapMaker.cc:57-114)"""
    _fields_ = [("status", C.c_int32), ("stages", C.c_int32), ("recent", MapBaResult), ("recent_outliers", MapOutliersResult),
                ("refind_new", MapRefindResult), ("all", MapBaResult), ("all_outliers", MapOutliersResult),
                ("refind_failure", MapRefindResult), ("notes", RmapNoteResult), ("bad_points", MapBadPointsResult),
                ("insert", RmapInsertResult), ("insert_rows", C.c_int32), ("insert_gone", C.c_int32), ("publish", MapPublishResult),
                ("converged_recent", C.c_int32), ("converged_full", C.c_int32), ("queue_size", C.c_int32), ("pad_", C.c_int32),
                ("draws", C.c_uint64)]


class SbiAlignment(C.Structure):
    """ptam_sbi_alignment (SmallBlurryImage::CalcSBIRotation, src/ImageProcess.cc:313-495)"""
    _fields_ = [("se2_rot", C.c_double * 4), ("se2_trans", C.c_double * 2), ("score", C.c_double), ("mean_offset", C.c_double),
                ("rotation", C.c_double * 9), ("iterations_done", C.c_int32), ("n_used", C.c_int32), ("degenerate", C.c_int32),
                ("pad_", C.c_int32)]


class TrackFrameInfo(C.Structure):
    """ptam_track_frame_info (ptam_track_frames_batch): the pose TrackMap started from, the alignment, the heuristics as applied"""
    _fields_ = [("pose_in", C.c_double * 12), ("align", SbiAlignment), ("try_coarse", C.c_int32), ("coarse_max", C.c_uint32),
                ("coarse_range", C.c_uint32), ("pad_", C.c_int32)]


class RelocResult(C.Structure):
    """ptam_reloc_result (Relocaliser::AttemptRecovery, src/Relocaliser.cc:12-38)"""
    _fields_ = [("best", C.c_int32), ("good", C.c_int32), ("best_ssd", C.c_double), ("pose", C.c_double * 12), ("align", SbiAlignment)]


TRACK_BAD, TRACK_GOOD = 0, 1
FRAME_TRACKED, FRAME_RECOVERED, FRAME_RECOVERY_FAILED = 0, 1, 2


class TrackState(C.Structure):
    """ptam_track_state: the motion model with mnLostFrames, mTrackingQuality, mnFrame, mnLastKeyFrameDropped"""
    _fields_ = [("model", MotionModel), ("lost_frames", C.c_int32), ("quality", C.c_int32), ("frame", C.c_int32),
                ("last_keyframe_dropped", C.c_int32)]


class TrackStateOpts(C.Structure):
    """ptam_track_state_opts (AssessTrackingQuality, IsNeedNewKeyFrame, the relocaliser's tunables)"""
    _fields_ = [("quality_good", C.c_double), ("quality_lost", C.c_double), ("wiggle_scale", C.c_double),
                ("wiggle_scale_depth_normalized", C.c_double), ("max_kf_dist_wiggle_mult", C.c_double), ("reloc_blur", C.c_double),
                ("reloc_max_score", C.c_double)]


class TrackFrameStateInfo(C.Structure):
    """ptam_track_frame_state_info (ptam_track_frames_recover_batch)"""
    _fields_ = [("branch", C.c_int32), ("closest_kf", C.c_int32), ("closest_kf_dist", C.c_double), ("need_new_keyframe", C.c_int32),
                ("want_keyframe", C.c_int32), ("frame", TrackFrameInfo), ("reloc", RelocResult)]


class CameraTrackerOpts(C.Structure):
    """ptam_camera_tracker_opts"""
    _fields_ = [("max_points", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("max_keyframes", C.c_int32),
                ("trackmap", TrackmapOpts), ("state", TrackStateOpts), ("use_rotation_estimator", C.c_int32), ("keyframe_gap", C.c_int32),
                ("rotation_blur", C.c_double), ("shuffle_seed", C.c_uint64), ("tag_base", C.c_int64), ("max_queue", C.c_int32),
                ("reports", C.c_int32), ("keyframes", C.c_int32), ("pad_", C.c_int32)]


TRAIL_TRACKING_NOT_STARTED, TRAIL_TRACKING_STARTED, TRAIL_TRACKING_COMPLETE = range(3)   # mnInitialStage


class CameraSessionOpts(C.Structure):
    """ptam_camera_session_opts"""
    _fields_ = [("max_initial_trails", C.c_int32), ("min_good_trails", C.c_int32), ("min_shi_tomasi", C.c_double), ("init", RmapInitOpts)]


class CameraSessionResult(C.Structure):
    """ptam_camera_session_result"""
    _fields_ = [("stage_before", C.c_int32), ("stage_after", C.c_int32), ("poked", C.c_int32), ("n_trails", C.c_int32),
                ("n_good", C.c_int32), ("n_alive", C.c_int32), ("trail_reset", C.c_int32), ("init_requested", C.c_int32),
                ("init_done", C.c_int32), ("init_status", C.c_int32), ("tracked", C.c_int32), ("pad_", C.c_int32), ("init_tag", C.c_int64)]


class CameraTrackResult(C.Structure):
    """ptam_camera_track_result"""
    _fields_ = [("track", TrackmapResult), ("info", TrackFrameStateInfo), ("report", FrameReportInfo), ("map_take", MapTakeResult),
                ("keyframes_take", KeyframesTakeResult), ("added_keyframe", C.c_int32), ("noted_frame", C.c_int32),
                ("report_in_chain", C.c_int32), ("queue_size", C.c_int32), ("tag", C.c_int64)]


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_size_t, C.c_void_p)


class CalibCorner(C.Structure):
    """ptam_calib_corner (CalibGridCorner: irGridPos, Params.v2Pos; include/CalibImage.h)"""
    _fields_ = [("gx", C.c_int32), ("gy", C.c_int32), ("u", C.c_double), ("v", C.c_double)]


class CalibResult(C.Structure):
    """ptam_calib_result (CameraCalibrator::OptimizeOneStep, src/CameraCalibrator.cc:215-269)"""
    _fields_ = [("status", C.c_int32), ("n_measurements", C.c_int32), ("steps", C.c_int32), ("pad_", C.c_int32),
                ("params", C.c_double * 5), ("rms", C.c_double), ("pixel_aspect_ratio", C.c_double)]


CALIB_OK, CALIB_NO_MEASUREMENTS = 0, 1
CALIB_GUESS_OK, CALIB_GUESS_REFUSED = 0, 1
CALIB_MAX_IMAGES, CALIB_MAX_CORNERS, CALIB_MAX_STEPS = 65536, 4194304, 65536

# include/ptam_hip_bench.h: the stages of ptam_tracker_stage_time, the lists of ptam_ba_debug_lists, the bits of ptam_ba_solve_plan
(TS_PYR_PVS, TS_DETECT, TS_COMPACT_SELECT, TS_SEARCH_COARSE, TS_GATHER_COARSE, TS_POSE_COARSE, TS_SEARCH_FINE, TS_GATHER_FINE, TS_POSE_FINE,
 TS_COUNT) = range(10)
(BL_COUNTS, BL_ROWPTR, BL_M_CAM, BL_M_PT, BL_M_ORIG, BL_M_FIDX, BL_M_FOUND, BL_M_S, BL_PT_ORIG, BL_POINTS, BL_CHUNKS, BL_S_ENTRIES, BL_S_SEGS,
 BL_S_WG_SEG, BL_S_PAIR_BEGIN, BL_S_WG_HEAD, BL_CAM_PTR, BL_CAM_MEAS) = range(18)
(SP_SMALL, SP_CHAIN_FWD_INV, SP_CHAIN_BW_IN_LAUNCH, SP_CHAIN_SEPARATE_BW, SP_STEPS, SP_TWO_CHAINS, SP_TWIN_STEPS, SP_MID_CHAIN, SP_MID_STEPS,
 SP_BW_TWO_WG, SP_BW_GLOBAL) = (1 << i for i in range(11))
SOLVE_PER_COLUMN, SOLVE_POISON_UPPER = 1, 2

_vp, _i, _d = C.c_void_p, C.c_int, C.c_double
_pd, _pi, _pu8 = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
_ppv = C.POINTER(C.c_void_p)

# name -> (restype, argtypes).  Names are given WITHOUT the prefix.
PROTOTYPES = {
    "last_error": (C.c_char_p, []),
    "device_count": (_i, [C.POINTER(_i)]),
    "ctx_create": (_i, [C.POINTER(CamParams), _i, _ppv]),
    "ctx_destroy": (_i, [_vp]),
    "ctx_set_halfsample": (_i, [_vp, _i]),
    "ctx_sync": (_i, [_vp]),
    "ctx_stream": (_vp, [_vp]),
    "ctx_camera_constants": (_i, [_vp, _pd]),
    "dev_alloc": (_i, [_vp, C.c_size_t, _ppv]),
    "dev_free": (_i, [_vp, _vp]),
    "dev_upload": (_i, [_vp, _vp, _vp, C.c_size_t]),
    "dev_download": (_i, [_vp, _vp, _vp, C.c_size_t]),
    "kf_create": (_i, [_vp, _i, _i, _ppv]),
    "kf_destroy": (_i, [_vp]),
    "make_keyframe_lite": (_i, [_vp, _vp, _vp, _i]),
    "make_keyframe_lite_dev": (_i, [_vp, _vp, _vp]),
    "kf_clone": (_i, [_vp, _vp, _ppv]),
    "kf_copy": (_i, [_vp, _vp, _vp]),
    "kf_level_info": (_i, [_vp, _vp, _i, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
    "kf_read_level": (_i, [_vp, _vp, _i, _vp, _vp, _vp]),
    "make_keyframe_rest": (_i, [_vp, _vp]),
    "kf_rest_info": (_i, [_vp, _vp, _i, C.POINTER(_i)]),
    "kf_read_rest": (_i, [_vp, _vp, _i, _vp, _vp]),
    "find_patch_coarse_batch": (_i, [_vp, _vp, _i, _vp, _vp, _vp]),
    "find_patch_coarse_batch_dev": (_i, [_vp, _vp, _i, _vp, _vp, _vp]),
    "zmssd_at_points": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp]),
    "project_points": (_i, [_vp, _i, _vp, _pd, _vp]),
    "subpix_batch": (_i, [_vp, _vp, _i, _vp, _vp, _vp]),
    "make_templates_batch": (_i, [_vp, _i, _vp, _vp, _vp]),
    "kf_implane_corners": (_i, [_vp, _vp, _i, _vp, _i, _vp]),
    "epipolar_search_batch": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp]),
    "ctx_one_pixel_dist": (_i, [_vp, _pd]),
    "ctx_cache_hazards": (_i, [_vp, C.POINTER(C.c_longlong)]),
    "track_pvs": (_i, [_vp, _i, _vp, _pd, _vp, _vp]),
    "gn_opts_default": (None, [C.POINTER(GnOpts)]),
    "pose_gn": (_i, [_vp, _i, _vp, _vp, _pd, C.POINTER(GnOpts), _vp, _vp]),
    "pose_gn_dev": (_i, [_vp, _i, _vp, _vp, _vp, C.POINTER(GnOpts), _vp, _vp]),
    "pose_gn_dev_counted": (_i, [_vp, _i, _vp, _vp, _vp, _vp, C.POINTER(GnOpts), _vp, _vp, _pd, _pd]),
    "gather_pose_meas_dev": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "calc_pose_update": (_i, [_vp, _i, _vp, _d, _i, _d, _pd, _vp]),
    "ba_opts_default": (None, [C.POINTER(BaOpts)]),
    "ba_create": (_i, [_vp, C.POINTER(BaOpts), _ppv]),
    "ba_destroy": (_i, [_vp]),
    "ba_add_camera": (_i, [_vp, _pd, _i]),
    "ba_add_point": (_i, [_vp, _pd]),
    "ba_add_meas": (_i, [_vp, _i, _i, _pd, _d]),
    "ba_add_cameras": (_i, [_vp, _i, _vp, _vp]),
    "ba_add_points": (_i, [_vp, _i, _vp]),
    "ba_add_measurements": (_i, [_vp, _i, _vp, _vp, _vp, _vp]),
    "ba_compute": (_i, [_vp, _vp, C.POINTER(_i)]),
    "ba_converged": (_i, [_vp]),
    "ba_get_point": (_i, [_vp, _i, _pd]),
    "ba_get_camera": (_i, [_vp, _i, _pd]),
    "ba_get_all": (_i, [_vp, _vp, _vp]),
    "ba_get_outliers": (_i, [_vp, _vp, _i]),
    "ba_get_trials": (_i, [_vp, _vp, _i]),
    "ba_counts": (_i, [_vp, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
    "ba_solve_fallbacks": (_i, [_vp]),
    "ba_duplicates_refused": (_i, [_vp]),
    "ba_set_profiling": (_i, [_vp, _i]),
    "ba_kernel_time": (_i, [_vp, _i, _pd, C.POINTER(_i)]),
    "ba_prepare": (_i, [_vp]),
    "ba_bench_jacobian": (_i, [_vp, _i, _pd, _pd]),
    "reproject_points": (_i, [_vp, _i, _vp, _pd, _vp]),
    "refind_batch": (_i, [_vp, _vp, _pd, _i, _vp, _vp, _vp]),
    "refinder_create": (_i, [_vp, C.POINTER(_vp)]),
    "refinder_destroy": (_i, [_vp]),
    "refind_pairs": (_i, [_vp, _vp, _i, _vp, _vp, _vp]),
    "epipolar_opts_default": (None, [C.POINTER(EpipolarOpts)]),
    "add_map_points_epipolar": (_i, [_vp, _vp, _pd, _vp, _pd, C.POINTER(EpipolarOpts), _i, _vp, _vp, _vp, _i, C.POINTER(C.c_int32), _vp]),
    "trails_create": (_i, [_vp, _i, _ppv]),
    "trails_destroy": (_i, [_vp]),
    "trails_start": (_i, [_vp, _vp, _d, _i, C.POINTER(_i)]),
    "trails_advance": (_i, [_vp, _vp, C.POINTER(_i), C.POINTER(_i)]),
    "trails_advance_batch": (_i, [_i, _vp, _vp, _vp, _vp, _vp]),
    "trails_read": (_i, [_vp, _vp, _i, C.POINTER(_i)]),
    "trails_read_patches": (_i, [_vp, _vp, _i, C.POINTER(_i)]),
    "trails_matches": (_i, [_vp, _vp, _i, C.POINTER(_i)]),
    "homography_opts_default": (None, [C.POINTER(HomographyOpts)]),
    "homography_samples": (_i, [C.c_uint64, _i, _i, _vp]),
    "homography_init": (_i, [_vp, _i, _vp, C.POINTER(HomographyOpts), _pd, C.POINTER(HomographyInfo), _vp]),
    "trails_homography": (_i, [_vp, C.POINTER(HomographyOpts), _pd, C.POINTER(HomographyInfo), _vp]),
    "init_points_from_trails": (_i, [_vp, _vp, _vp, _pd, _i, _vp, _i, _vp, _vp, C.POINTER(C.c_int32)]),
    "pose_gn_state": (_i, [_vp, _i, _vp, _vp, _pd, _vp, _vp, _vp, _vp]),
    "trackmap_opts_default": (None, [_vp]),
    "tracker_create": (_i, [_vp, _i, _ppv]),
    "tracker_destroy": (_i, [_vp]),
    "tracker_set_map": (_i, [_vp, _i, _vp, _vp]),
    "tracker_update_map": (_i, [_vp, _i, _vp, _vp, _vp]),
    "tracker_set_shuffle": (_i, [_vp, _vp, _vp]),
    "tracker_draw_shuffles": (_i, [_vp, C.c_uint64, C.c_uint64]),
    "tracker_read_shuffle": (_i, [_vp, _vp, _vp]),
    "shuffle_order_host": (_i, [C.c_uint64, C.c_uint64, _i, _i, _vp]),
    "track_map": (_i, [_vp, _vp, _pd, _vp, _vp]),
    "track_map_frame": (_i, [_vp, _vp, _vp, _pd, _vp, _vp]),
    "motion_reset": (None, [C.POINTER(MotionModel), _pd]),
    "motion_predict": (None, [C.POINTER(MotionModel)]),
    "motion_update": (None, [C.POINTER(MotionModel), _vp]),
    "se3_exp": (None, [_vp, _vp]),
    "se3_ln": (None, [_vp, _vp]),
    "track_frame": (_i, [_vp, _vp, _vp, C.POINTER(MotionModel), _vp, _vp]),
    "sbi_create": (_i, [_vp, _i, _i, _ppv]),
    "sbi_destroy": (_i, [_vp]),
    "sbi_make": (_i, [_vp, _vp, _d]),
    "sbi_size": (_i, [_vp, C.POINTER(_i), C.POINTER(_i)]),
    "sbi_read": (_i, [_vp, _vp, _vp, _vp]),
    "sbi_calc_rotation": (_i, [_vp, _vp, _i, C.POINTER(SbiAlignment)]),
    "sbi_bank_create": (_i, [_vp, _i, _i, _i, _ppv]),
    "sbi_bank_destroy": (_i, [_vp]),
    "sbi_bank_add": (_i, [_vp, _vp, _d, C.POINTER(_i)]),
    "sbi_bank_add_batch": (_i, [_vp, _i, _vp, _d, C.POINTER(_i)]),
    "sbi_bank_count": (_i, [_vp, C.POINTER(_i)]),
    "relocalise": (_i, [_vp, _vp, _vp, _vp, _d, _d, C.POINTER(RelocResult), _vp]),
    "rotation_estimator_create": (_i, [_vp, _i, _i, _d, _ppv]),
    "rotation_estimator_destroy": (_i, [_vp]),
    "rotation_estimator_reset": (_i, [_vp]),
    "motion_predict_sbi": (None, [C.POINTER(MotionModel), _pd]),
    "motion_recover": (None, [C.POINTER(MotionModel), _pd]),
    "track_frame_sbi": (_i, [_vp, _vp, _vp, C.POINTER(MotionModel), _vp, _vp, _vp, C.POINTER(SbiAlignment)]),
    "bench_track_sequence": (_i, [_vp, _vp, _i, _vp, C.POINTER(MotionModel), _vp, _vp, _vp, _i, _vp, _pd, _pd]),
    "tracker_set_profiling": (_i, [_vp, _i]),
    "tracker_stage_time": (_i, [_vp, _i, _pd, C.POINTER(_i)]),
    "bench_track_frames": (_i, [_i, _vp, _vp, _vp, _pd, _vp, _vp, _vp, _i, _pd]),
    "track_map_frames_batch": (_i, [_i, _vp, _vp, _vp, _pd, _vp, _vp]),
    "track_frames_batch": (_i, [_i, _vp, _vp, _vp, C.POINTER(MotionModel), _vp, _vp, _vp, C.POINTER(TrackFrameInfo)]),
    "motion_predict_sbi_dev": (_i, [_vp, _i, C.POINTER(MotionModel), _pd, _pd]),
    "track_state_reset": (None, [C.POINTER(TrackState), _pd]),
    "track_state_opts_default": (None, [C.POINTER(TrackStateOpts)]),
    "assess_tracking_quality": (None, [C.POINTER(TrackState), _vp, _vp, _d, C.POINTER(TrackStateOpts)]),
    "sbi_bank_set_poses": (_i, [_vp, _i, _i, _vp]),
    "sbi_bank_poses": (_i, [_vp, _i, _i, _vp]),
    "tracker_read_reloc_ssd": (_i, [_vp, _i, _i, _pd]),
    "track_frames_recover_batch": (_i, [_i, _vp, _vp, _vp, C.POINTER(TrackState), _vp, _vp, _vp, _vp, C.POINTER(TrackStateOpts), _vp,
                                        C.POINTER(TrackFrameStateInfo)]),
    "track_frames_report_batch": (_i, [_i, _vp, _vp, _vp, C.POINTER(TrackState), _vp, _vp, _vp, _vp, C.POINTER(TrackStateOpts), _vp,
                                       C.POINTER(TrackFrameStateInfo), _vp, _vp, _vp, C.POINTER(TrackReportInfo)]),
    "camera_tracker_opts_default": (_i, [C.POINTER(CameraTrackerOpts)]),
    "camera_tracker_create": (_i, [_vp, C.POINTER(CameraTrackerOpts), _vp, _vp, _ppv]),
    "camera_tracker_destroy": (_i, [_vp]),
    "camera_tracker_reset": (_i, [_vp, _pd]),
    "camera_tracker_state": (_i, [_vp, C.POINTER(TrackState)]),
    "camera_tracker_tracker": (_vp, [_vp]),
    "camera_tracker_current_keyframe": (_vp, [_vp]),
    "camera_tracker_last_report": (_vp, [_vp]),
    "camera_tracker_pool": (_i, [_vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "camera_tracker_track_frames": (_i, [_i, _vp, _vp, C.POINTER(CameraTrackResult)]),
    "camera_session_opts_default": (_i, [C.POINTER(CameraSessionOpts)]),
    "camera_tracker_enable_session": (_i, [_vp, C.POINTER(CameraSessionOpts)]),
    "camera_tracker_restart": (_i, [_vp]),
    "camera_tracker_session_frames": (_i, [_i, _vp, _vp, _vp, C.POINTER(CameraTrackResult), C.POINTER(CameraSessionResult)]),
    "camera_tracker_trails": (_vp, [_vp]),
    "camera_tracker_init_result": (_i, [_vp, C.POINTER(RmapInitResult)]),
    "camera_tracker_stage": (_i, [_vp, C.POINTER(C.c_int32)]),
    "bench_track_batch": (_i, [_i, _vp, _vp, _vp, _pd, _vp, _vp, _vp, _i, _i, _pd]),
    "tracker_read_iteration_set": (_i, [_vp, _vp, _i, C.POINTER(_i)]),
    "ba_bench_jacobian_rotating": (_i, [_vp, _i, _i, _pd]),
    "ba_schur_index_map": (_i, [_i, _vp, _i]),
    "ba_debug_lists": (_i, [_vp, _i, _vp, C.c_size_t]),
    "ba_solve_plan": (_i, [_i, _i, _i]),
    "ba_debug_solve": (_i, [_vp, _vp, _vp, _i, _vp, _pd, _vp, C.POINTER(_i)]),
    "ba_set_comm": (_i, [_vp, _i, _i, ALLREDUCE_FN, _vp]),
    "map_bundle_adjust": (_i, [_vp, C.POINTER(BaOpts), _i, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, C.POINTER(MapBaResult), _vp, _i, _vp, _vp]),
    "plane_opts_default": (None, [C.POINTER(PlaneOpts)]),
    "plane_samples": (_i, [C.c_uint64, _i, _i, _vp]),
    "calc_plane_aligner": (_i, [_vp, _i, _vp, C.POINTER(PlaneOpts), _pd, C.POINTER(PlaneInfo), _vp]),
    "map_apply_global_transform": (_i, [_vp, _pd, _i, _vp, _i, _vp, _vp, _vp]),
    "map_align_to_plane": (_i, [_vp, C.POINTER(PlaneOpts), _i, _vp, _i, _vp, _vp, _vp, _pd, C.POINTER(PlaneInfo), _vp]),
    "map_scene_depth": (_i, [_vp, _i, _vp, _i, _vp, _i, _vp, _vp]),
    "map_refind": (_i, [_vp, _vp, C.POINTER(MapRefindOpts), _i, _i, _vp, _vp, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _vp,
                        C.POINTER(MapRefindResult), _vp, _vp, _vp, _i, _vp, _vp]),
    "map_apply_outliers": (_i, [_vp, _i, _i, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _vp, C.POINTER(MapOutliersResult), _vp, _vp, _vp]),
    "map_handle_bad_points": (_i, [_vp, _i, _i, _vp, _vp, _vp, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _i, _vp, C.POINTER(MapBadPointsResult),
                                   _vp, _vp, _vp, _vp, _vp, _vp]),
    "map_add_points": (_i, [_vp, _i, _i, _i, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "rmap_create": (_i, [_vp, _ppv]),
    "rmap_destroy": (_i, [_vp]),
    "rmap_reserve": (_i, [_vp, _i, _i, _i, _i, _i, _i]),
    "rmap_counts": (_i, [_vp, C.POINTER(RmapCounts)]),
    "rmap_upload": (_i, [_vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _i, _vp, _i, _vp]),
    "rmap_download": (_i, [_vp, _i, _i, _i, _vp]),
    "rmap_last_refusal": (_i, [_vp, C.POINTER(_i), C.POINTER(_i)]),
    "rmap_traffic": (_i, [_vp, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]),
    "rmap_bundle_adjust": (_i, [_vp, C.POINTER(BaOpts), _i, _vp, C.POINTER(MapBaResult), _vp, _i, _vp, _vp]),
    "rmap_refind": (_i, [_vp, _vp, C.POINTER(MapRefindOpts), _i, _i, _vp, _vp, C.POINTER(MapRefindResult), _vp, _vp, _vp, _i]),
    "rmap_refind_queue": (_i, [_vp, _vp, C.POINTER(MapRefindOpts), _i, _vp, C.POINTER(MapRefindResult)]),
    "rmap_apply_global_transform": (_i, [_vp, _pd, _vp]),
    "rmap_apply_outliers": (_i, [_vp, _i, _vp, C.POINTER(MapOutliersResult)]),
    "rmap_bundle_adjust_routed": (_i, [_vp, C.POINTER(BaOpts), _i, _vp, C.POINTER(MapBaResult), C.POINTER(MapOutliersResult)]),
    "rmap_handle_bad_points": (_i, [_vp, C.POINTER(MapBadPointsResult), _vp, _vp]),
    "rmap_add_points": (_i, [_vp, _i, _i, _i, _i, _vp]),
    "rmap_add_keyframe": (_i, [_vp, _vp, _pd, _i, _i, _vp]),
    "rmap_note_tracked": (_i, [_vp, _i, _vp, _vp]),
    "rmap_scene_depth": (_i, [_vp, _vp]),
    "rmap_closest_keyframes": (_i, [_vp, _i, _i, _vp, _pd, C.POINTER(C.c_int32)]),
    "rmap_insert_keyframe": (_i, [_vp, _vp, _vp, _pd, _i, _i, _vp, C.POINTER(RmapInsertOpts), C.POINTER(RmapInsertResult)]),
    "rmap_init_opts_default": (_i, [C.POINTER(RmapInitOpts)]),
    "rmap_init_from_stereo": (_i, [_vp, _vp, _vp, _vp, _i, _vp, C.POINTER(RmapInitOpts), _vp, C.POINTER(RmapInitResult)]),
    "rmap_align_to_plane": (_i, [_vp, C.POINTER(PlaneOpts), _pd, C.POINTER(PlaneInfo), _vp]),
    "rmap_clear": (_i, [_vp]),
    "rmap_publish": (_i, [_vp, _vp, C.POINTER(MapPublishResult)]),
    "rmap_point_serials": (_i, [_vp, _i, _i, _vp]),
    "rmap_resolve_serials": (_i, [_vp, _i, _vp, _vp, C.POINTER(C.c_int32)]),
    "map_snapshot_create": (_i, [_vp, _i, _ppv]),
    "map_snapshot_destroy": (_i, [_vp]),
    "map_snapshot_reserve": (_i, [_vp, _i]),
    "map_snapshot_info": (_i, [_vp, C.POINTER(MapSnapshotInfo)]),
    "tracker_take_map": (_i, [_vp, _vp, C.POINTER(MapTakeResult)]),
    "snapshot_keyframes_enable": (_i, [_vp, _i, _d]),
    "snapshot_keyframes_info": (_i, [_vp, C.POINTER(SnapshotKeyframesInfo)]),
    "sbi_bank_take_keyframes": (_i, [_vp, _vp, C.POINTER(KeyframesTakeResult)]),
    "sbi_bank_clear": (_i, [_vp]),
    "sbi_bank_read": (_i, [_vp, _i, _vp, _vp, _vp]),
    "tracker_point_serials": (_i, [_vp, _i, _i, _vp]),
    "tracker_read_iteration_serials": (_i, [_vp, _vp, _i, C.POINTER(_i)]),
    "frame_report_create": (_i, [_vp, _i, _ppv]),
    "frame_report_destroy": (_i, [_vp]),
    "frame_report_info": (_i, [_vp, C.POINTER(FrameReportInfo)]),
    "frame_report_read": (_i, [_vp, _i, _i, _vp]),
    "frame_report_from_host": (_i, [_vp, C.c_int64, _i, _vp, _i, _vp]),
    "tracker_report_frames": (_i, [_i, _vp, _vp, _vp]),
    "rmap_note_reports": (_i, [_vp, _i, _vp, C.POINTER(RmapNoteResult)]),
    "rmap_insert_keyframe_report": (_i, [_vp, _vp, _vp, _pd, _i, _vp, C.POINTER(RmapInsertOpts), C.POINTER(RmapInsertResult),
                                         C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "mapmaker_opts_default": (_i, [C.POINTER(MapmakerOpts)]),
    "mapmaker_create": (_i, [_vp, _vp, _vp, C.POINTER(MapmakerOpts), _ppv]),
    "mapmaker_destroy": (_i, [_vp]),
    "mapmaker_add_keyframe": (_i, [_vp, _vp, _pd, _i, _vp, _d, _d, C.c_int64]),
    "mapmaker_note_frame": (_i, [_vp, _vp, C.c_int64]),
    "mapmaker_queue_size": (_i, [_vp, C.POINTER(C.c_int32)]),
    "mapmaker_request_reset": (_i, [_vp]),
    "mapmaker_reset_done": (_i, [_vp, C.POINTER(C.c_int32)]),
    "mapmaker_request_init": (_i, [_vp, _vp, _vp, _i, _vp, C.POINTER(RmapInitOpts), C.c_int64]),
    "mapmaker_init_poll": (_i, [_vp, C.POINTER(C.c_int32), C.POINTER(RmapInitResult)]),
    "mapmaker_flags": (_i, [_vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "mapmaker_set_flags": (_i, [_vp, _i, _i]),
    "mapmaker_released": (_i, [_vp, _i, _vp, C.POINTER(C.c_int32)]),
    "mapmaker_step": (_i, [_vp, C.POINTER(MapmakerStepResult)]),
    "calib_create": (_i, [_vp, _i, _i, _ppv]),
    "calib_destroy": (_i, [_vp]),
    "calib_reset": (_i, [_vp, _pd, _i]),
    "calib_counts": (_i, [_vp, _pi, _pi]),
    "calib_add_images": (_i, [_vp, _i, _pi, _vp, _pi]),
    "calib_set_poses": (_i, [_vp, _pd]),
    "calib_read_poses": (_i, [_vp, _pd]),
    "calib_optimize": (_i, [_vp, _i, C.POINTER(CalibResult), _pd]),
    "calib_params": (_i, [_vp, _pd]),
    "calib_residuals": (_i, [_vp, _i, _pd, _pi]),
    "rccl_unique_id": (_i, [_vp]),
    "rccl_create": (_i, [_vp, _vp, _i, _i, _ppv]),
    "rccl_destroy": (_i, [_vp]),
    "rccl_allreduce_f64": (_i, [_vp, _pd, C.c_size_t, _vp]),
}

# every symbol include/ptam_hip.h declares (checked by the CPU test-suite against the built .so)
DECLARED = sorted(PROTOTYPES)


class Bound:
    """Attribute access to `<prefix><name>` functions of one shared library."""

    def __init__(self, lib, prefix):
        self.lib, self.prefix = lib, prefix
        self.missing = []
        for name, (res, args) in PROTOTYPES.items():
            try:
                fn = getattr(lib, prefix + name)
            except AttributeError:
                self.missing.append(name)
                continue
            fn.restype, fn.argtypes = res, args
            setattr(self, name, fn)

    def has(self, name):
        return hasattr(self, name)


def bind(lib, prefix):
    return Bound(lib, prefix)
