"""ctypes binding of include/irmv_hip.h (libirmv_hip.so).

Thin by design: every function here is one C-ABI call.  There is no fallback of
any kind -- if the HIP library is missing or a call fails, IrmvError is raised.
"""
from __future__ import annotations

import ctypes as C
import os

from . import _build

OK, ERR_ARG, ERR_HIP, ERR_MODEL = 0, -1, -2, -3
RESIZE_STRETCH, RESIZE_LETTERBOX = 0, 1
ARMOR_SMALL, ARMOR_LARGE = 0, 1
SUBMIT_H2D = 1
SUBMIT_ASYNC_UPLOAD = 2
POINTS_AUTO, POINTS_KEYPOINT_HEAD, POINTS_CLASSICAL, POINTS_REFINED = 0, 1, 2, 3
SRC_HWC8, SRC_BAYER_RGGB8, SRC_BAYER_BGGR8, SRC_BAYER_GRBG8, SRC_BAYER_GBRG8 = 0, 1, 2, 3, 4
BAYER_FORMATS = {"RGGB": SRC_BAYER_RGGB8, "BGGR": SRC_BAYER_BGGR8, "GRBG": SRC_BAYER_GRBG8, "GBRG": SRC_BAYER_GBRG8}
DEMOSAIC_BILINEAR, DEMOSAIC_MHC = 0, 1
DEMOSAIC_ALGOS = {"bilinear": DEMOSAIC_BILINEAR, "mhc": DEMOSAIC_MHC}
VIEW_WINDOW, VIEW_FRAME = 0, 1
VIEWS = {"window": VIEW_WINDOW, "frame": VIEW_FRAME}
NUM_CLASSES = 14
MAX_DET_CAP = 256
CAND_CAP = 8192
MAX_TILES = 16


class IrmvError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"irmv_hip error {code}: {msg}")
        self.code = code


class EngineCfg(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("device", C.c_int32),
        ("src_width", C.c_int32), ("src_height", C.c_int32), ("net_size", C.c_int32),
        ("resize_mode", C.c_int32), ("rotate180", C.c_int32), ("swap_rb", C.c_int32),
        ("score_thr", C.c_float), ("iou_thr", C.c_float),
        ("max_det", C.c_int32), ("pre_nms_cap", C.c_int32), ("num_slots", C.c_int32),
        ("armor_size", C.c_int32),
        ("camera_matrix", C.c_double * 9), ("dist_coeffs", C.c_double * 5),
        ("weights_path", C.c_char_p), ("weights_blob", C.c_void_p), ("weights_bytes", C.c_uint64),
        ("weights_on_device", C.c_int32), ("num_streams", C.c_int32),
        ("point_source", C.c_int32), ("binary_threshold", C.c_int32),
        ("light_min_ratio", C.c_float), ("light_max_ratio", C.c_float), ("light_max_angle", C.c_float), ("reserved0", C.c_float),
        ("armor_min_small_center_distance", C.c_double), ("armor_max_small_center_distance", C.c_double),
        ("armor_min_large_center_distance", C.c_double), ("armor_max_large_center_distance", C.c_double),
        ("src_format", C.c_int32), ("bayer_gain_q8", C.c_uint16 * 3), ("bayer_demosaic", C.c_uint16),
        ("net_height", C.c_int32), ("reserved2", C.c_int32),   # net_height 0: square net_size x net_size input
        ("win_width", C.c_int16), ("win_height", C.c_int16),   # tracking window; 0, 0: none (the struct's former tail padding)
    ]


class Det(C.Structure):
    _fields_ = [
        ("xyxy", C.c_float * 4), ("score", C.c_float), ("class_id", C.c_int32),
        ("anchor", C.c_int32), ("pnp_ok", C.c_int32), ("kpts", C.c_float * 8),
        ("rvec", C.c_double * 3), ("tvec", C.c_double * 3), ("quat", C.c_double * 4),
        ("armor_valid", C.c_int32), ("armor_size", C.c_int32), ("n_lights", C.c_int32), ("reserved", C.c_int32),
    ]


class TileDet(C.Structure):
    """irmv_tile_det (include/irmv_hip.h): a record of the merged list of a tiled step."""
    _fields_ = [("det", Det), ("tile", C.c_int32), ("index", C.c_int32), ("cut", C.c_int32), ("reserved", C.c_int32)]


class RawDets(C.Structure):
    _fields_ = [
        ("num_dets", C.c_int32), ("n_candidates", C.c_int32),
        ("det_boxes", C.POINTER(C.c_float)), ("det_scores", C.POINTER(C.c_float)),
        ("det_classes", C.POINTER(C.c_int32)), ("det_anchors", C.POINTER(C.c_int32)),
        ("det_kpts", C.POINTER(C.c_float)),
    ]


class ClassPolicy(C.Structure):
    """irmv_class_policy (include/irmv_hip.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("score_thr", C.c_float * 16), ("plate", C.c_uint8 * 16)]


POSE_MIN_ERR, POSE_PRIOR = 0, 1
POSE_MODES = {"min_err": POSE_MIN_ERR, "prior": POSE_PRIOR}
NORMAL_UP_ROBOT = -0.25881904510252074   # -sin 15 deg: a plate whose outward normal points 15 degrees upward


class PosePrior(C.Structure):
    """irmv_pose_prior (include/irmv_hip.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("mode", C.c_int32), ("ambiguity_ratio", C.c_double),
                ("normal_up", C.c_double * 16), ("normal_up_default", C.c_double)]


class PoseAlt(C.Structure):
    """irmv_pose_alt (include/irmv_hip.h): the IPPE solution a result record does not report."""
    _fields_ = [("rvec", C.c_double * 3), ("tvec", C.c_double * 3), ("quat", C.c_double * 4),
                ("err", C.c_double), ("err_alt", C.c_double), ("state", C.c_int32), ("alt_ok", C.c_int32)]


RENDER_COLOR, RENDER_BINARY = 0, 1
RENDER_KINDS = {"color": RENDER_COLOR, "binary": RENDER_BINARY}
MARK_BOXES, MARK_LABELS, MARK_ARMORS = 1, 2, 4
MARK_ALL = MARK_BOXES | MARK_LABELS | MARK_ARMORS


class RenderOpts(C.Structure):
    """irmv_render_opts (include/irmv_hip.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("kind", C.c_int32), ("scale", C.c_int32), ("marks", C.c_uint32),
                ("binary_threshold", C.c_int32), ("reserved", C.c_int32 * 3)]


class KernelStat(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("layer", C.c_char * 32), ("flops", C.c_double),
                ("bytes", C.c_double), ("ms", C.c_float), ("reserved", C.c_int32)]


class ConvSeg(C.Structure):
    _fields_ = [("tensor", C.c_char * 32), ("coff", C.c_int32), ("C", C.c_int32), ("shift", C.c_int32)]


class ConvOp(C.Structure):
    _fields_ = [("op", C.c_int32), ("layer", C.c_char * 32),
                ("ks", C.c_int32), ("stride", C.c_int32), ("act", C.c_int32), ("out_f32", C.c_int32),
                ("cin", C.c_int32), ("cout", C.c_int32), ("cout_pad", C.c_int32),
                ("Hin", C.c_int32), ("Win", C.c_int32), ("Hout", C.c_int32), ("Wout", C.c_int32),
                ("s0", ConvSeg), ("s1", ConvSeg), ("res", ConvSeg),
                ("out_tensor", C.c_char * 32), ("out_coff", C.c_int32), ("out_lazy", C.c_int32),
                ("fused", C.c_int32), ("tune_fused", C.c_int32),
                ("fuse_layer", C.c_char * 32), ("fuse_tensor", C.c_char * 32),
                ("fuse_coff", C.c_int32), ("fuse_cout", C.c_int32), ("fuse_cout_pad", C.c_int32), ("reserved", C.c_int32),
                ("kname", C.c_char * 48), ("kname_one", C.c_char * 48)]


class ConvCand(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("mt", C.c_int32), ("nt", C.c_int32), ("flags", C.c_int32), ("ipw", C.c_int32),
                ("forced", C.c_int32), ("reserved", C.c_int32)]


class GraphOp(C.Structure):
    _fields_ = [("op", C.c_int32), ("kind", C.c_char * 16), ("layer", C.c_char * 48), ("kname", C.c_char * 48),
                ("s0", ConvSeg), ("s1", ConvSeg), ("out_tensor", C.c_char * 32), ("out_coff", C.c_int32), ("out_C", C.c_int32),
                ("fused_away", C.c_int32), ("reserved", C.c_int32)]


class OpIo(C.Structure):
    """irmv_op_io (irmv_engine_op_io): the conv ops a fused op stands for, what its launch writes and reads."""
    _fields_ = [("op", C.c_int32), ("n_sub", C.c_int32), ("sub", C.c_int32 * 4), ("n_writes", C.c_int32), ("n_reads", C.c_int32),
                ("writes", ConvSeg * 2), ("reads", ConvSeg * 2), ("reserved", C.c_int32)]


LIGHT_MAX_CONTOURS, LIGHT_POINTS_CAP = 1024, 4096   # array bounds of irmv_light_trace (the kernel's limits: light_limits())


FRONT_FUSED, FRONT_WIDTH_MOD4, FRONT_TAP_RANGE, FRONT_STAGE_LIMIT = 0, 1, 2, 3
MAX_FRAME_BYTES = 1 << 32


class FrontPlan(C.Structure):
    """irmv_front_plan_t (include/irmv_hip.h)."""
    _fields_ = [("fused", C.c_int32), ("reason", C.c_int32), ("fastx", C.c_int32), ("tile_y", C.c_int32),
                ("tiles_x", C.c_int32), ("tiles_y", C.c_int32), ("stage_bytes", C.c_int32), ("box", C.c_int32 * 4),
                ("fx_i0", C.c_int32), ("fx_step", C.c_int32), ("pair_cases", C.c_int32),
                ("tiles_inside", C.c_int32), ("tiles_x_edge", C.c_int32), ("tiles_y_edge", C.c_int32), ("tiles_corner", C.c_int32),
                ("max_pitch", C.c_int32), ("max_rows", C.c_int32), ("upload_kernel", C.c_int32), ("reserved", C.c_int32 * 3)]


class WindowMap(C.Structure):
    """irmv_window_map_t (include/irmv_hip.h)."""
    _fields_ = [("bx0", C.c_int32), ("by0", C.c_int32), ("band_offset", C.c_uint64), ("band_bytes", C.c_uint64),
                ("cx", C.c_double), ("cy", C.c_double), ("reserved", C.c_int32 * 4)]


class LightRec(C.Structure):
    _fields_ = [("corners", C.c_float * 8), ("top", C.c_float * 2), ("bottom", C.c_float * 2), ("center", C.c_float * 2),
                ("length", C.c_double), ("measured", C.c_int32), ("ok", C.c_int32), ("hull_edges", C.c_int32), ("in_lds", C.c_int32)]


class LightTrace(C.Structure):
    _fields_ = [("n_contours", C.c_int32), ("n_found", C.c_int32), ("n_points", C.c_int32), ("too_large", C.c_int32),
                ("pool_fit", C.c_int32), ("in_lds", C.c_int32), ("rx", C.c_int32), ("ry", C.c_int32), ("rw", C.c_int32), ("rh", C.c_int32),
                ("max_contours", C.c_int32), ("points_cap", C.c_int32), ("lds_image", C.c_int32), ("lds_points", C.c_int32),
                ("label_pool", C.c_uint64), ("pool_offset", C.c_uint64),
                ("starts", C.c_int32 * (LIGHT_MAX_CONTOURS + 1)), ("points", C.c_int16 * 2 * LIGHT_POINTS_CAP), ("reserved", C.c_int32),
                ("recs", LightRec * LIGHT_MAX_CONTOURS)]


METER_VIEW, METER_RAW = 0, 1
METER_DOMAINS = {"view": METER_VIEW, "raw": METER_RAW}


class YawOpts(C.Structure):
    """irmv_yaw_opts (include/irmv_hip.h, "constrained pose")."""
    _fields_ = [("struct_size", C.c_uint32), ("enable", C.c_int32), ("rounds", C.c_int32), ("reserved", C.c_int32),
                ("tau_max", C.c_double), ("horizon_min", C.c_double)]


class YawPose(C.Structure):
    """irmv_yaw_pose (include/irmv_hip.h): the constrained pose of one detection."""
    _fields_ = [("rvec", C.c_double * 3), ("tvec", C.c_double * 3), ("quat", C.c_double * 4),
                ("tau", C.c_double), ("cs", C.c_double), ("sn", C.c_double), ("err", C.c_double),
                ("state", C.c_int32), ("lane", C.c_int32 * 6), ("reserved", C.c_int32)]


class PoseCovOpts(C.Structure):
    """irmv_pose_cov_opts (include/irmv_hip.h, "pose uncertainty")."""
    _fields_ = [("struct_size", C.c_uint32), ("enable", C.c_int32), ("sigma_px", C.c_double)]


class PoseCov(C.Structure):
    """irmv_pose_cov (include/irmv_hip.h): the covariance of one detection's IPPE pose and of its constrained pose."""
    _fields_ = [("cov", C.c_double * 21), ("chi2", C.c_double), ("sigma_range", C.c_double),
                ("yaw_cov", C.c_double * 10), ("yaw_chi2", C.c_double), ("sigma_yaw", C.c_double),
                ("state", C.c_int32), ("yaw_state", C.c_int32)]


class TrackOpts(C.Structure):
    """irmv_track_opts (include/irmv_hip.h, "armor tracks")."""
    _fields_ = [("struct_size", C.c_uint32), ("enable", C.c_int32), ("confirm_hits", C.c_int32), ("max_misses", C.c_int32),
                ("match_class", C.c_int32), ("reserved", C.c_int32), ("gate", C.c_double), ("max_coast_s", C.c_double),
                ("accel_sigma", C.c_double), ("init_vel_sigma", C.c_double), ("sigma_lat", C.c_double), ("sigma_rng", C.c_double)]


class DetTrack(C.Structure):
    """irmv_det_track: what the tracker made of one detection."""
    _fields_ = [("state", C.c_int32), ("track", C.c_int32), ("id", C.c_uint32), ("hits", C.c_int32), ("d2", C.c_double),
                ("pos", C.c_double * 3), ("vel", C.c_double * 3)]


class TrackFrame(C.Structure):
    """irmv_track_frame: the header of a slot's track snapshot."""
    _fields_ = [("stamp", C.c_double), ("state", C.c_int32), ("n_live", C.c_int32), ("n_confirmed", C.c_int32), ("n_started", C.c_int32),
                ("n_deleted", C.c_int32), ("n_no_room", C.c_int32), ("next_id", C.c_uint32), ("reserved", C.c_int32)]


class Track(C.Structure):
    """irmv_track: one entry of the track table."""
    _fields_ = [("id", C.c_uint32), ("class_id", C.c_int32), ("state", C.c_int32), ("hits", C.c_int32), ("misses", C.c_int32),
                ("det", C.c_int32), ("first_stamp", C.c_double), ("last_hit", C.c_double), ("stamp", C.c_double),
                ("x", C.c_double * 6), ("P", C.c_double * 36)]


class TrackObs(C.Structure):
    """irmv_track_obs: one observation of the stand-alone tracker."""
    _fields_ = [("class_id", C.c_int32), ("valid", C.c_int32), ("has_cov", C.c_int32), ("reserved", C.c_int32),
                ("tvec", C.c_double * 3), ("cov", C.c_double * 9)]


TRACK_CAP = 32


def track_opts_struct(enable=1, **fields) -> TrackOpts:
    """An irmv_track_opts: the library's defaults (irmv_track_default_opts), then `fields` (no check: the library's are the
    ones under test)."""
    o = TrackOpts()
    check(load().irmv_track_default_opts(C.byref(o)))
    o.enable = int(enable)
    for name, v in fields.items():
        if name not in dict(TrackOpts._fields_) or name in ("struct_size", "reserved"):
            raise TypeError(f"irmv_track_opts has no option {name!r}")
        setattr(o, name, v)
    return o


def pose_cov_opts_struct(enable=1, sigma_px=1.0) -> PoseCovOpts:
    """An irmv_pose_cov_opts (no check: the library's are the ones under test)."""
    o = PoseCovOpts()
    o.struct_size = C.sizeof(PoseCovOpts)
    o.enable, o.sigma_px = int(enable), float(sigma_px)
    return o


def yaw_opts_struct(enable=1, rounds=4, tau_max=1.0, horizon_min=1e-4) -> YawOpts:
    """An irmv_yaw_opts (no check: the library's are the ones under test)."""
    o = YawOpts()
    o.struct_size = C.sizeof(YawOpts)
    o.enable, o.rounds, o.reserved = int(enable), int(rounds), 0
    o.tau_max, o.horizon_min = float(tau_max), float(horizon_min)
    return o


PATCH_W, PATCH_H = 20, 28


class PatchOpts(C.Structure):
    """irmv_patch_opts (include/irmv_hip.h, "plate patches")."""
    _fields_ = [("struct_size", C.c_uint32), ("enable", C.c_int32), ("span", C.c_int32 * 2), ("light_rows", C.c_int32),
                ("top", C.c_int32), ("reserved", C.c_int32 * 2)]


class PlatePatch(C.Structure):
    """irmv_plate_patch (include/irmv_hip.h): the rectified number image of one detection."""
    _fields_ = [("gray", (C.c_uint8 * PATCH_W) * PATCH_H), ("state", C.c_int32), ("otsu", C.c_int32), ("n_outside", C.c_int32),
                ("armor_size", C.c_int32), ("bar_sum", C.c_uint32 * 2), ("sum", C.c_uint32), ("reserved", C.c_int32)]


NUM_IN_BINARY, NUM_IN_GRAY, NUM_CLASSES_MAX = 0, 1, 16


class NumberModel(C.Structure):
    """irmv_number_model (include/irmv_hip.h, "plate numbers"); number_net.NumberModel.c_struct fills one."""
    _fields_ = [("struct_size", C.c_uint32), ("n_layers", C.c_int32), ("dims", C.c_int32 * 4), ("input", C.c_int32),
                ("weight", C.POINTER(C.c_float) * 3), ("bias", C.POINTER(C.c_float) * 3)]


class NumberOpts(C.Structure):
    """irmv_number_opts (include/irmv_hip.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("enable", C.c_int32), ("reserved", C.c_int32 * 3)]


class PlateNumber(C.Structure):
    """irmv_plate_number (include/irmv_hip.h): the MLP's reading of one detection's plate patch."""
    _fields_ = [("state", C.c_int32), ("label", C.c_int32), ("second", C.c_int32), ("ones", C.c_int32), ("margin", C.c_float),
                ("reserved", C.c_int32 * 3), ("logits", C.c_float * NUM_CLASSES_MAX)]


def patch_opts_struct(enable=1, span=(32, 54), light_rows=12, top=7) -> PatchOpts:
    """An irmv_patch_opts (no check: the library's are the ones under test)."""
    o = PatchOpts()
    o.struct_size = C.sizeof(PatchOpts)
    o.enable, o.light_rows, o.top = int(enable), int(light_rows), int(top)
    o.span[0], o.span[1] = int(span[0]), int(span[1])
    return o


class MeterOpts(C.Structure):
    """irmv_meter_opts (include/irmv_hip.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("domain", C.c_int32), ("x0", C.c_int32), ("y0", C.c_int32), ("w", C.c_int32),
                ("h", C.c_int32), ("step", C.c_int32), ("reserved", C.c_int32 * 2)]


class FrameStats(C.Structure):
    """irmv_frame_stats (include/irmv_hip.h)."""
    _fields_ = [("hist", C.c_uint32 * 256 * 4), ("n", C.c_uint32 * 4), ("rect", C.c_int32 * 4), ("domain", C.c_int32),
                ("step", C.c_int32), ("reserved", C.c_int32 * 2)]


class MeterMap(C.Structure):
    """irmv_meter_map_t (include/irmv_hip.h)."""
    _fields_ = [("rect", C.c_int32 * 4), ("region", C.c_int32 * 4), ("phase", C.c_int32 * 2), ("grid", C.c_int32 * 2),
                ("n", C.c_uint32 * 4), ("reserved", C.c_int32 * 4)]


DECLINED = 1    # irmv_engine_run_conv_candidate: no kernel runs that candidate
RUN_POISON, RUN_POISON_ONLY = 1, 2   # ... its flags: NaN over the output it must write first (and launch nothing)
RUN_BOX_ONLY, RUN_WRITTEN_LISTS = 4, 8   # a boxg op: without the keypoint branch that rides; on written lists (no cand_list_kernel)


def RUN_GRID(n):
    """IRMV_RUN_GRID: a boxg op's launch on n persistent workgroups (0: the engine's own grid)."""
    assert 0 <= n < 65536
    return n << 16


MEM_CLASSES = ("CONST", "ACT", "CARRIED", "SCRATCH")   # IRMV_MEM_CONST .. IRMV_MEM_SCRATCH
MEM_KINDS = ("U8", "F16", "F32", "F64", "INDEX")       # IRMV_MEM_U8 .. IRMV_MEM_INDEX


class MemRange(C.Structure):
    """irmv_mem_range (irmv_engine_debug_allocs): one device range of an engine with its class and kind."""
    _fields_ = [("name", C.c_char * 48), ("mem_class", C.c_int32), ("kind", C.c_int32), ("index_max", C.c_uint32),
                ("reserved", C.c_int32), ("bytes", C.c_uint64), ("base", C.c_uint64)]


# every symbol include/irmv_hip.h declares: (name, restype, argtypes)
_P = C.c_void_p
SYMBOLS = [
    ("irmv_last_error", C.c_char_p, []),
    ("irmv_version", C.c_char_p, []),
    ("irmv_device_count", C.c_int, [C.POINTER(C.c_int)]),
    ("irmv_device_synchronize", C.c_int, [C.c_int]),
    ("irmv_engine_cfg_default", None, [C.POINTER(EngineCfg)]),
    ("irmv_engine_create", C.c_int, [C.POINTER(EngineCfg), C.POINTER(_P)]),
    ("irmv_engine_destroy", None, [_P]),
    ("irmv_engine_num_slots", C.c_int, [_P]),
    ("irmv_engine_max_det", C.c_int, [_P]),
    ("irmv_engine_num_streams", C.c_int, [_P]),
    ("irmv_engine_sync_launch", C.c_int, [_P]),
    ("irmv_engine_numa_node", C.c_int, [_P]),
    ("irmv_engine_numa_placed", C.c_int, [_P]),
    ("irmv_numa_device_node", C.c_int, [C.c_int, C.POINTER(C.c_int)]),
    ("irmv_numa_bind_thread", C.c_int, [C.c_int]),
    ("irmv_numa_page_node", C.c_int, [C.c_void_p]),
    ("irmv_numa_parse_cpulist", C.c_int, [C.c_char_p, C.POINTER(C.c_int), C.c_int]),
    ("irmv_engine_src_buffer", C.POINTER(C.c_uint8), [_P, C.c_int]),
    ("irmv_engine_src_device_buffer", C.c_void_p, [_P, C.c_int]),
    ("irmv_engine_set_window", C.c_int, [_P, C.c_int, C.c_int, C.c_int]),
    ("irmv_engine_get_window", C.c_int, [_P, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("irmv_window_map", C.c_int, [C.POINTER(EngineCfg), C.c_int, C.c_int, C.POINTER(WindowMap)]),
    ("irmv_tile_grid", C.c_int, [C.POINTER(EngineCfg), C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("irmv_engine_submit_tiles", C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_uint32]),
    ("irmv_engine_merge_tiles", C.c_int, [_P, C.c_int, C.c_int]),
    ("irmv_engine_tile_results", C.c_int, [_P, C.c_int, C.POINTER(TileDet), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("irmv_engine_set_tile_merge", C.c_int, [_P, C.c_float, C.c_float]),
    ("irmv_engine_get_tile_merge", C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    ("irmv_engine_set_view", C.c_int, [_P, C.c_int, C.c_int]),
    ("irmv_engine_get_view", C.c_int, [_P, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("irmv_engine_debug_graph_count", C.c_int, [_P]),
    ("irmv_engine_src_format", C.c_int, [_P]),
    ("irmv_engine_src_bytes", C.c_size_t, [_P]),
    ("irmv_engine_submit", C.c_int, [_P, C.c_int, C.c_int, C.c_uint32]),
    ("irmv_engine_wait", C.c_int, [_P]),
    ("irmv_engine_wait_slots", C.c_int, [_P, C.c_int, C.c_int]),
    ("irmv_engine_wait_upload", C.c_int, [_P, C.c_int, C.c_int]),
    ("irmv_engine_set_extract_params", C.c_int, [_P, C.c_int, C.c_float, C.c_float, C.c_float, C.POINTER(C.c_double)]),
    ("irmv_engine_point_source", C.c_int, [_P]),
    ("irmv_engine_set_refine", C.c_int, [_P, C.c_float, C.c_float]),
    ("irmv_engine_get_refine", C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    ("irmv_engine_refine_points", C.c_int, [_P, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.POINTER(LightTrace), C.POINTER(Det)]),
    ("irmv_engine_results", C.c_int, [_P, C.c_int, C.POINTER(Det), C.c_int, C.POINTER(C.c_int)]),
    ("irmv_engine_detect", C.c_int, [_P, C.c_int, C.POINTER(Det), C.c_int, C.POINTER(C.c_int)]),
    ("irmv_engine_last_detect_ms", C.c_double, [_P]),
    ("irmv_engine_rotated_image", C.c_int, [_P, C.c_int, C.POINTER(C.c_uint8)]),
    ("irmv_engine_render_dims", C.c_int, [_P, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("irmv_engine_render", C.c_int, [_P, C.c_int, C.POINTER(RenderOpts), C.POINTER(Det), C.c_int, C.POINTER(C.c_uint8)]),
    ("irmv_render_glyph", C.c_int, [C.c_int, C.POINTER(C.c_uint8)]),
    ("irmv_engine_extract_armors", C.c_int, [_P, C.c_int, C.POINTER(C.c_float), C.c_int, C.POINTER(Det)]),
    ("irmv_engine_set_bayer_isp", C.c_int, [_P, C.POINTER(C.c_uint16), C.POINTER(C.c_uint8)]),
    ("irmv_engine_get_bayer_isp", C.c_int, [_P, C.POINTER(C.c_uint16), C.POINTER(C.c_uint8)]),
    ("irmv_engine_set_class_policy", C.c_int, [_P, C.POINTER(ClassPolicy)]),
    ("irmv_engine_get_class_policy", C.c_int, [_P, C.POINTER(ClassPolicy)]),
    ("irmv_class_policy_uniform", C.c_int, [C.c_float, C.c_int, C.POINTER(ClassPolicy)]),
    ("irmv_class_policy_enemy", C.c_int, [C.c_int, C.c_float, C.c_int, C.POINTER(ClassPolicy)]),
    ("irmv_class_policy_table", C.c_int, [C.POINTER(ClassPolicy), C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    ("irmv_engine_light_trace", C.c_int, [_P, C.c_int, C.POINTER(C.c_float), C.c_int, C.POINTER(LightTrace), C.POINTER(Det)]),
    ("irmv_light_limits", C.c_int, [C.POINTER(C.c_int32)]),
    ("irmv_post_limits", C.c_int, [C.POINTER(C.c_int32)]),
    ("irmv_engine_read_input", C.c_int, [_P, C.c_int, C.POINTER(C.c_float)]),
    ("irmv_engine_read_head", C.c_int, [_P, C.c_int, C.POINTER(C.c_float)]),
    ("irmv_engine_write_head", C.c_int, [_P, C.c_int, C.POINTER(C.c_float)]),
    ("irmv_engine_run_post", C.c_int, [_P, C.c_int, C.c_int]),
    ("irmv_engine_debug_poke_candidate_counts", C.c_int, [_P, C.c_int]),
    ("irmv_engine_debug_read_cand_bits", C.c_int, [_P, C.c_int, C.POINTER(C.c_uint32), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("irmv_engine_debug_write_cand_bits", C.c_int, [_P, C.c_int, C.POINTER(C.c_uint32), C.c_int]),
    ("irmv_engine_debug_write_cand_lists", C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ("irmv_engine_debug_read_head_rows", C.c_int, [_P, C.c_int, C.POINTER(C.c_float), C.c_size_t]),
    ("irmv_engine_debug_read_head_raw", C.c_int, [_P, C.c_int, C.POINTER(C.c_float)]),
    ("irmv_engine_read_tap", C.c_int, [_P, C.c_int, C.c_char_p, C.POINTER(C.c_float), C.POINTER(C.c_int)]),
    ("irmv_engine_read_raw", C.c_int, [_P, C.c_int, C.POINTER(RawDets)]),
    ("irmv_engine_num_anchors", C.c_int, [_P]),
    ("irmv_engine_head_channels", C.c_int, [_P]),
    ("irmv_engine_net_dims", C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("irmv_engine_conv_ops", C.c_int, [_P, C.POINTER(ConvOp), C.c_int, C.POINTER(C.c_int)]),
    ("irmv_engine_conv_candidates", C.c_int, [_P, C.c_int, C.c_int, C.POINTER(ConvCand), C.c_int, C.POINTER(C.c_int)]),
    ("irmv_engine_run_conv_candidate", C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32]),
    ("irmv_engine_read_tensor", C.c_int, [_P, C.c_char_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t]),
    ("irmv_engine_write_tensor", C.c_int, [_P, C.c_char_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t]),
    ("irmv_engine_ops", C.c_int, [_P, C.POINTER(GraphOp), C.c_int, C.POINTER(C.c_int)]),
    ("irmv_engine_op_io", C.c_int, [_P, C.c_int, C.POINTER(OpIo)]),
    ("irmv_engine_run_op", C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_uint32]),
    ("irmv_sppf_slab", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
    ("irmv_front_plan", C.c_int, [C.POINTER(EngineCfg), C.POINTER(FrontPlan)]),
    ("irmv_engine_profile", C.c_int, [_P, C.c_int, C.c_int, C.POINTER(KernelStat), C.c_int, C.POINTER(C.c_int)]),
    ("irmv_debug_lds_fill", C.c_int, [C.c_uint32]),
    ("irmv_debug_lds_probe", C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.c_int, C.POINTER(C.c_int)]),
    ("irmv_engine_debug_allocs", C.c_int, [_P, C.POINTER(MemRange), C.c_int, C.POINTER(C.c_int)]),
    ("irmv_engine_debug_fill_mem", C.c_int, [_P, C.c_uint32, C.POINTER(C.c_uint64)]),
    ("irmv_engine_debug_read_mem", C.c_int, [_P, C.c_int, C.c_uint64, C.c_void_p, C.c_uint64]),
    ("irmv_engine_debug_read_cand_counts", C.c_int, [_P, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int)]),
    ("irmv_pnp_create", C.c_int, [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(_P)]),
    ("irmv_pnp_destroy", None, [_P]),
    ("irmv_pnp_solve", C.c_int, [_P, C.POINTER(C.c_float), C.c_int, C.c_int, C.POINTER(C.c_double),
                                 C.POINTER(C.c_double), C.POINTER(C.c_int32)]),
    ("irmv_pnp_solve2", C.c_int, [_P, C.POINTER(C.c_float), C.c_int, C.c_int, C.POINTER(C.c_double),
                                  C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32)]),
    ("irmv_engine_set_pose_prior", C.c_int, [_P, C.POINTER(PosePrior)]),
    ("irmv_engine_get_pose_prior", C.c_int, [_P, C.POINTER(PosePrior)]),
    ("irmv_engine_set_up", C.c_int, [_P, C.c_int, C.POINTER(C.c_double)]),
    ("irmv_engine_get_up", C.c_int, [_P, C.c_int, C.POINTER(C.c_double)]),
    ("irmv_engine_pose_alts", C.c_int, [_P, C.c_int, C.POINTER(PoseAlt), C.c_int, C.POINTER(C.c_int)]),
    ("irmv_engine_set_yaw_solve", C.c_int, [_P, C.POINTER(YawOpts)]),
    ("irmv_engine_get_yaw_solve", C.c_int, [_P, C.POINTER(YawOpts)]),
    ("irmv_engine_yaw_poses", C.c_int, [_P, C.c_int, C.POINTER(YawPose), C.c_int, C.POINTER(C.c_int)]),
    ("irmv_pnp_solve_yaw", C.c_int, [_P, C.POINTER(C.c_float), C.c_int, C.c_int, C.POINTER(C.c_double), C.c_double,
                                     C.POINTER(YawOpts), C.POINTER(YawPose)]),
    ("irmv_engine_set_pose_cov", C.c_int, [_P, C.POINTER(PoseCovOpts)]),
    ("irmv_engine_get_pose_cov", C.c_int, [_P, C.POINTER(PoseCovOpts)]),
    ("irmv_engine_pose_covs", C.c_int, [_P, C.c_int, C.POINTER(PoseCov), C.c_int, C.POINTER(C.c_int)]),
    ("irmv_pnp_pose_cov", C.c_int, [_P, C.POINTER(C.c_float), C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                    C.POINTER(C.c_double), C.c_double, C.POINTER(PoseCov)]),
    ("irmv_engine_set_patches", C.c_int, [_P, C.POINTER(PatchOpts)]),
    ("irmv_engine_get_patches", C.c_int, [_P, C.POINTER(PatchOpts)]),
    ("irmv_engine_plate_patches", C.c_int, [_P, C.c_int, C.POINTER(PlatePatch), C.c_int, C.POINTER(C.c_int)]),
    ("irmv_engine_patches_at", C.c_int, [_P, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_int32), C.c_int, C.POINTER(PlatePatch)]),
    ("irmv_patch_limits", C.c_int, [C.POINTER(C.c_int32)]),
    ("irmv_engine_set_number_model", C.c_int, [_P, C.POINTER(NumberModel)]),
    ("irmv_number_model_read", C.c_int, [C.c_char_p, C.POINTER(NumberModel), C.POINTER(C.c_float), C.c_int64, C.POINTER(C.c_int64)]),
    ("irmv_engine_load_number_model", C.c_int, [_P, C.c_char_p]),
    ("irmv_engine_set_numbers", C.c_int, [_P, C.POINTER(NumberOpts)]),
    ("irmv_engine_get_numbers", C.c_int, [_P, C.POINTER(NumberOpts)]),
    ("irmv_engine_plate_numbers", C.c_int, [_P, C.c_int, C.POINTER(PlateNumber), C.c_int, C.POINTER(C.c_int)]),
    ("irmv_engine_numbers_at", C.c_int, [_P, C.POINTER(PlatePatch), C.c_int, C.POINTER(PlateNumber)]),
    ("irmv_number_limits", C.c_int, [C.POINTER(C.c_int32)]),
    ("irmv_engine_set_tracking", C.c_int, [_P, C.POINTER(TrackOpts)]),
    ("irmv_engine_get_tracking", C.c_int, [_P, C.POINTER(TrackOpts)]),
    ("irmv_track_default_opts", C.c_int, [C.POINTER(TrackOpts)]),
    ("irmv_engine_set_stamp", C.c_int, [_P, C.c_int, C.c_double]),
    ("irmv_engine_get_stamp", C.c_int, [_P, C.c_int, C.POINTER(C.c_double)]),
    ("irmv_engine_set_camera_pose", C.c_int, [_P, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("irmv_engine_get_camera_pose", C.c_int, [_P, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("irmv_engine_det_tracks", C.c_int, [_P, C.c_int, C.POINTER(DetTrack), C.c_int, C.POINTER(C.c_int)]),
    ("irmv_engine_tracks", C.c_int, [_P, C.c_int, C.POINTER(TrackFrame), C.POINTER(Track), C.c_int, C.POINTER(C.c_int)]),
    ("irmv_engine_reset_tracks", C.c_int, [_P]),
    ("irmv_track_limits", C.c_int, [C.POINTER(C.c_int32)]),
    ("irmv_track_predict", C.c_int, [C.POINTER(Track), C.c_double, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("irmv_tracker_create", C.c_int, [C.c_int, C.POINTER(TrackOpts), C.POINTER(C.c_void_p)]),
    ("irmv_tracker_destroy", None, [_P]),
    ("irmv_tracker_update", C.c_int, [_P, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(TrackObs), C.c_int,
                                      C.POINTER(DetTrack), C.POINTER(TrackFrame), C.POINTER(Track)]),
    ("irmv_tracker_reset", C.c_int, [_P]),
    ("irmv_number_softmax", C.c_int, [C.POINTER(PlateNumber), C.c_int, C.POINTER(C.c_float)]),
    ("irmv_meter_map", C.c_int, [C.POINTER(EngineCfg), C.POINTER(MeterOpts), C.c_int, C.c_int, C.c_int, C.POINTER(MeterMap)]),
    ("irmv_meter_limits", C.c_int, [C.POINTER(C.c_int32)]),
    ("irmv_engine_meter", C.c_int, [_P, C.c_int, C.POINTER(MeterOpts), C.POINTER(FrameStats)]),
    ("irmv_engine_set_metering", C.c_int, [_P, C.POINTER(MeterOpts)]),
    ("irmv_engine_get_metering", C.c_int, [_P, C.POINTER(MeterOpts), C.POINTER(C.c_int)]),
    ("irmv_engine_frame_stats", C.c_int, [_P, C.c_int, C.POINTER(FrameStats)]),
    ("irmv_stats_mean_q8", C.c_int, [C.POINTER(FrameStats), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("irmv_stats_percentile", C.c_int, [C.POINTER(FrameStats), C.c_int, C.c_uint64, C.c_uint64, C.POINTER(C.c_int)]),
    ("irmv_stats_gray_world", C.c_int, [C.POINTER(FrameStats), C.c_int, C.c_int, C.POINTER(C.c_uint16)]),
    ("irmv_stats_exposure_q8", C.c_int, [C.POINTER(FrameStats), C.c_int, C.c_uint64, C.c_uint64, C.c_int, C.POINTER(C.c_int)]),
]

_lib = None


def lib_path() -> str:
    """The in-tree library; IRMV_LIB_PATH names another build of it (A/B runs of two kernel versions on one box)."""
    return os.environ.get("IRMV_LIB_PATH") or _build.LIB_PATH


def load():
    """Load libirmv_hip.so (must have been built in-tree; see __graft_entry__.build)."""
    global _lib
    if _lib is None:
        path = lib_path()
        if not os.path.exists(path):
            raise IrmvError(ERR_HIP, f"{path} is missing: build the HIP extension first "
                                     "(python -m irmv_detection_amd._build); there is no CPU fallback")
        L = C.CDLL(path)
        for name, res, args in SYMBOLS:
            if os.environ.get("IRMV_LIB_PATH") and not hasattr(L, name):
                continue                    # A/B runs against an OLDER build of the library: entries added since are absent there
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc: int, allow=()):
    if rc != OK and rc not in allow:
        raise IrmvError(rc, load().irmv_last_error().decode(errors="replace"))
    return rc


def device_count() -> int:
    """HIP devices visible to this process (0 without a GPU)."""
    n = C.c_int(0)
    return n.value if load().irmv_device_count(C.byref(n)) == OK else 0


def device_synchronize(device: int = 0) -> None:
    check(load().irmv_device_synchronize(device))


DEBUG_LDS_WORDS = 40960   # IRMV_DEBUG_LDS_WORDS


def debug_lds_fill(pattern32: int) -> None:
    """Test hook: leave pattern32 in every LDS word of every CU of the current device (several 160 KiB workgroups per CU)."""
    check(load().irmv_debug_lds_fill(pattern32))


def debug_lds_probe(pattern32: int, word: int = 0):
    """Test hook: -> uint32 [workgroups][4]: words that hold pattern32, the value found in `word`, HW_ID, XCC_ID.  The probe
    writes no LDS."""
    import numpy as np
    n = C.c_int(0)
    check(load().irmv_debug_lds_probe(pattern32, word, None, 0, C.byref(n)))
    out = np.zeros((n.value, 4), np.uint32)
    check(load().irmv_debug_lds_probe(pattern32, word, out.ctypes.data_as(C.POINTER(C.c_uint32)), n.value, C.byref(n)))
    return out


def light_limits() -> dict:
    """The light extraction's limits as the kernel is compiled (host only): contours and contour points per box (more
    = no answer), bytes of a label image that stays in LDS, points of a contour that is measured in LDS."""
    v = (C.c_int32 * 4)()
    check(load().irmv_light_limits(v))
    return dict(max_contours=v[0], points_cap=v[1], lds_image=v[2], lds_points=v[3])


POST_LIMIT_NAMES = ("rank_use", "rank_max", "lazy_n", "sup_cap", "cand_cap", "pre_hi", "pre_lo", "max_tiles", "max_det_cap",
                    "scan_blocks", "scan_step", "scan_lds_max", "inscan_chunk", "mat_n")


def post_limits() -> dict:
    """The candidate counts at which decode + NMS (k_post.hip) changes its code path and the tile merge's capacities, as the
    kernels are compiled (host only; irmv_post_limits in include/irmv_hip.h names each)."""
    v = (C.c_int32 * 16)()
    check(load().irmv_post_limits(v))
    return {k: int(v[i]) for i, k in enumerate(POST_LIMIT_NAMES)}


def render_opts(kind=RENDER_COLOR, scale=1, marks=MARK_ALL, binary_threshold=-1) -> RenderOpts:
    """An irmv_render_opts (no check: the library's are the ones under test)."""
    o = RenderOpts()
    o.struct_size = C.sizeof(RenderOpts)
    o.kind, o.scale, o.marks, o.binary_threshold = int(kind), int(scale), int(marks), int(binary_threshold)
    return o


def render_glyph(ch: str):
    """irmv_render_glyph (host only): the seven rows of the 5 x 7 glyph drawn for ch, or None where there is none."""
    rows = (C.c_uint8 * 7)()
    return tuple(rows) if load().irmv_render_glyph(ord(ch), rows) == OK else None


def class_policy_struct(score_thr, plate) -> ClassPolicy:
    """An irmv_class_policy from 16 thresholds and 16 plates (no check: the library's are the ones under test)."""
    p = ClassPolicy()
    p.struct_size = C.sizeof(ClassPolicy)
    for c in range(16):
        p.score_thr[c] = float(score_thr[c])
        p.plate[c] = int(plate[c])
    return p


def pose_prior_struct(mode=POSE_MIN_ERR, ratio=8.0, normal_up=NORMAL_UP_ROBOT, normal_up_default=None) -> PosePrior:
    """An irmv_pose_prior (no check: the library's are the ones under test).  normal_up: one number for every class, or 16."""
    import numpy as np
    p = PosePrior()
    p.struct_size = C.sizeof(PosePrior)
    p.mode = POSE_MODES[mode] if isinstance(mode, str) else int(mode)
    p.ambiguity_ratio = float(ratio)
    nu = np.broadcast_to(np.asarray(normal_up, np.float64), (16,))
    for c in range(16):
        p.normal_up[c] = float(nu[c])
    p.normal_up_default = float(nu[0] if normal_up_default is None else normal_up_default)
    return p


def class_policy_uniform(score_thr: float, armor_size: int = ARMOR_SMALL) -> ClassPolicy:
    p = ClassPolicy()
    check(load().irmv_class_policy_uniform(score_thr, armor_size, C.byref(p)))
    return p


def class_policy_enemy(enemy_color: int, score_thr: float, armor_size: int = ARMOR_SMALL) -> ClassPolicy:
    """irmv_class_policy_enemy: 0 = the enemy is blue (B1..BS on, R1..RS off), 1 = red, -1 = both on."""
    p = ClassPolicy()
    check(load().irmv_class_policy_enemy(enemy_color, score_thr, armor_size, C.byref(p)))
    return p


def class_policy_table(p: ClassPolicy, nc: int):
    """irmv_class_policy_table (host only): -> (logit_thr float32[16], min_logit_thr float32), the table an engine of nc
    classes uploads for p."""
    import numpy as np
    thr = np.zeros(16, np.float32)
    mn = C.c_float(0)
    check(load().irmv_class_policy_table(C.byref(p), nc, thr.ctypes.data_as(C.POINTER(C.c_float)), C.byref(mn)))
    return thr, np.float32(mn.value)


def _geometry_cfg(src_size, net_size, net_height, resize_mode, rotate180, src_format, window) -> EngineCfg:
    cfg = EngineCfg()
    load().irmv_engine_cfg_default(C.byref(cfg))
    cfg.src_width, cfg.src_height = int(src_size[0]), int(src_size[1])
    cfg.net_size, cfg.net_height = int(net_size), 0 if net_height is None else int(net_height)
    cfg.resize_mode, cfg.rotate180 = int(resize_mode), int(bool(rotate180))
    cfg.src_format = BAYER_FORMATS[src_format.upper()] if isinstance(src_format, str) else int(src_format)
    if window is not None:
        cfg.win_width, cfg.win_height = int(window[0]), int(window[1])
    return cfg


def meter_opts(domain=METER_VIEW, rect=None, step=1) -> MeterOpts:
    """An irmv_meter_opts (no check: the library's are the ones under test).  domain: "view" / "raw" or IRMV_METER_*;
    rect: (x0, y0, w, h) in view-local result coordinates, None = the whole view."""
    o = MeterOpts()
    o.struct_size = C.sizeof(MeterOpts)
    o.domain = METER_DOMAINS[domain] if isinstance(domain, str) else int(domain)
    if rect is not None:
        o.x0, o.y0, o.w, o.h = (int(v) for v in rect)
    o.step = int(step)
    return o


def stats_dict(s: FrameStats) -> dict:
    """An irmv_frame_stats as metering.meter returns it: hist uint32 [4][256], n uint32 [4], rect, domain, step."""
    import numpy as np
    return dict(hist=np.ctypeslib.as_array(s.hist).astype(np.uint32).reshape(4, 256).copy(), n=np.array(list(s.n), np.uint32),
                rect=tuple(s.rect), domain=int(s.domain), step=int(s.step))


def stats_struct(stats) -> FrameStats:
    """The irmv_frame_stats of a record dict (metering.meter, stats_dict)."""
    import numpy as np
    s = FrameStats()
    h = np.ascontiguousarray(np.asarray(stats["hist"], np.uint32).reshape(4, 256))
    C.memmove(s.hist, h.ctypes.data, h.nbytes)
    for i in range(4):
        s.n[i] = int(stats["n"][i])
        s.rect[i] = int(stats.get("rect", (0, 0, 0, 0))[i])
    s.domain, s.step = int(stats.get("domain", 0)), int(stats.get("step", 1))
    return s


def meter_map(src_size, opts: MeterOpts, view=0, window=None, win_xy=(0, 0), rotate180=True, src_format=SRC_HWC8, net_size=640, net_height=None) -> dict:
    """Where a metering rectangle lies (host only, irmv_meter_map): the record's rect, the region in the buffer that is read,
    the sample grid and n[4], as the engine's kernels compute them; raises IrmvError where an argument is refused."""
    cfg = _geometry_cfg(src_size, net_size, net_height, RESIZE_STRETCH, rotate180, src_format, window)
    m = MeterMap()
    check(load().irmv_meter_map(C.byref(cfg), C.byref(opts), int(view), int(win_xy[0]), int(win_xy[1]), C.byref(m)))
    return dict(rect=tuple(m.rect), region=tuple(m.region), phase=tuple(m.phase), grid=tuple(m.grid), n=tuple(m.n))


METER_LIMIT_NAMES = ("rows_per_block", "blocks_max", "lds_bytes", "threads", "batch_frames", "blocks_batch")


def meter_limits() -> dict:
    """The metering kernel's launch shape as compiled (host only, irmv_meter_limits)."""
    v = (C.c_int32 * 8)()
    check(load().irmv_meter_limits(v))
    return {k: int(v[i]) for i, k in enumerate(METER_LIMIT_NAMES)}


def stats_mean_q8(stats, row, lo=0, hi=255):
    """irmv_stats_mean_q8 -> (mean_q8, count)."""
    m, n = C.c_uint64(0), C.c_uint64(0)
    check(load().irmv_stats_mean_q8(C.byref(stats_struct(stats)), int(row), int(lo), int(hi), C.byref(m), C.byref(n)))
    return m.value, n.value


def stats_percentile(stats, row, num, den) -> int:
    v = C.c_int(0)
    check(load().irmv_stats_percentile(C.byref(stats_struct(stats)), int(row), int(num), int(den), C.byref(v)))
    return v.value


def stats_gray_world(stats, lo=8, hi=247):
    """irmv_stats_gray_world -> (gain_R, 256, gain_B), Q8."""
    g = (C.c_uint16 * 3)()
    check(load().irmv_stats_gray_world(C.byref(stats_struct(stats)), int(lo), int(hi), g))
    return tuple(g)


def stats_exposure_q8(stats, row, num, den, target) -> int:
    v = C.c_int(0)
    check(load().irmv_stats_exposure_q8(C.byref(stats_struct(stats)), int(row), int(num), int(den), int(target), C.byref(v)))
    return v.value


def window_map(src_size, window, x0, y0, rotate180=True, camera_matrix=None, net_size=640, net_height=None) -> dict:
    """Where a window at (x0, y0) lies (host only, irmv_window_map): the corner in buffer coordinates, the band of
    full-width rows it covers and the shifted principal point, as the engine computes them."""
    cfg = _geometry_cfg(src_size, net_size, net_height, RESIZE_STRETCH, rotate180, SRC_HWC8, window)
    if camera_matrix is not None:
        for i, v in enumerate(camera_matrix):
            cfg.camera_matrix[i] = float(v)
    m = WindowMap()
    check(load().irmv_window_map(C.byref(cfg), int(x0), int(y0), C.byref(m)))
    return dict(bx0=m.bx0, by0=m.by0, band_offset=m.band_offset, band_bytes=m.band_bytes, cx=m.cx, cy=m.cy)


def tile_grid(src_size, window, overlap, rotate180=True, net_size=640, net_height=None):
    """The tile grid of a tiled search (host only, irmv_tile_grid): -> (corners [(x, y)] row-major in result coordinates, nx, ny).
    overlap: one number or (ox, oy), the least overlap of neighbouring tiles.  irmv_detection_amd.tiles.grid is its reference."""
    import numpy as np
    ox, oy = (overlap, overlap) if np.ndim(overlap) == 0 else overlap
    cfg = _geometry_cfg(src_size, net_size, net_height, RESIZE_STRETCH, rotate180, SRC_HWC8, window)
    n, nx, ny = C.c_int(0), C.c_int(0), C.c_int(0)
    check(load().irmv_tile_grid(C.byref(cfg), int(ox), int(oy), None, 0, C.byref(n), C.byref(nx), C.byref(ny)))
    xy = (C.c_int32 * (2 * n.value))()
    check(load().irmv_tile_grid(C.byref(cfg), int(ox), int(oy), xy, n.value, C.byref(n), C.byref(nx), C.byref(ny)))
    return [(xy[2 * t], xy[2 * t + 1]) for t in range(n.value)], nx.value, ny.value


def front_plan(src_size, net_size, net_height=None, resize_mode=RESIZE_STRETCH, rotate180=True, src_format=SRC_HWC8, window=None) -> dict:
    """The front's plan for a configuration (host only, irmv_front_plan): what irmv_engine_create decides from the same
    fields.  Raises IrmvError where the engine's validation refuses them.  window = (w, h): the plan of a window engine."""
    L = load()
    cfg = _geometry_cfg(src_size, net_size, net_height, resize_mode, rotate180, src_format, window)
    p = FrontPlan()
    check(L.irmv_front_plan(C.byref(cfg), C.byref(p)))
    d = {f: getattr(p, f) for f, _ in FrontPlan._fields_ if f not in ("box", "reserved")}
    d["box"] = tuple(p.box)
    d["fused"], d["upload_kernel"] = bool(p.fused), bool(p.upload_kernel)
    return d


def numa_parse_cpulist(text: str):
    """The library's own parser of a sysfs cpulist ("0-3,8,10-11"), as used for thread placement."""
    buf = (C.c_int * 4096)()
    n = load().irmv_numa_parse_cpulist(text.encode(), buf, 4096)
    return [buf[i] for i in range(min(n, 4096))]


def numa_bind_to_device(device: int = 0) -> int:
    """Bind the calling thread to the CPUs of the host NUMA node closest to `device` (multi-GPU runners call this per rank /
    per worker thread BEFORE creating the engine and filling its slots).  Returns the node, or -1 if nothing was bound."""
    node = C.c_int(-1)
    if not hasattr(load(), "irmv_numa_device_node"):
        return -1
    if load().irmv_numa_device_node(device, C.byref(node)) != OK or node.value < 0:
        return -1
    return node.value if load().irmv_numa_bind_thread(node.value) == OK else -1
