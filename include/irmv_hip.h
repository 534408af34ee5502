/*
 * irmv_hip.h -- C ABI of libirmv_hip.so: the MI355X (gfx950) armor-detection hot path.
 *
 * This is the boundary a maintainer of illini-robomaster/irmv_detection binds
 * against to replace the TensorRT/NPP/CUDA-graph implementation of
 * irmv_detection::YoloEngine and the OpenCV implementation of
 * irmv_detection::PnPSolver (reference include/irmv_detection/yolo_engine.hpp:28-35,
 * include/irmv_detection/pnp_solver.hpp:15-23).  Plain C types only: pointers,
 * sizes, POD structs.  The header-only C++ facade in include/irmv_detection/
 * wraps these entry points 1:1 behind the reference's own class names.
 *
 * Every entry returns IRMV_OK (0) or a negative error code (one test hook also
 * IRMV_DECLINED); irmv_last_error() returns a thread-local message.  (The reference checks no CUDA/NPP/TensorRT
 * return code at all -- src/yolo_engine.cpp passim.)
 *
 * There is no CPU fallback anywhere behind this ABI: without a HIP device every
 * compute entry fails with IRMV_ERR_HIP.
 */
#ifndef IRMV_HIP_H
#define IRMV_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IRMV_OK 0
#define IRMV_ERR_ARG (-1)      /* bad argument / configuration            */
#define IRMV_ERR_HIP (-2)      /* HIP runtime failure (message has detail) */
#define IRMV_ERR_MODEL (-3)    /* weight blob missing or not matching      */

#define IRMV_RESIZE_STRETCH 0   /* reference behaviour: src/yolo_engine.cpp:186-190 */
#define IRMV_RESIZE_LETTERBOX 1 /* north-star variant */

#define IRMV_ARMOR_SMALL 0 /* 135 x 55 mm; the reference always solves with this one (src/pnp_solver.cpp:47) */
#define IRMV_ARMOR_LARGE 1 /* 225 x 55 mm */

#define IRMV_POINTS_AUTO 0
#define IRMV_POINTS_KEYPOINT_HEAD 1
#define IRMV_POINTS_CLASSICAL 2 /* gray -> threshold -> contours -> minAreaRect -> lights, on the GPU */
#define IRMV_POINTS_REFINED 3   /* the keypoint head's points, snapped to the light bars found at them (irmv_engine_set_refine) */

/* Format of the frames a producer writes into the source slots (irmv_engine_cfg.src_format).
 *   IRMV_SRC_HWC8: H x W x 3 bytes per slot, interleaved pixels in the model's channel order (swap_rb = 0) -- the reference's
 *                  CAMERA_MEDIA_TYPE_RGB8 frame after the camera SDK's CPU ISP.
 *   IRMV_SRC_BAYER_*8: H x W bytes per slot, the sensor's raw 8-bit colour-filter-array frame; the name gives the colours of
 *                  the 2 x 2 cell at (0,0) (0,1) / (1,0) (1,1).  H and W must be even.  The first kernel of every step
 *                  demosaics it on the GPU into the R, G, B frame an IRMV_SRC_HWC8 engine would have been handed: integer
 *                  bilinear interpolation (round half up, reflect-101 borders) or, with bayer_demosaic =
 *                  IRMV_DEMOSAIC_MHC, the 5 x 5 Malvar-He-Cutler filters, then the white-balance gains
 *                  out = min(255, (v * gain + 128) >> 8) per channel (bayer_gain_q8, Q8, 256 = 1.0) and, once
 *                  irmv_engine_set_bayer_isp has been called, a per-channel tone LUT.  swap_rb, rotate180,
 *                  resize_mode and everything downstream then act on that frame exactly as on an HWC8 one.
 *                  irmv_detection_amd/bayer.py is the bit-exact host reference. */
#define IRMV_SRC_HWC8 0
#define IRMV_SRC_BAYER_RGGB8 1
#define IRMV_SRC_BAYER_BGGR8 2
#define IRMV_SRC_BAYER_GRBG8 3
#define IRMV_SRC_BAYER_GBRG8 4

/* Interpolation of a Bayer engine (irmv_engine_cfg.bayer_demosaic).
 *   IRMV_DEMOSAIC_BILINEAR: the 3 x 3 integer bilinear interpolation above (default).
 *   IRMV_DEMOSAIC_MHC: Malvar-He-Cutler in integers.  Reflect-101 borders at radius 2 (-1 -> 1, -2 -> 2, W -> W-2,
 *                  W+1 -> W-3); a site's own colour is its raw value; the other two are clamp((s + 8) >> 4, 0, 255) of a
 *                  signed sum s in sixteenths (arithmetic shift = floor).  C the centre, S1 / S2 the four axis neighbours at
 *                  distance 1 / 2, X the four diagonals:
 *                    G at an R or B site                                  8 C + 4 S1 - 2 S2
 *                    at a G site, the colour sampled in this site's row     10 C + 8 (W1 + E1) - 2 X - 2 (W2 + E2) + (N2 + S2)
 *                    at a G site, the colour sampled in this site's column  10 C + 8 (N1 + S1) - 2 X - 2 (N2 + S2) + (W2 + E2)
 *                    B at an R site, R at a B site                        12 C + 4 X - 3 S2
 *                  Needs src_width >= 4 and src_height >= 4.  Gains and LUT apply afterwards, as one table look-up. */
#define IRMV_DEMOSAIC_BILINEAR 0
#define IRMV_DEMOSAIC_MHC 1

#define IRMV_NUM_CLASSES 14   /* ArmorClass B1..RS; 14 = UNKNOWN (include/irmv_detection/armor.hpp:7) */
#define IRMV_MAX_DET_CAP 256
#define IRMV_CAND_CAP 8192    /* most candidates the NMS walk can take (upper bound of pre_nms_cap) */

typedef struct irmv_engine irmv_engine;

/* Replaces the arguments of YoloEngine::YoloEngine (src/yolo_engine.cpp:24-26)
 * plus everything that constructor bakes in (640, EfficientNMS thresholds inside
 * the absent TensorRT plan, PnP constants of src/pnp_solver.cpp:7-34). */
typedef struct irmv_engine_cfg {
    uint32_t struct_size;      /* = sizeof(irmv_engine_cfg) */
    int32_t device;            /* HIP device ordinal */
    int32_t src_width;         /* camera frame, e.g. 1280 (cv::Size src_image_size) */
    int32_t src_height;        /* e.g. 1024 */
    int32_t net_size;          /* network input width; also its height when net_height is 0: 640 (src/yolo_engine.cpp:98-99,189) */
    int32_t resize_mode;       /* IRMV_RESIZE_* */
    int32_t rotate180;         /* 1 = reference (nppiMirror both axes, :182-184) */
    int32_t swap_rb;           /* 0 = reference: producer deposits model channel order */
    float score_thr;           /* EfficientNMS score_threshold, default 0.25 */
    float iou_thr;             /* EfficientNMS iou_threshold, default 0.45 */
    int32_t max_det;           /* EfficientNMS max_output_boxes, default 100, <= IRMV_MAX_DET_CAP */
    int32_t pre_nms_cap;       /* candidates entering the NMS walk, default 4096, <= IRMV_CAND_CAP */
    int32_t num_slots;         /* frames in flight; the reference node uses 3 (src/irm_detector.cpp:35-38) */
    int32_t armor_size;        /* IRMV_ARMOR_*: object points of the fused PnP */
    double camera_matrix[9];   /* row-major K (config/camera_info.yaml:7) */
    double dist_coeffs[5];     /* k1 k2 p1 p2 k3 (config/camera_info.yaml:12) */
    const char *weights_path;  /* "<stem>.onnx" (sibling "<stem>.irmw" is loaded, like :28-31) or a ".irmw" path; NULL -> weights_blob */
    const void *weights_blob;  /* .irmw image in host memory, or in device memory if weights_on_device */
    uint64_t weights_bytes;
    int32_t weights_on_device; /* 1: weights_blob is a device pointer (e.g. filled by an RCCL broadcast) */
    int32_t num_streams;       /* compute streams (0 = default: one per 64 slots, at least 2 and at most 4; one per slot for engines
                                  of <= 4 slots).  A multi-slot submit() is cut into that many sub-batches replayed as concurrent
                                  graphs, whose launch gaps and tails fill each other (measured: 128 frames as 2 x 64 +9 % over 1 x 128,
                                  as 3 or 4 graphs -10 %; 192 frames as 3 x 64 +5 % over 128 as 2 x 64); a single-slot submit rides
                                  stream (slot mod num_streams), so the steps of different slots overlap (three single frames in
                                  flight: 6.1 k FPS against 2.7 k one at a time) */
    /* Source of the four armor points PnP consumes.  The reference obtains them by classical CV inside
     * each bbox (IrmDetector::extract_armors, src/irm_detector.cpp:292-355); a pose-style model carries them
     * in a keypoint head.  IRMV_POINTS_AUTO picks the keypoint head when the model has one (never IRMV_POINTS_REFINED, which
     * like IRMV_POINTS_KEYPOINT_HEAD is refused with IRMV_ERR_MODEL on a model without a keypoint head). */
    int32_t point_source;      /* IRMV_POINTS_* */
    int32_t binary_threshold;  /* 150 (src/irm_detector.cpp:152) */
    float light_min_ratio;     /* 0.1 */
    float light_max_ratio;     /* 0.4 */
    float light_max_angle;     /* 40 degrees */
    float reserved0;
    double armor_min_small_center_distance; /* 0.8 */
    double armor_max_small_center_distance; /* 3.2 */
    double armor_min_large_center_distance; /* 3.2 */
    double armor_max_large_center_distance; /* 5.5 */
    /* Appended fields.  irmv_engine_create also accepts struct_size = offsetof(irmv_engine_cfg, src_format) (callers built
     * against the header without them) and then uses IRMV_SRC_HWC8 and gains of 256. */
    int32_t src_format;        /* IRMV_SRC_* (default IRMV_SRC_HWC8) */
    uint16_t bayer_gain_q8[3]; /* R, G, B white-balance gains of a Bayer engine, Q8 in [0, 1023]; 256 = identity (default) */
    uint16_t bayer_demosaic;   /* IRMV_DEMOSAIC_* of a Bayer engine (default IRMV_DEMOSAIC_BILINEAR; callers with an older struct_size get it) */
    /* Appended after those.  irmv_engine_create also accepts struct_size = offsetof(irmv_engine_cfg, reserved2) (= the sizeof
     * of the header before this field; bytes from net_height on are then not read) and uses net_height = 0.
     * Rectangular network input: net_size is the width W, net_height the height H, both multiples of 32 in [64, 2048];
     * 0 = square (H = net_size, default).  The input is [3][H][W]; the head has A = sum over s in {8, 16, 32} of
     * (H / s)(W / s) anchors (640 x 512: 6720).  Geometry per axis, sw x sh the source frame:
     *   IRMV_RESIZE_STRETCH:   scale_x = sw / W, scale_y = sh / H (1280 x 1024 -> 640 x 512: 2 : 1 on both axes, no distortion)
     *   IRMV_RESIZE_LETTERBOX: r = min(W / sw, H / sh), nw = min(W, floor(sw r + 0.5)), nh = min(H, floor(sh r + 0.5)),
     *                          px = (W - nw) / 2, py = (H - nh) / 2; the rest is grey padding (none for 1280 x 1024 -> 640 x 512)
     * For W == H this is exactly the square arithmetic. */
    int32_t net_height;
    int32_t reserved2;
    /* Appended after those, into what was the struct's tail padding: sizeof(irmv_engine_cfg) is what it was without them, so a
     * caller built against that header passes the same struct_size and whatever its padding bytes hold -- zeros, since every
     * caller fills the struct with irmv_engine_cfg_default first (which clears all of it).  Anything else there is refused as
     * a bad window, never run.  The two older struct sizes get 0, 0.
     * Tracking window: run the step on a win_width x win_height crop of the camera frame, at the sensor's resolution.  Both 0
     * (default): no window.  Otherwise 1 <= win_width <= src_width and 1 <= win_height <= src_height.  src_width x src_height
     * stays the full frame -- what a producer writes, what irmv_engine_src_bytes / _src_buffer / _src_device_buffer describe
     * and IRMV_MAX_FRAME_BYTES bounds -- and the first kernel of every step (the second of a Bayer engine, behind the
     * demosaic of the whole frame) cuts the slot's window out of it.  Everything downstream sees win_width x win_height where
     * it saw src_width x src_height: the resize or letterbox into the net input, irmv_front_plan (src_width % 4 now asks it of
     * win_width), the light extraction, irmv_engine_rotated_image.  Where the window lies is per-slot state, moved with
     * irmv_engine_set_window without re-capturing anything; at creation every slot's window is centred.  Detections come
     * back in full-frame coordinates; PnP sees the window's pixels with the principal point moved by the corner. */
    int16_t win_width, win_height;
} irmv_engine_cfg;

/* One detection: YoloEngine::bbox (yolo_engine.hpp:19-26) in source-frame
 * pixels as produced by parse_output (src/yolo_engine.cpp:202-220), plus what
 * the node derives per armor downstream: the four points PnP consumes
 * (src/pnp_solver.cpp:41-44), rvec/tvec (:49-51) and the pose quaternion
 * (src/irm_detector.cpp:218-226). */
typedef struct irmv_det {
    float xyxy[4];
    float score;
    int32_t class_id;  /* 0..13, 14 = UNKNOWN.  A model with nc > 14 reports its classes >= 14 as UNKNOWN here;
                        * irmv_raw_dets.det_classes keeps them. */
    int32_t anchor;    /* index of the originating anchor (debug / parity) */
    int32_t pnp_ok;    /* 1 if rvec/tvec are valid */
    float kpts[8];     /* left-bottom, left-top, right-top, right-bottom; source-frame pixels */
    double rvec[3];
    double tvec[3];
    double quat[4];    /* x, y, z, w */
    int32_t armor_valid; /* 1: kpts are an armor's points (keypoint head: always; classical: two gated lights found);
                            0: no armor in this bbox; -1: no answer, the extraction scratch was exhausted (the frame's
                            bboxes cover more than 8 frame areas in total, or one bbox holds more than 1024 contours /
                            4096 contour points) -- reported, never replaced by a truncated result */
    int32_t armor_size;  /* IRMV_ARMOR_*: classical path derives it from the light-centre distance (src/irm_detector.cpp:340-341) */
    int32_t n_lights;    /* classical path: lights that passed is_light() in this bbox; refined path: in the guided ROI */
    int32_t reserved;    /* IRMV_POINTS_REFINED engines and irmv_engine_refine_points: the refine flag --
                            1: kpts and the pose are the light bars'; 0: the head's points kept (no admissible pair, one light for
                            both sides, unusable keypoints, or PnP refused the new quad); -1: the head's points kept because the
                            extraction had no answer (label pool, contour or point limit: where the classical source reports
                            armor_valid = -1).  Every other engine: 0 */
} irmv_det;

/* EfficientNMS-layout view of one frame's result in net-input coordinates
 * (what the reference binds as num_dets / det_boxes / det_scores / det_classes,
 * src/yolo_engine.cpp:53-57,82-85).  Arrays hold max_det entries. */
typedef struct irmv_raw_dets {
    int32_t num_dets;
    int32_t n_candidates;  /* (anchor, class) pairs above their class's score threshold (irmv_class_policy; cfg.score_thr) before any cap */
    float *det_boxes;      /* [max_det][4] xyxy, net-input pixels */
    float *det_scores;     /* [max_det] */
    int32_t *det_classes;  /* [max_det] */
    int32_t *det_anchors;  /* [max_det] */
    float *det_kpts;       /* [max_det][8] net-input pixels */
} irmv_raw_dets;

typedef struct irmv_kernel_stat {
    char name[48];      /* kernel family, e.g. "conv3x3s1_mt2_nt4" */
    char layer[32];     /* graph node, e.g. "model.22.cv2.0.0" */
    double flops;       /* algorithmic FLOPs of this launch (2*MAC) */
    double bytes;       /* algorithmic bytes: inputs once + outputs once + weights once */
    float ms;           /* HIP-event duration on the engine's compute stream */
    int32_t reserved;
} irmv_kernel_stat;

const char *irmv_last_error(void);
const char *irmv_version(void);
int irmv_device_count(int *count);
int irmv_device_synchronize(int device);   /* hipDeviceSynchronize on that device */

void irmv_engine_cfg_default(irmv_engine_cfg *cfg);
int irmv_engine_create(const irmv_engine_cfg *cfg, irmv_engine **out);
void irmv_engine_destroy(irmv_engine *e);
int irmv_engine_num_slots(const irmv_engine *e);
int irmv_engine_max_det(const irmv_engine *e);
int irmv_engine_num_streams(const irmv_engine *e);
int irmv_engine_sync_launch(const irmv_engine *e);   /* how a synchronous single-frame step is launched on this box: 0 = one hipGraph replay, 1 = kernel by kernel
                                                        behind the upload (same kernels, same bits; timed at creation, IRMV_SYNC_LAUNCH=graph|eager forces) */

/* ---- NUMA placement of the frame hand-off (multi-GPU nodes; the reference is single-device, test/yolo_test.cpp:16) ----
 * An engine allocates and first-touches its pinned frame slots on the host NUMA node closest to its device
 * (hipDeviceAttributeHostNumaId; IRMV_NUMA=0 switches that off).  The threads that FILL the slots and submit belong on the
 * same node: a runner binds each of them with irmv_numa_bind_thread(node of its device) before it creates the engine. */
int irmv_engine_numa_node(const irmv_engine *e);     /* host NUMA node of the engine's device; -1 unknown */
int irmv_engine_numa_placed(const irmv_engine *e);   /* 1: the frame slots were allocated under that node's CPU set and memory policy */
int irmv_numa_device_node(int device, int *node);    /* the same attribute without an engine (before irmv_engine_create) */
int irmv_numa_bind_thread(int node);                 /* sched_setaffinity(calling thread, CPUs of /sys/devices/system/node/nodeN/cpulist within the process's cpuset) */
int irmv_numa_page_node(const void *p);              /* node holding the page of p (move_pages query); < 0 unknown */
int irmv_numa_parse_cpulist(const char *s, int *cpus, int cap);   /* "0-3,8" -> {0,1,2,3,8}; returns the count (test aid) */

/* Pinned host frame slot, valid for the engine's lifetime; producer threads write straight into it -- the counterpart
 * of YoloEngine::get_src_image_buffer() (yolo_engine.hpp:35) and of the TripleBuffer hand-off
 * (include/irmv_detection/triple_buffer.hpp:24-40).  It holds irmv_engine_src_bytes() bytes: src_height*src_width*3
 * (HWC u8) for IRMV_SRC_HWC8, src_height*src_width (the raw CFA frame, row-major) for the Bayer formats. */
uint8_t *irmv_engine_src_buffer(irmv_engine *e, int slot);
/* Device-side staging of the same slot, in the same format (for producers that already hold the frame in HBM -- a Bayer
 * producer writes the raw frame here and submits without IRMV_SUBMIT_H2D -- and for HBM-resident benchmarking). */
void *irmv_engine_src_device_buffer(irmv_engine *e, int slot);
/* ---- tracking window (irmv_engine_cfg.win_width / win_height) ----
 * (x0, y0): the window's top-left corner in the coordinates detections come back in -- the rotated frame when rotate180 = 1,
 * the frame a tracker sees.  The call waits until the slot's last submitted step is done, then writes the slot's corner and
 * shifted camera into device memory; it takes effect from the slot's next submit, and no captured graph changes.  Results
 * read later with irmv_engine_results still carry the corner their step was submitted with.
 * IRMV_ERR_ARG: null engine, an engine without a window, a slot out of range, a window not inside the frame. */
int irmv_engine_set_window(irmv_engine *e, int slot, int x0, int y0);
/* The slot's current corner and the window's size (any pointer may be NULL). */
int irmv_engine_get_window(const irmv_engine *e, int slot, int *x0, int *y0, int *w, int *h);
/* Host only: where a window at (x0, y0) lies -- the function the engine itself builds from.  cfg must have a window. */
typedef struct irmv_window_map_t {
    int32_t bx0, by0;        /* the corner in buffer coordinates: rotate180 ? src_width - x0 - win_width : x0, likewise y */
    uint64_t band_offset;    /* the full-width rows the window covers, as bytes of an HWC frame: by0 * src_width * 3 ... */
    uint64_t band_bytes;     /* ... and win_height * src_width * 3 (what a band upload moves) */
    double cx, cy;           /* the principal point of the window's pixels: camera_matrix[2] - x0, camera_matrix[5] - y0 */
    int32_t reserved[4];
} irmv_window_map_t;
int irmv_window_map(const irmv_engine_cfg *cfg, int x0, int y0, irmv_window_map_t *out);

/* ---- search view: a window engine runs a slot's step on the whole frame on demand ----
 * Per-slot state, like the window's corner.  A slot in IRMV_VIEW_FRAME behaves as a slot of an engine WITHOUT a window on the
 * same src_width x src_height frame, net, weights, camera and switches: no crop; the front reads the full frame where the
 * uploads or the demosaic put it, with the plan irmv_front_plan gives for win_* = 0 (so the two views may differ in whether
 * the front runs fused, and on which of its paths); results are scaled by the full frame's factors and carry no offset; PnP
 * sees the configured camera.  Uploads follow the view at submit time: in the frame view whole frames move, never a band and
 * never the crop out of the pinned slot; a submit without IRMV_SUBMIT_H2D reads the device frame as it is.  Everything that acts
 * on "the slot's frame" -- the read-backs, irmv_engine_run_post, irmv_engine_profile, irmv_engine_extract_armors,
 * irmv_engine_light_trace, irmv_engine_rotated_image -- acts on the slot's current view.
 * irmv_engine_set_view waits for the slot's last submitted step and takes effect from the slot's next submit; results read
 * later still carry the view (and, in the window view, the corner) their step was submitted with.  Switching back and forth
 * re-captures nothing: each (slots, step kind, view) graph is captured once.  All slots of one irmv_engine_submit must be in
 * one view (IRMV_ERR_ARG otherwise, before anything is enqueued).  irmv_engine_set_window stays allowed in the frame view: it
 * records the corner, which is in force again when the slot returns to the window view.
 * The first IRMV_VIEW_FRAME of an engine builds the frame view (tap tables, launch lists, the larger scratch of the classical
 * extraction and of irmv_engine_rotated_image) after waiting for every step in flight, as irmv_engine_set_bayer_isp does: call
 * it once at start-up to pay that there.  An engine on which it is never called allocates and runs what it always did.
 * IRMV_ERR_ARG: null engine, an engine without a window, a slot out of range, an unknown view, a frame view whose letterboxed
 * frame would have no row or no column (the rule of irmv_engine_create); the engine stays usable. */
#define IRMV_VIEW_WINDOW 0   /* the slot's step runs on its window (what every window engine does until told otherwise) */
#define IRMV_VIEW_FRAME  1   /* ... on the whole src_width x src_height frame, into the same net input */
int irmv_engine_set_view(irmv_engine *e, int slot, int view);
/* The slot's view and the size of the source frame its steps see: the window's, or the full frame's (any pointer may be NULL). */
int irmv_engine_get_view(const irmv_engine *e, int slot, int *view, int *src_w, int *src_h);
/* Read-only (tests): the hipGraphExec objects the engine holds. */
int irmv_engine_debug_graph_count(const irmv_engine *e);

int irmv_engine_src_format(const irmv_engine *e);      /* IRMV_SRC_* of this engine; -1 for a null engine */
size_t irmv_engine_src_bytes(const irmv_engine *e);    /* bytes of one source slot (host and device); 0 for a null engine */

/* Without IRMV_SUBMIT_H2D a step reads the slot's device frame as it is: what a producer wrote through
 * irmv_engine_src_device_buffer, what the last WHOLE upload of the slot left there (a step with IRMV_SUBMIT_H2D in the frame
 * view, of a Bayer engine or of an engine without a window; a tiled step's frame_slot), or what an on-demand entry loaded
 * (irmv_engine_rotated_image, _render, _meter, _extract_armors, _refine_points, _light_trace: the pinned frame as it was at
 * that call -- on an HWC window engine in the window view only the rows under the window of that call).  A window-view step
 * with IRMV_SUBMIT_H2D of an HWC window engine leaves the device frame UNSPECIFIED: it uploads the window's band, or crops
 * out of the pinned slot and uploads nothing, as the launch form decides. */
#define IRMV_SUBMIT_H2D 1u          /* copy the pinned slots -> HBM first */
#define IRMV_SUBMIT_ASYNC_UPLOAD 2u /* ... on the engine's upload stream, event-chained to the compute stream: this
                                       group's frames cross PCIe while other groups' kernels run (one cross-stream hop) */

/* ---- tiled search: one frame as overlapping windows in one step, merged ------------------------------------------------
 * The frame view squeezes the frame into the net; a tiled step searches it at the sensor's resolution instead.  N slots of a
 * window engine -- the tiles, each with its own corner (irmv_engine_set_window: data, moving a tile re-captures nothing) --
 * run ONE step in which every slot's crop cuts its window out of the full frame of ONE slot, frame_slot.  Behind the crop each
 * slot is what it always is: the same kernels and the same bits as a window engine's step of that slot on that frame, so
 * irmv_engine_results(slot), the read-backs and the classical point source work per tile.  The step's last node merges the N
 * result lists into one, in full-frame coordinates (k_tiles.hip; irmv_detection_amd/tiles.py is the bit-exact host reference).
 * Tiling is a way of submitting, not a view: irmv_engine_set_view knows IRMV_VIEW_WINDOW and IRMV_VIEW_FRAME only.
 *
 * The merge.  Every coordinate is the fp32 value irmv_engine_results returns, float(local) + float(corner).  Tile t is slot
 * first + t with corner (x0, y0), window ww x wh, frame FW x FH; m = edge_margin.
 *   seam cut  a record is cut if  x0 > 0 && X1 < float(x0) + m,  or  y0 > 0 && Y1 < float(y0) + m,
 *             or  x0 + ww < FW && X2 > float(x0 + ww) - m,  or  y0 + wh < FH && Y2 > float(y0 + wh) - m:
 *             its box touches an edge of its tile that is not an edge of the frame, so the tile may have seen a part of it.
 *   order     (cut ascending, score descending, tile ascending, index ascending): whole boxes first.
 *   walk      in that order a record is kept unless an already kept record of a DIFFERENT tile and the SAME class_id has
 *             inter > ios_thr * min(area_a, area_b) with it -- intersection over the smaller area, no division --, where
 *             inter = max(0, min(X2) - max(X1)) * max(0, min(Y2) - max(Y1)) and area = (X2 - X1) * (Y2 - Y1), plain fp32.
 *             Records of one tile never suppress each other (their own NMS has ruled).  It stops at max_det kept records.
 * Capacity: IRMV_MAX_TILES x IRMV_MAX_DET_CAP = 4096 records, sorted and walked by one workgroup out of LDS.
 * The merge's buffers are allocated by an engine's first tiled call; an engine on which none is made allocates, captures and
 * runs what it always did, and the merge is no entry of irmv_engine_ops. */
#define IRMV_MAX_TILES 16
typedef struct irmv_tile_det {
    irmv_det det;            /* byte-identical to record `index` of irmv_engine_results(first + tile) */
    int32_t tile, index;     /* the slot (first + tile) and the place in its list the record comes from */
    int32_t cut;             /* 1: the seam cut applies to it (it was kept all the same: nothing whole covered it) */
    int32_t reserved;
} irmv_tile_det;
/* Host only, no GPU (like irmv_window_map / irmv_front_plan): the grid the engine documents.  cfg must have a window.  Per axis,
 * with frame extent F, window extent w and least overlap 0 <= ov < w: n = 1 tiles if w == F, else ceil((F - ov) / (w - ov)),
 * with corners c_i = (2 i (F - w) + (n - 1)) / (2 (n - 1)) in integers (0 when n == 1): the fewest tiles that cover the axis,
 * spread evenly, neighbours overlapping by at least ov.  Tiles are row-major, t = iy * nx + ix; xy[t] = (x, y) in result
 * coordinates, as irmv_engine_set_window takes them.  xy == NULL queries *n (and *nx, *ny; either may be NULL).
 * 1280 x 1024, window 640 x 512, overlap 128: 3 x 3, x 0 320 640, y 0 256 512.
 * IRMV_ERR_ARG: no window, an overlap out of range, more than IRMV_MAX_TILES tiles, cap smaller than the grid. */
int irmv_tile_grid(const irmv_engine_cfg *cfg, int min_overlap_x, int min_overlap_y,
                   int32_t *xy /* [cap][2] */, int cap, int *n, int *nx, int *ny);
/* One tiled step of slots [first, first + count), 1 <= count <= IRMV_MAX_TILES, all in IRMV_VIEW_WINDOW, on the full frame of
 * frame_slot (any slot of the engine, inside or outside the range).  With IRMV_SUBMIT_H2D only frame_slot's pinned frame
 * crosses PCIe, once and whole -- never as bands, never cropped out of the pinned slot; IRMV_SUBMIT_ASYNC_UPLOAD moves that
 * upload to the upload stream as it does for irmv_engine_submit; without IRMV_SUBMIT_H2D the device frame of frame_slot is read
 * as it is.  A Bayer engine demosaics frame_slot's raw frame once.  The pinned and device frames of the other slots are
 * neither read nor written.
 * The step is ONE slot group: one captured graph -- [upload], [demosaic], crop, the slots' step, merge -- replayed on compute
 * stream 0 of the engine (the stream of slot 0's single-slot steps), captured once per (frame_slot, first, count, upload
 * form).  It is ordered against other groups like every submit; frame_slot counts as touched, so a later upload into it
 * waits for this step.  irmv_engine_wait_slots(e, first, count) covers the merge.  A tiled step keeps the slots' result records
 * in device memory (the merge reads them there) and copies them to the host behind the merge, also on engines whose ordinary
 * steps write their records straight into pinned memory.
 * IRMV_ERR_ARG, before anything is enqueued and leaving the engine usable: an engine without a window, a slot in the frame
 * view, a bad range, count or frame_slot. */
int irmv_engine_submit_tiles(irmv_engine *e, int frame_slot, int first, int count, uint32_t flags);
/* Test hook, like irmv_engine_run_post: waits for everything in flight, runs the merge alone on the current results of slots
 * [first, first + count) (e.g. of irmv_engine_write_head + irmv_engine_run_post) at the slots' current corners, and
 * synchronizes.  From then on irmv_engine_results reads those slots' records in these corners. */
int irmv_engine_merge_tiles(irmv_engine *e, int first, int count);
/* The merged list of the last tiled step (after its wait) or irmv_engine_merge_tiles whose first slot was `first`: up to cap
 * records in merge order, *n of them; *n_in (may be NULL) = the records that entered the merge.  The records are read out of the
 * slots' result lists: they are valid until one of those slots is stepped again.  IRMV_ERR_ARG if no merge has run for `first`. */
int irmv_engine_tile_results(irmv_engine *e, int first, irmv_tile_det *out, int cap, int *n, int *n_in);
/* The merge's two parameters, two floats in device memory that the merge kernel reads when it runs: like
 * irmv_engine_set_class_policy the call waits for every step in flight and re-captures nothing.  Defaults: ios_thr = 0.5 (the
 * usual default of sliced inference), edge_margin = 2.0 source pixels.  Neither has been validated on a trained model -- none
 * exists here --, which is why both are live.  IRMV_ERR_ARG: ios_thr outside (0, 1] or NaN, a negative or NaN margin. */
int irmv_engine_set_tile_merge(irmv_engine *e, float ios_thr, float edge_margin);
int irmv_engine_get_tile_merge(const irmv_engine *e, float *ios_thr, float *edge_margin);

/* Enqueue one step for slots [first, first+count) and return immediately:
 *   [async H2D of the frames] -> ONE hipGraph {preprocess -> network -> decode -> NMS -> keypoints -> PnP} ->
 *   async D2H of the results.
 * With IRMV_SUBMIT_ASYNC_UPLOAD the upload rides a side stream -- the dGPU form of the reference's TripleBuffer
 * hand-off (triple_buffer.hpp:24-40, src/camera.cpp:40-61): submit slot n+1 while slot n is in flight, collect each
 * with irmv_engine_wait_slots().  count == 1 is the reference's per-slot detect(); count > 1 batches independent
 * frames through every kernel.  One thread submits.
 * A multi-slot step is cut into one sub-batch (one captured graph) per compute stream of the engine; a submit of exactly
 * one stream's share of the engine's slots, aligned to it (e.g. slots [128, 256) of a 256-slot, two-stream engine), IS
 * that sub-batch -- the same graph on the same stream -- so a producer may feed the shares separately. */
int irmv_engine_submit(irmv_engine *e, int first_slot, int count, uint32_t flags);
/* Block until everything submitted so far is done and host-visible. */
int irmv_engine_wait(irmv_engine *e);
/* Block until the pinned slots [first, first+count) have been uploaded by their last submit: a producer may overwrite them
 * from then on (the TripleBuffer's consumer can give the buffer back) while the kernels still run. */
int irmv_engine_wait_upload(irmv_engine *e, int first_slot, int count);
/* Block until the results of slots [first, first+count) are host-visible; other slots stay in flight. */
int irmv_engine_wait_slots(irmv_engine *e, int first_slot, int count);
/* Results of one slot after wait(): up to cap detections, score-descending. */
int irmv_engine_results(irmv_engine *e, int slot, irmv_det *out, int cap, int *n);
/* submit(slot, 1, H2D) + wait + results == YoloEngine::detect() (src/yolo_engine.cpp:153-177) */
int irmv_engine_detect(irmv_engine *e, int slot, irmv_det *out, int cap, int *n);
/* Wall-clock ms of the last detect() (get_profiling_time(), yolo_engine.hpp:33) */
double irmv_engine_last_detect_ms(const irmv_engine *e);

/* 180-degree rotated frame of a slot (what get_rotated_image() aliases after the
 * in-place mirror, src/yolo_engine.cpp:77-78,182-184), rotated on the GPU.  dst_hwc
 * receives src_height*src_width*3 bytes in every format: a Bayer engine uploads the
 * raw slot, demosaics it and returns the rotated R, G, B frame.  A window engine
 * returns the rotated window: win_height*win_width*3 bytes -- or, for a slot in
 * IRMV_VIEW_FRAME, the rotated full frame: src_height*src_width*3 bytes.
 * On demand, callable at any time: the call waits for the slot's own step in flight (as irmv_engine_wait_slots(slot, 1) does;
 * other slots stay in flight), then loads the slot's pinned frame AS IT IS NOW into the device frame -- in the window view of
 * an HWC window engine the band of rows under the window -- and returns its rotation.  A step of the slot that was in flight
 * keeps the frame it was submitted with, also where the producer has overwritten the pinned slot since
 * irmv_engine_wait_upload. */
int irmv_engine_rotated_image(irmv_engine *e, int slot, uint8_t *dst_hwc);

/* ---- debug images: the node's visualized and binary frames, rendered on the GPU -----------------------------------------
 * What the reference node publishes in debug mode (src/irm_detector.cpp:259-280): the frame with the armors and boxes drawn on
 * it, and gray -> threshold -> three channels with the boxes.  One kernel (k_render.hip render_view) produces either from the
 * slot's device frame, optionally at 1/2 or 1/4 size, and only the finished picture crosses PCIe.  On demand, like
 * irmv_engine_rotated_image, and no part of a captured step: the call waits for what is in flight, loads the slot's current
 * frame (a Bayer engine's demosaiced, a window slot's cropped; IRMV_VIEW_FRAME: the full frame), copies the marks to a device
 * scratch, launches once, copies the picture back and synchronizes.  Its scratch is allocated by the first call; it captures
 * and drops no graph.  irmv_detection_amd/render.py is the host reference, bit for bit:
 *   R        the W x H frame of the slot's view in the coordinates detections come back in (rotated under cfg.rotate180: what
 *            irmv_engine_rotated_image returns), channels as stored;  output ow = W / s, oh = H / s, trailing source columns and
 *            rows dropped
 *   colour   per channel (sum of the s x s block of R + s*s/2) / (s*s)
 *   binary   255 on all three channels where any pixel of the block has gray > T,
 *            gray = (p0*3735 + p1*19235 + p2*9798 + (1<<14)) >> 15 (the light extraction's), else 0
 *   marks    every float truncated toward zero, a window slot's corner subtracted, floor-divided by s.  A record with a
 *            non-finite xyxy value or one of magnitude >= 2^24 gets no box and no label; one with such a kpts value or
 *            armor_valid != 1 no armor mark.  First the armor marks of every record, then per record its box and its label;
 *            later marks overwrite earlier ones.
 *   box      2-px lines, (0,0,255) for classes 0..6, (255,0,0) otherwise; label: the ArmorClass name (class_id outside 0..13:
 *            UNKNOWN) in the 5 x 7 font of irmv_render_glyph, cell 3, 2, 1 px for s = 1, 2, 4, bottom-left corner at the box's
 *            first corner -- at s = 1 exactly YoloEngine::visualize_bboxes without OpenCV
 *   armor    green (0,255,0): a ring of radius r = 5, 3, 2 at LB, LT, RT, RB (|dx^2 + dy^2 - r^2| <= 2r) and the segments
 *            LT-LB, RT-RB, LT-RT, LB-RB: every pixel within distance 1 of the segment, in 64-bit integers */
#define IRMV_RENDER_COLOR  0
#define IRMV_RENDER_BINARY 1
#define IRMV_MARK_BOXES  1u
#define IRMV_MARK_LABELS 2u
#define IRMV_MARK_ARMORS 4u
typedef struct irmv_render_opts {
    uint32_t struct_size;      /* = sizeof(irmv_render_opts) */
    int32_t kind;              /* IRMV_RENDER_* */
    int32_t scale;             /* 1, 2 or 4 */
    uint32_t marks;            /* IRMV_MARK_* bits */
    int32_t binary_threshold;  /* 0..255, or -1 = the engine's current one (irmv_engine_set_extract_params) */
    int32_t reserved[3];       /* must be 0 */
} irmv_render_opts;
/* The picture's size at `scale` for the slot's current view. */
int irmv_engine_render_dims(const irmv_engine *e, int slot, int scale, int *w, int *h);
/* dets == NULL with n == -1: the slot's last results, as irmv_engine_results returns them (a slot never stepped has none;
 * creation may have stepped slot 0 on its empty frame to time detect()'s launch form);
 * otherwise 0 <= n <= max_det explicit records, of which xyxy, class_id, kpts and armor_valid are read.  dst_hwc receives
 * h * w * 3 bytes.  IRMV_ERR_ARG (a null engine, opts or dst, a wrong struct_size, an unknown kind, a scale other than 1, 2, 4,
 * unknown mark bits, non-zero reserved fields, a threshold outside -1..255, a bad slot or n) leaves the engine as it was. */
int irmv_engine_render(irmv_engine *e, int slot, const irmv_render_opts *o, const irmv_det *dets, int n, uint8_t *dst_hwc);
/* Host only: the 5 x 7 glyph the kernel draws for ch, row 0 on top, bit 4 the leftmost column; IRMV_ERR_ARG if there is none.
 * The device table is uploaded from this one. */
int irmv_render_glyph(int ch, uint8_t rows[7]);

/* The gains and tone curve of a Bayer engine, changeable while it lives (the camera SDK's ISP retuned per venue):
 *   out = lut[c][min(255, (v * gain_q8[c] + 128) >> 8)]   per channel c = R, G, B,
 * v the interpolated value.  gain_q8: Q8 in [0, 1023]; lut: [3][256] bytes, rows R, G, B, NULL = identity (then exactly the
 * arithmetic of bayer_gain_q8).  The engine folds both into one [3][256] byte table in device memory that the demosaic
 * kernel stages in LDS.  The call blocks until every step in flight on every stream of the engine has finished, then
 * writes the table: every later submit, detect, irmv_engine_rotated_image and irmv_engine_extract_armors uses it.  An engine
 * on which it was never called (and whose bayer_demosaic is bilinear) keeps the kernel that takes the gains as arguments;
 * the first call drops the captured graphs that hold that kernel, and they are captured again with the table kernel.
 * IRMV_ERR_ARG: null engine, an IRMV_SRC_HWC8 engine, null gain_q8, a gain above 1023. */
int irmv_engine_set_bayer_isp(irmv_engine *e, const uint16_t gain_q8[3], const uint8_t *lut);
/* The current gains and LUT (either pointer may be NULL); the LUT of an engine that has none set is the identity. */
int irmv_engine_get_bayer_isp(const irmv_engine *e, uint16_t gain_q8[3], uint8_t *lut);

/* ---- class policy: per-class score thresholds, colour mask, plate size ------------------------------------------------
 * One score threshold and one plate model per class, in a small table in device memory that every kernel deciding "is this
 * (anchor, class) pair a candidate" reads when it runs, as does the place that picks PnP's object points.  A class that is
 * off is off where candidates are emitted: it sets no candidate bit, appends no key and is not counted, so nothing behind
 * the class carriers (head rows, the gated box and keypoint launches, the NMS walk) does any work for it.
 * irmv_raw_dets.n_candidates counts the pairs that pass their own class's threshold; pre_nms_cap, max_det and NMS act on
 * that list as they always did.  An engine on which irmv_engine_set_class_policy is never called runs the uniform policy of
 * cfg.score_thr / cfg.armor_size: the same float compared with the same float, the same plate.
 * irmv_detection_amd/class_policy.py is the host reference. */
typedef struct irmv_class_policy {
    uint32_t struct_size;    /* = sizeof(irmv_class_policy) */
    float    score_thr[16];  /* class c < nc: in (0,1) -> (anchor, c) is a candidate iff logit > float32(log(t/(1-t))),
                                evaluated in double on the float32 t -- the arithmetic cfg.score_thr gets;
                                >= 1: the class is off (threshold +inf).  <= 0 or NaN: IRMV_ERR_ARG.  Entries >= nc ignored */
    uint8_t  plate[16];      /* IRMV_ARMOR_SMALL / _LARGE: object points PnP uses for a detection of class c (keypoint head, and
                                the classical extraction of a step's detections; irmv_engine_extract_armors on explicit
                                boxes has no class and keeps cfg.armor_size).  irmv_det.armor_size of the keypoint path
                                reports it; the classical path's stays the size the light gates classify */
} irmv_class_policy;
/* Waits for every step in flight on every stream of the engine, then writes the table with a small synchronous copy: the new
 * policy holds from the next submit.  No captured graph changes: the graphs hold the table's address, never its contents.
 * p == NULL: back to cfg.score_thr / cfg.armor_size for every class.  IRMV_ERR_ARG (null engine, wrong struct_size, a
 * threshold <= 0 or NaN, a plate other than IRMV_ARMOR_SMALL / _LARGE) leaves policy and engine as they were. */
int irmv_engine_set_class_policy(irmv_engine *e, const irmv_class_policy *p);
int irmv_engine_get_class_policy(const irmv_engine *e, irmv_class_policy *out);
/* Host only, no GPU touched.  _uniform: every class at score_thr (> 0; >= 1: off) with plate armor_size.
 * _enemy: the reference node's enemy_color ("0 for blue, 1 for red", src/irm_detector.cpp:154-160), which it declares and
 * never uses: 0 = the enemy is blue -> B1..BS (classes 0..6) on at score_thr, R1..RS (7..13) off; 1 = the enemy is red ->
 * the reverse; -1 = both on (= _uniform).  Classes 14 and 15 stay on. */
int irmv_class_policy_uniform(float score_thr, int armor_size, irmv_class_policy *out);
int irmv_class_policy_enemy(int enemy_color, float score_thr, int armor_size, irmv_class_policy *out);
/* The table the engine uploads for a model of nc classes (1..16), and every check irmv_engine_set_class_policy runs -- the
 * function the engine itself builds from, as irmv_window_map / irmv_front_plan are.  logit_thr[c] for c >= nc is +inf;
 * *min_logit_thr = the smallest entry (+inf: every class off), the kernels' wave-uniform pre-test. */
int irmv_class_policy_table(const irmv_class_policy *p, int nc, float logit_thr[16], float *min_logit_thr);

/* IrmDetector::extract_armors(get_rotated_image(), bboxes) (src/irm_detector.cpp:183,292-355) on the GPU:
 * for each of the n boxes (xyxy, rotated-frame pixels) on the slot's current frame -> out[i].kpts (LB, LT, RT,
 * RB), armor_valid, armor_size, n_lights, and the PnP pose.  Works for any model / point_source.  A window engine takes the
 * boxes and returns kpts in the full frame's coordinates and looks at the slot's current window (IRMV_VIEW_FRAME: at the
 * whole frame). */
int irmv_engine_extract_armors(irmv_engine *e, int slot, const float *xyxy, int n, irmv_det *out);
/* The node's live parameters of that extraction (IrmDetector::param_event_callback, src/irm_detector.cpp:372-403):
 * binary_threshold, light.{min_ratio,max_ratio,max_angle}, armor.{min_small,max_small,min_large,max_large}_center_distance.
 * Takes effect from the next submit / extract call. */
int irmv_engine_set_extract_params(irmv_engine *e, int binary_threshold, float light_min_ratio, float light_max_ratio,
                                   float light_max_angle, const double center_distances[4]);
/* IRMV_POINTS_KEYPOINT_HEAD, IRMV_POINTS_CLASSICAL or IRMV_POINTS_REFINED: where this engine's four armor points come from
 * (AUTO resolved). */
int irmv_engine_point_source(const irmv_engine *e);

/* ---- refined point source (IRMV_POINTS_REFINED) ------------------------------------------
 * A refined engine runs the keypoint engine's step; behind the NMS a guided light extraction (one more launch, profile name
 * light_refine) takes each detection's four keypoints LB, LT, RT, RB as a prior and replaces them by the ends of the light
 * bars found at them.  Where no bar is found the head's points and pose stay untouched.  Per detection, all in fp32 and in
 * the written association order, in the pixels of the frame of the slot's view (a window engine: the window's):
 *   1. All eight keypoint values are finite and below 2^24 in magnitude; else flag 0, n_lights 0, nothing is extracted.
 *   2. Guided ROI: gx1 = min(x1, min kx) - roi_margin, gy1 = min(y1, min ky) - roi_margin, gx2 = max(x2, max kx) + roi_margin,
 *      gy2 = max(y2, max ky) + roi_margin, then clamped to the frame and truncated like a bbox of the classical source.  The
 *      label pool is handed out in detection order over these ROIs.  (A bar that ends at the bbox's edge would be cut by the
 *      bbox's own ROI and measure a stump: hence the margin.)
 *   3. Lights as the classical source finds them (threshold, external contours of >= 5 points, minimum-area rectangle,
 *      is_light); n_lights counts those of the ROI.
 *   4. Side L: (B, T) = (kpts[0..1], kpts[2..3]); side R: (B, T) = (kpts[6..7], kpts[4..5]).  A light with ends b (bottom),
 *      t (top) has cost = ((b.x-B.x)^2 + (b.y-B.y)^2) + ((t.x-T.x)^2 + (t.y-T.y)^2) and, with len2 = (B.x-T.x)^2 + (B.y-T.y)^2,
 *      is admissible for the side iff cost <= (snap * snap) * len2.
 *   5. Per side the admissible light of least cost; on equal cost the contour found later (the classical source prefers the
 *      same direction).
 *   6. Refined iff both sides have a light, the two are different contours and PnP on {L.bottom, L.top, R.top, R.bottom}
 *      succeeds -- with the plate the keypoint path uses (the class policy's plate[cls]; cfg.armor_size for explicit boxes) and
 *      the slot's camera.  Then kpts, rvec, tvec, quat and pnp_ok are replaced; a quad PnP refuses changes nothing.
 *   7. armor_valid stays 1, armor_size the policy's plate; irmv_raw_dets.det_kpts stay the net's output.
 *   8. irmv_det.reserved carries the flag (see there).
 * The two parameters are live like the tile merge's: the kernel reads them from device memory when it runs, the setter waits
 * for every step in flight and re-captures nothing.  Defaults: snap = 0.5, allowed (0, 4]; roi_margin = 4.0 source pixels,
 * allowed [0, 64].  Neither default has been validated on a trained model -- none exists here --, which is why both are live.
 * IRMV_ERR_ARG (and nothing changes): a value outside its range or NaN.  Both calls work on an engine of any point source:
 * irmv_engine_refine_points uses the parameters.  irmv_detection_amd/refine.py is the host reference of rules 1, 2, 4, 5, 8. */
int irmv_engine_set_refine(irmv_engine *e, float snap, float roi_margin);
int irmv_engine_get_refine(const irmv_engine *e, float *snap, float *roi_margin);

/* ---- pose ambiguity: both IPPE solutions per armor, and a gravity prior ------------------------------------------------
 * IPPE has two solutions per plate, mirror images about the line of sight.  A is the one cv::solvePnP(SOLVEPNP_IPPE) reports
 * -- solution 0 unless !(err0 <= err1) --, B the other.  For a 135 x 55 mm plate a few metres away the two residuals differ
 * by less than the keypoint noise, and the reported yaw flips between the mirror poses from frame to frame.  From the first
 * irmv_engine_set_pose_prior on, a step delivers BOTH (irmv_engine_pose_alts, as cv::solvePnPGeneric does) and, in mode
 * IRMV_POSE_PRIOR, chooses between them by what the scene knows and IPPE does not use: a plate is mounted at a known tilt
 * against gravity, and the gimbal knows where "up" is.
 * The rule, fp64 in the written order (no fused multiply-add), per detection of class c in slot k:
 *   n_X    = column 0 of R_X (R_X[0], R_X[3], R_X[6] row-major): the model x axis in camera coordinates, the plate normal
 *            pointing AWAY from the camera
 *   u      = the slot's unit up vector (irmv_engine_set_up), s = normal_up[c]: the class's expected n . u
 *   cost_X = fabs(((R_X[0]*u.x + R_X[3]*u.y) + R_X[6]*u.z) - s)
 *   report B  iff  mode == IRMV_POSE_PRIOR  &&  errB <= ambiguity_ratio * errA  &&  costB < costA
 * Any NaN makes a comparison false: A stays.  rvec and quat of either pose are converted as always; pnp_ok keeps its meaning
 * (a failed translation of either solution fails the call, then the reported pose's finiteness).  A robot plate whose outward
 * normal points 15 degrees upward has s = -sin 15 deg = -0.25881904510252074 (the outpost's: +); the library takes s, not
 * an angle, so neither side does trigonometry.  irmv_detection_amd/pose_prior.py is the bit-exact host reference.
 * An engine on which irmv_engine_set_pose_prior is never called allocates nothing for this, launches the kernels it always
 * launched and returns the bits it always returned.  The first call allocates the side records, the prior table and the up
 * table and drops the captured graphs once (as the first irmv_engine_set_bayer_isp does); later calls and every
 * irmv_engine_set_up rewrite device memory the kernels read when they run and re-capture nothing.  In mode IRMV_POSE_MIN_ERR
 * an enabled engine's irmv_det records stay byte-identical to a never-enabled engine's.
 * Window engines: the crop only moves the principal point, so u is the same in the window and the frame view and for any
 * corner.  rotate180: u is in the frame PnP sees, the rotated one.  Explicit boxes (irmv_engine_extract_armors,
 * irmv_engine_refine_points) have no class: the rule runs with normal_up_default and no alt record is exposed -- the rule the
 * plate follows there.  Classical and refined engines: the record is the alt of the quad whose pose irmv_det finally reports.
 * Tiled steps: the alt of merged record r is irmv_engine_pose_alts(first + r.tile)[r.index].
 * The default ambiguity_ratio = 8 rests on a CPU experiment alone (the project's fp64 reference on synthetic corner noise: at
 * 0.3 px the min-error rule reports the mirror pose in 25 - 27 % of the poses of a plate leaning back 15 degrees, this rule in
 * 7 - 12 %; ratios 2, 8 and +inf within that range).  No trained keypoint head exists here, which is why every parameter is live. */
#define IRMV_POSE_MIN_ERR 0   /* cv::solvePnP's choice (default) */
#define IRMV_POSE_PRIOR   1
typedef struct irmv_pose_prior {
    uint32_t struct_size;        /* = sizeof(irmv_pose_prior) */
    int32_t  mode;               /* IRMV_POSE_* */
    double   ambiguity_ratio;    /* >= 1, +inf allowed (the cost alone decides); default 8 */
    double   normal_up[16];      /* per class, in [-1, 1]; default -0.25881904510252074 (a robot's plate) */
    double   normal_up_default;  /* detections without a class (explicit boxes) */
} irmv_pose_prior;
typedef struct irmv_pose_alt {
    double  rvec[3], tvec[3], quat[4];   /* the solution irmv_det does NOT report */
    double  err, err_alt;                /* the solver's rms normalised residual of irmv_det's pose / of this one */
    int32_t state;                       /* 0: pnp_ok == 0, nothing here (all zero); 1: irmv_det holds A; 2: the prior reported B */
    int32_t alt_ok;                      /* this pose's own finiteness check */
} irmv_pose_alt;
/* Waits for every step in flight on every stream of the engine, as irmv_engine_set_class_policy does.  p == NULL: mode
 * IRMV_POSE_MIN_ERR with the defaults; the records are still delivered.  IRMV_ERR_ARG, before the GPU is touched and leaving
 * everything as it was: a null engine, a wrong struct_size, an unknown mode, a ratio < 1 or NaN, |normal_up| > 1 or NaN
 * (all 16 entries and the default). */
int irmv_engine_set_pose_prior(irmv_engine *e, const irmv_pose_prior *p);
int irmv_engine_get_pose_prior(const irmv_engine *e, irmv_pose_prior *out);   /* before the first set: the defaults */
/* The slot's up vector, normalised on the host: v / sqrt((x*x + y*y) + z*z).  Default (0, -1, 0): a level camera (image y
 * points down).  Waits for the slot's last step, as irmv_engine_set_window does; works before the first
 * irmv_engine_set_pose_prior (the value is kept and uploaded then).  IRMV_ERR_ARG: a slot out of range, a zero, non-finite
 * or NaN vector (also one whose squared length overflows). */
int irmv_engine_set_up(irmv_engine *e, int slot, const double up[3]);
int irmv_engine_get_up(const irmv_engine *e, int slot, double up[3]);   /* the unit vector in force */
/* Parallel to irmv_engine_results: out[i] belongs to record i of the slot's last step; *n = min(num_dets, cap).  The records
 * reach the host the way the slot's irmv_det records do.  IRMV_ERR_ARG before the first irmv_engine_set_pose_prior. */
int irmv_engine_pose_alts(irmv_engine *e, int slot, irmv_pose_alt *out, int cap, int *n);

/* ---- constrained pose: the plate's yaw at its known tilt ---------------------------------------------------------------
 * The prior above only chooses between two noisy IPPE poses.  A plate has ONE free rotational degree of freedom once the
 * slot's up vector u (irmv_engine_set_up), the class's tilt s = n . u (irmv_pose_prior.normal_up) and the fact that a plate's
 * long edge is horizontal are used: four corners then determine one angle and a translation.  From the first
 * irmv_engine_set_yaw_solve on, a step solves that angle for every record with pnp_ok == 1 and armor_valid == 1 in a kernel of
 * its own behind the NMS (behind the light extraction on classical and refined engines) and delivers one side record per
 * detection (irmv_engine_yaw_poses).  irmv_det, irmv_pose_alt and irmv_tile_det stay byte-identical whether or not it is on.
 * The model, fp64 in the written order (no fused multiply-add); irmv_detection_amd/yaw_solve.py states it operation for
 * operation:
 *   per slot, on the host:   g = e_z - (e_z . u) u,  h1 = g / |g|  (the optical axis in the horizontal plane),  h2 = u x h1;
 *                            |g|^2 < horizon_min: the slot has no basis (the camera looks along gravity)
 *   per class, on the host:  c = sqrt(1 - s s);  c == 0: the class has no basis
 *   for tau = tan(psi / 2):  d = 1 + tau tau,  cs = (1 - tau tau) / d,  sn = (2 tau) / d
 *                            n = s u + c (cs h1 + sn h2)   (model x: the normal, away from the camera)
 *                            y = cs h2 - sn h1             (model y: left)
 *                            z = n x y,   R = [n y z]
 *   translation:             the least-squares translation of the IPPE solver for that R, on the same undistorted points
 *   cost q(tau):             the sum of the eight squared normalised residuals; +inf where a corner has depth <= 0, where
 *                            !(n . t > 0) (a plate seen from behind) and where anything is NaN
 * The search: one 64-lane wavefront per detection; lane k evaluates tau_k = lo + ((hi - lo) k) / 63, first on
 * [-tau_max, tau_max]; the lane of least q wins (ties: the lower lane); the next round is [max(tau* - step, -tau_max),
 * min(tau* + step, tau_max)] with step = (hi - lo) / 63; `rounds` rounds.  err = sqrt(q / 8) of the last winner.
 * A record is refused (state -1) where the slot or the class has no basis, where every lane of the first round is +inf, and
 * where the last winner's q is +inf.
 * Nothing is allocated and nothing new is launched until the first irmv_engine_set_yaw_solve.  That call waits for everything
 * in flight, allocates the records and the two tables and drops the captured graphs once; later calls, irmv_engine_set_up
 * and irmv_engine_set_pose_prior rewrite the tables the kernel reads when it runs and re-capture nothing.  enable = 0: the
 * kernel returns at once and irmv_engine_yaw_poses delivers all-zero records.  Before irmv_engine_set_up /
 * irmv_engine_set_pose_prior their documented defaults apply.  Explicit boxes have no such record.  Tiled steps: the record of
 * merged record r is irmv_engine_yaw_poses(first + r.tile)[r.index].
 * Measured on the CPU alone (the reference on synthetic corner noise); no trained keypoint head exists. */
typedef struct irmv_yaw_opts {
    uint32_t struct_size;        /* = sizeof(irmv_yaw_opts) */
    int32_t  enable;             /* 0 | 1 */
    int32_t  rounds;             /* 1 .. 6; default 4 */
    int32_t  reserved;           /* 0 */
    double   tau_max;            /* in (0, 4]; default 1 = +-90 degrees */
    double   horizon_min;        /* in (0, 1); default 1e-4 */
} irmv_yaw_opts;
typedef struct irmv_yaw_pose {
    double  rvec[3], tvec[3], quat[4];
    double  tau, cs, sn, err;            /* the winner's parameter, cos psi, sin psi, rms normalised residual */
    int32_t state;                       /* 0: nothing here (pnp_ok == 0 or armor_valid != 1; all zero); 1: solved; -1: refused */
    int32_t lane[6];                     /* the winning lane of each round; -1: the round did not run */
    int32_t reserved;
} irmv_yaw_pose;
/* IRMV_ERR_ARG before the GPU is touched, leaving everything as it was: a null engine or opts, a wrong struct_size, enable
 * outside {0, 1}, rounds outside 1 .. 6, tau_max outside (0, 4] or NaN, horizon_min outside (0, 1) or NaN, reserved != 0. */
int irmv_engine_set_yaw_solve(irmv_engine *e, const irmv_yaw_opts *opts);
int irmv_engine_get_yaw_solve(const irmv_engine *e, irmv_yaw_opts *opts);   /* before the first set: the defaults with enable = 0 */
/* Parallel to irmv_engine_results, as irmv_engine_pose_alts is.  IRMV_ERR_ARG before the first irmv_engine_set_yaw_solve. */
int irmv_engine_yaw_poses(irmv_engine *e, int slot, irmv_yaw_pose *out, int cap, int *n);

/* ---- pose uncertainty: the first-order covariance of the IPPE and the constrained pose ---------------------------------
 * A tracker behind these records needs a measurement noise per measurement.  From the first irmv_engine_set_pose_cov on, a
 * step computes, for every record with pnp_ok == 1 and armor_valid == 1, the Gauss-Newton covariance of its pose under
 * independent corner noise of sigma_px pixels, in a kernel of its own behind the constrained pose's (behind the NMS / the
 * light extraction where there is none), and delivers one side record per detection (irmv_engine_pose_covs).  irmv_det,
 * irmv_pose_alt, irmv_yaw_pose, irmv_plate_patch, irmv_plate_number and irmv_tile_det stay byte-identical whether or not it is
 * on.  The model, fp64 in the written order (no fused multiply-add, every division a division);
 * irmv_detection_amd/pose_cov.py states it operation for operation:
 *   corners      (nx_i, ny_i): the four undistorted normalised corners the IPPE solver sees for the record's kpts
 *   object       P_i: the corners of the plate the pose was solved with (the record's armor_size)
 *   pose         R from rvec by Rodrigues' formula, sin and cos from two stated series (the device has no libm the host could
 *                follow bit for bit; the series are exact to ~ 1e-15 on the reduced angle); t = tvec
 *   projection   X_i = R P_i + t,  x_i = X_i.x / X_i.z,  y_i = X_i.y / X_i.z
 *   residuals    r_2i = ((x_i - nx_i) fx) / sigma_px,  r_2i+1 = ((y_i - ny_i) fy) / sigma_px -- a PIXEL residual that ignores
 *                the distortion's own Jacobian
 *   parameters   R <- exp([w]x) R, t <- t + tau, ordered (w_x, w_y, w_z, tau_x, tau_y, tau_z) in the CAMERA frame;
 *                dX_i/dw = -[R P_i]x, dX_i/dtau = I; J is the analytic 8 x 6 Jacobian of r
 *   covariance   A = J^T J (each entry summed over the rows in ascending order), Cholesky A = L L^T, Sigma = A^-1 by two
 *                triangular solves per column; cov[21] is Sigma's upper triangle, row-major
 *   chi2         the sum of the eight r^2;  sigma_range = sqrt(d^T Sigma_tautau d), d = t / |t|
 *   yaw block    where the engine solves constrained poses and the record's irmv_yaw_pose.state == 1: the parameters are
 *                (psi, tau) at THAT pose, dX_i/dpsi = u x (R_yaw P_i) with the slot's up vector u; yaw_cov[10] is the upper
 *                triangle of the 4 x 4 inverse, sigma_yaw = sqrt(yaw_cov[0]) (radians)
 * A record is refused (state -1, everything else zero) where a corner has depth <= 0, an input is not finite (a coordinate
 * >= 2^24 counts, as for the solver), a pivot p has !(p > 0) or an output is not finite; yaw_state likewise for its block.
 * sigma_px is the only modelling parameter: a caller who prefers the a-posteriori scale multiplies cov by chi2 / 2 (yaw_cov by
 * yaw_chi2 / 4) itself.
 * Nothing is allocated and nothing new is launched until the first irmv_engine_set_pose_cov.  That call waits for everything
 * in flight, allocates the records and the option table and drops the captured graphs once; later calls rewrite the table the
 * kernel reads when it runs and re-capture nothing.  enable = 0: the kernel returns at once and irmv_engine_pose_covs delivers
 * all-zero records.  Explicit boxes have no such record.  Tiled steps: the record of merged record r is
 * irmv_engine_pose_covs(first + r.tile)[r.index].  Window slots: the crop only moves the principal point, so a window engine's
 * record equals a plain engine's on the cropped frame. */
typedef struct irmv_pose_cov_opts {
    uint32_t struct_size;        /* = sizeof(irmv_pose_cov_opts) */
    int32_t  enable;             /* 0 | 1 */
    double   sigma_px;           /* in (0, 64]; default 1 */
} irmv_pose_cov_opts;
typedef struct irmv_pose_cov {
    double  cov[21], chi2, sigma_range;          /* upper triangle of the 6 x 6, row-major; sum of r^2; metres along the ray */
    double  yaw_cov[10], yaw_chi2, sigma_yaw;    /* upper triangle of the 4 x 4 of (psi, tau); sum of r^2; radians */
    int32_t state, yaw_state;                    /* 0: nothing here (all zero); 1: computed; -1: refused */
} irmv_pose_cov;                                 /* 288 bytes */
/* IRMV_ERR_ARG before the GPU is touched, leaving everything as it was: a null engine or opts, a wrong struct_size, enable
 * outside {0, 1}, sigma_px outside (0, 64] or NaN. */
int irmv_engine_set_pose_cov(irmv_engine *e, const irmv_pose_cov_opts *opts);
int irmv_engine_get_pose_cov(const irmv_engine *e, irmv_pose_cov_opts *opts);   /* before the first set: the defaults with enable = 0 */
/* Parallel to irmv_engine_results, as irmv_engine_pose_alts is.  IRMV_ERR_ARG before the first irmv_engine_set_pose_cov. */
int irmv_engine_pose_covs(irmv_engine *e, int slot, irmv_pose_cov *out, int cap, int *n);

/* ---- armor tracks: frame-to-frame ids and a constant-velocity filter ---------------------------------------------------
 * Every record above belongs to one frame.  From the first irmv_engine_set_tracking on, an engine keeps ONE table of
 * IRMV_TRACK_CAP tracks in device memory and advances it behind every ordinary step, in a kernel of its own (k_track.hip), and a
 * slot delivers two more records: one irmv_det_track per detection (irmv_engine_det_tracks) and the table as that step left it
 * (irmv_engine_tracks).  irmv_det and every other record stay byte-identical whether or not it is on.  The arithmetic, fp64 in
 * the written order (no fused multiply-add; +, -, *, / and comparisons only); irmv_detection_amd/tracks.py states it operation
 * for operation:
 *   frame        the slot's stamp t (irmv_engine_set_stamp, seconds), its camera pose in the world (R_wc row-major, t_wc:
 *                irmv_engine_set_camera_pose) and the n = min(num_dets, max_det) records of the step
 *   eligible     pnp_ok == 1, armor_valid == 1, tvec finite with z > 0, and a measurement and noise that are finite (noise
 *                diagonal > 0)
 *   measurement  z = R_wc tvec + t_wc;  noise R = R_wc C R_wc^T with C the translation block (rows, columns 3 .. 5) of the
 *                record's irmv_pose_cov where that feature is enabled and its state is 1, else
 *                C = diag((sigma_lat z)^2, (sigma_lat z)^2, (sigma_rng z^2)^2) with z = tvec.z
 *   stamps       t not greater than the stamp of the last processed frame (or not finite): the frame is refused ON THE DEVICE --
 *                frame state -2, the table and its stamp untouched, the frame's detection records all zero
 *   1 predict    every live track to t: x = [p, v], p += dt v; P = F P F^T + Q, per axis Q = accel_sigma^2 [dt^4/4 dt^3/2; . dt^2]
 *   2 gate       for every live track and eligible record of the same class (match_class = 0: of any): y = z - p,
 *                S = P_pp + R, inverted by cofactors, d2 = y^T S^-1 y; kept where det S > 0 and 0 <= d2 <= gate
 *   3 assign     greedily: the least d2 left; ties to the lower track index, then the lower record index
 *   4 update     x += K y, P -= K H P with K = P H^T S^-1 (upper triangle, mirrored); hits++, misses = 0, last_hit = t;
 *                confirmed from confirm_hits hits on
 *   5 misses     every other live track: misses++; deleted (entry zeroed) when misses > max_misses or t - last_hit > max_coast_s
 *   6 births     every other eligible record, in index order: a tentative track in the lowest free entry with p = z, v = 0,
 *                P = blockdiag(R, init_vel_sigma^2 I) and the next id; no free entry: state -1 ("no room")
 * Ids start at 1 and are never reused in the life of the engine (of the stand-alone tracker).
 * `det` is a word of the snapshots: the table carries whatever the last launch left in it (a refused frame writes -1 into its
 * snapshot, and a launch that advances behind it writes that back) and nothing ever reads it from there.
 * Ordering (rule 7): tracks advance in SUBMIT order, and within a multi-slot submit in slot order, however
 * the steps' graphs overlap on their streams.  A slot's two track records are those of its last ordinary step and describe the
 * table as that step left it.  Stamp and camera pose are seen as of the submit.
 * Fed: every ordinary step (irmv_engine_detect, irmv_engine_submit of one or more slots), in the window and the frame view, of
 * every point source.  NOT fed: tiled steps, irmv_engine_run_post and the on-demand entries; they leave the table alone, and a
 * tiled step's and run_post's two channels read as zero for their slots.
 * Nothing is allocated and nothing new is launched until the first irmv_engine_set_tracking.  That call waits for everything in
 * flight; it re-captures NOTHING (the launch is no graph node: it follows the step's graph on the step's stream, chained to the
 * previous track launch by one event).  enable = 0 zeroes both channels and clears the table; the id counter goes on.
 * Sizes: irmv_track_opts 72, irmv_det_track 72, irmv_track_frame 40, irmv_track 384 bytes. */
#define IRMV_TRACK_CAP 32
#define IRMV_TRACK_FREE      0
#define IRMV_TRACK_TENTATIVE 1
#define IRMV_TRACK_CONFIRMED 2
typedef struct irmv_track_opts {
    uint32_t struct_size;        /* = sizeof(irmv_track_opts) */
    int32_t  enable;             /* 0 | 1 */
    int32_t  confirm_hits;       /* 1 .. 2^20; default 3 */
    int32_t  max_misses;         /* 1 .. 2^20; default 5 */
    int32_t  match_class;        /* 0 | 1; default 1 */
    int32_t  reserved;           /* 0 */
    double   gate;               /* default 16.27: the 0.999 quantile of chi-square with three degrees of freedom */
    double   max_coast_s;        /* default 0.5 */
    double   accel_sigma;        /* m/s^2; default 8 */
    double   init_vel_sigma;     /* m/s; default 3 */
    double   sigma_lat;          /* default 0.002 */
    double   sigma_rng;          /* default 0.01 */
} irmv_track_opts;               /* 72 bytes; every double finite and > 0 */
typedef struct irmv_det_track {
    int32_t  state;              /* 0: not eligible (all zero); 1: matched; 2: started a track; -1: no room */
    int32_t  track;              /* table index; -1: no room */
    uint32_t id;
    int32_t  hits;
    double   d2;                 /* matched: the gated distance */
    double   pos[3], vel[3];     /* filtered, world frame */
} irmv_det_track;                /* 72 bytes */
typedef struct irmv_track_frame {
    double   stamp;              /* the frame's stamp */
    int32_t  state;              /* 1: processed; -2: stamp refused; 0: tracking off / no ordinary step yet */
    int32_t  n_live, n_confirmed, n_started, n_deleted, n_no_room;
    uint32_t next_id;
    int32_t  reserved;
} irmv_track_frame;              /* 40 bytes */
typedef struct irmv_track {
    uint32_t id;                 /* from 1; 0: free entry (all zero but det) */
    int32_t  class_id;
    int32_t  state;              /* IRMV_TRACK_* */
    int32_t  hits, misses;
    int32_t  det;                /* snapshots: the frame's record matched to (or starting) the track; -1: none */
    double   first_stamp, last_hit, stamp;   /* stamp: the time x and P are valid at */
    double   x[6];               /* p, v in the world frame */
    double   P[36];              /* row-major, exactly symmetric */
} irmv_track;                    /* 384 bytes */
/* IRMV_ERR_ARG before the GPU is touched, leaving everything as it was (the values first): null opts, a wrong struct_size,
 * enable or match_class outside {0, 1}, confirm_hits or max_misses outside 1 .. 2^20, reserved != 0, a double that is not
 * finite and positive; then a null engine. */
int irmv_engine_set_tracking(irmv_engine *e, const irmv_track_opts *opts);
/* Host only: the defaults above with struct_size filled in and enable = 0 -- the one place the values are written down for
 * the facades. */
int irmv_track_default_opts(irmv_track_opts *opts);
int irmv_engine_get_tracking(const irmv_engine *e, irmv_track_opts *opts);   /* before the first set: the defaults with enable = 0 */
/* The slot's stamp (default 0) and camera pose (default identity, zero): live per-slot state as irmv_engine_set_up is -- the
 * call waits for the slot's last step, then writes the slot's entry of a device table; works before the first
 * irmv_engine_set_tracking.  IRMV_ERR_ARG: a slot out of range, a value that is not finite. */
int irmv_engine_set_stamp(irmv_engine *e, int slot, double t);
int irmv_engine_get_stamp(const irmv_engine *e, int slot, double *t);
int irmv_engine_set_camera_pose(irmv_engine *e, int slot, const double R_wc[9], const double t_wc[3]);
int irmv_engine_get_camera_pose(const irmv_engine *e, int slot, double R_wc[9], double t_wc[3]);
/* Parallel to irmv_engine_results, as irmv_engine_pose_covs is.  IRMV_ERR_ARG before the first irmv_engine_set_tracking. */
int irmv_engine_det_tracks(irmv_engine *e, int slot, irmv_det_track *out, int cap, int *n);
/* The slot's frame header and the first min(cap, IRMV_TRACK_CAP) entries of its snapshot (free entries included); *n = that
 * number.  frame or out may be NULL (out with cap = 0).  IRMV_ERR_ARG before the first irmv_engine_set_tracking. */
int irmv_engine_tracks(irmv_engine *e, int slot, irmv_track_frame *frame, irmv_track *out, int cap, int *n);
/* Waits for everything in flight, then clears the table and its stamp; the id counter goes on, the slots' records stay. */
int irmv_engine_reset_tracks(irmv_engine *e);
/* out[0] = IRMV_TRACK_CAP, [1] = sizeof(irmv_track), [2] = sizeof(irmv_det_track), [3] = sizeof(irmv_track_frame),
 * [4] = sizeof(irmv_track_opts), [5] = the most observations of one irmv_tracker_update, [6], [7] = 0 */
int irmv_track_limits(int32_t out[8]);
/* Host only, the bits of tracks.py predict_position: a live track's position and its 3 x 3 covariance (row-major) at stamp
 * t >= track->stamp under white acceleration accel_sigma (the filter's own prediction step).  IRMV_ERR_ARG: a null argument, a
 * free track, t before the track's stamp or not finite, accel_sigma not finite and positive. */
int irmv_track_predict(const irmv_track *track, double t, double accel_sigma, double pos[3], double cov[9]);

/* The same tracker stand-alone on explicit observations, as irmv_pnp offers the pose kernels: one table per object. */
typedef struct irmv_tracker irmv_tracker;
typedef struct irmv_track_obs {
    int32_t class_id;
    int32_t valid;               /* 1: what pnp_ok == 1 and armor_valid == 1 say of a record */
    int32_t has_cov;             /* 1: cov is the noise C in the camera frame; 0: the default from sigma_lat / sigma_rng */
    int32_t reserved;
    double  tvec[3];
    double  cov[9];              /* row-major 3 x 3 */
} irmv_track_obs;                /* 112 bytes */
int irmv_tracker_create(int device, const irmv_track_opts *opts, irmv_tracker **out);   /* opts NULL: the defaults, enabled */
void irmv_tracker_destroy(irmv_tracker *tr);
/* One frame of n <= 256 observations at stamp t under the camera pose (NULL: identity / zero): det_out [n], *frame, tracks_out
 * [IRMV_TRACK_CAP]; each may be NULL.  A refused stamp is a result (frame->state == -2), not an error. */
int irmv_tracker_update(irmv_tracker *tr, double t, const double R_wc[9], const double t_wc[3], const irmv_track_obs *obs, int n,
                        irmv_det_track *det_out, irmv_track_frame *frame, irmv_track *tracks_out);
int irmv_tracker_reset(irmv_tracker *tr);   /* the table and its stamp; the id counter goes on */

/* ---- plate patches: each armor's rectified number image ---------------------------------------------------------------
 * A consumer of such a detector cuts the number plate out of the frame between the two light bars, rectifies it with the
 * four points and hands the small gray image to a number classifier.  From the first irmv_engine_set_patches on, a step does
 * that for every record with armor_valid == 1 in a kernel of its own behind the NMS (behind the light extraction on classical
 * and refined engines), on the slot's frame at the sensor's resolution, and delivers one side record per detection
 * (irmv_engine_plate_patches): the patch, its Otsu threshold and a colour vote of its two light bars.  irmv_det,
 * irmv_pose_alt, irmv_yaw_pose and irmv_tile_det stay byte-identical whether or not it is on.
 * irmv_detection_amd/patches.py states the model operation for operation; fp64 in the written order (no fused
 * multiply-add), divisions are divisions.
 *   Layout.  The patch is IRMV_PATCH_W = 20 columns by IRMV_PATCH_H = 28 rows.  A rectified image of `span` columns has the
 *     light bars' centre lines in columns 0 and span - 1 (span[IRMV_ARMOR_SMALL] = 32, span[IRMV_ARMOR_LARGE] = 54), the
 *     bars' top ends in row `top` = 7 and their bottom ends in row top + light_rows = 19.  The patch is that image's middle
 *     20 columns: with off = (span - 20) / 2, patch pixel (i, j) -- column i, row j -- has plate coordinates
 *     s = (i + off) / (span - 1), t = (j - top) / light_rows; t runs past [0, 1] on purpose.
 *   Mapping (Heckbert's square-to-quad).  The record's eight float keypoints (LB, LT, RT, RB) widened to double;
 *     p0 = LT, p1 = RT, p2 = RB, p3 = LB:
 *       dx1 = x1 - x2   dx2 = x3 - x2   sx = ((x0 - x1) + x2) - x3        (the same for y)
 *       den = dx1 dy2 - dx2 dy1
 *       g = (sx dy2 - dx2 sy) / den        h = (dx1 sy - sx dy1) / den
 *       a = (x1 - x0) + g x1   b = (x3 - x0) + h x3   c = x0
 *       d = (y1 - y0) + g y1   e = (y3 - y0) + h y3   f = y0
 *       w = (g s + h t) + 1     x = ((a s + b t) + c) / w     y = ((d s + e t) + f) / w
 *     (x, y) is in the pixels of the frame the slot's step saw, in the coordinates its results come in (W x H): with
 *     rotate180 the one irmv_engine_rotated_image returns -- the rotation is folded into the fetch --, without it the slot's
 *     frame as it lies in the buffer.  The records' keypoints are in that frame already; a window slot's result keypoints
 *     are those plus the window's corner.
 *   Sampling (integers).  A sample for which 0 <= x <= W - 1 && 0 <= y <= H - 1 is false (NaN fails it) counts in n_outside.
 *     One for which -1 <= x <= W && -1 <= y <= H is false has value 0.  Every other one: X = floor(32 x + 0.5), ix = X >> 5,
 *     fx = X & 31, likewise y; texel gray (p0 3735 + p1 19235 + p2 9798 + 2^14) >> 15 (the light extraction's), 0 outside
 *     the frame; v = (g00 (32 - fx)(32 - fy) + g10 fx (32 - fy) + g01 (32 - fx) fy + g11 fx fy + 512) >> 10.
 *   Otsu.  N = 560, S = sum v; for k in 0 .. 255: w0 = #(v <= k), w1 = N - w0, m0 = sum(v <= k), A = m0 N - S w0,
 *     q_k = (double)(A A) / (double)(w0 w1) where w0 > 0 && w1 > 0, else -1.  otsu is the smallest k of maximal q; a patch of
 *     one gray level reports that level.
 *   Bar colour vote.  The 2 x (light_rows + 1) points s in {0, 1}, t = r / light_rows; the nearest texel
 *     ((X + 16) >> 5, (Y + 16) >> 5) under the second guard above; bar_sum[0] sums channel 0, bar_sum[1] channel 2 of the
 *     texels inside the frame.
 *   No patch (state 0, the record all zero): armor_valid != 1, a non-finite keypoint, den == 0 or a non-finite coefficient,
 *     !(w > 0) at any of the 560 samples.  Otherwise state 1.
 * Nothing is allocated and nothing new is launched until the first irmv_engine_set_patches.  That call waits for everything
 * in flight, allocates the records and the option table and drops the captured graphs once; later calls rewrite the table
 * the kernel reads when it runs and re-capture nothing.  enable = 0: the kernel returns at once, and the call zeroes the
 * records.  The kernel reads the slot's frame where and when the light extraction of a refined engine reads it: the frame the
 * step was submitted with, under every upload path.  Tiled steps: the patch of merged record r is
 * irmv_engine_plate_patches(first + r.tile)[r.index]. */
#define IRMV_PATCH_W 20
#define IRMV_PATCH_H 28
typedef struct irmv_patch_opts {
    uint32_t struct_size;        /* = sizeof(irmv_patch_opts) */
    int32_t  enable;             /* 0 | 1 */
    int32_t  span[2];            /* per plate size: 20 .. 128, span - 20 even; default 32, 54 */
    int32_t  light_rows;         /* 1 .. 28; default 12 */
    int32_t  top;                /* 0 .. 27; default 7 */
    int32_t  reserved[2];        /* 0 */
} irmv_patch_opts;
typedef struct irmv_plate_patch {
    uint8_t  gray[IRMV_PATCH_H][IRMV_PATCH_W];
    int32_t  state, otsu, n_outside, armor_size;   /* armor_size: the record's, whose span the patch used */
    uint32_t bar_sum[2], sum;                       /* sum: S, the 560 values' */
    int32_t  reserved;
} irmv_plate_patch;   /* 592 bytes */
/* IRMV_ERR_ARG before the engine is looked at, leaving everything as it was: null opts, a wrong struct_size, enable outside
 * {0, 1}, a value outside its range above, reserved != 0.  Then: a null engine. */
int irmv_engine_set_patches(irmv_engine *e, const irmv_patch_opts *opts);
int irmv_engine_get_patches(const irmv_engine *e, irmv_patch_opts *opts);   /* before the first set: the defaults with enable = 0 */
/* Parallel to irmv_engine_results, as irmv_engine_yaw_poses is.  IRMV_ERR_ARG before the first irmv_engine_set_patches. */
int irmv_engine_plate_patches(irmv_engine *e, int slot, irmv_plate_patch *out, int cap, int *n);
/* On demand, on any engine, enabled or not: the patches of n explicit quads (kpts [n][8] in result coordinates, LB LT RT RB;
 * armor_size [n], IRMV_ARMOR_SMALL / _LARGE) on the slot's current frame in its current view, as irmv_engine_refine_points
 * acts, under the engine's present options (enable is not read): out [n], 0 <= n <= IRMV_MAX_DET_CAP.  Every quad is taken as
 * an armor (state is 0 only for the geometric reasons above).  Waits for the engine's steps in flight. */
int irmv_engine_patches_at(irmv_engine *e, int slot, const float *kpts, const int32_t *armor_size, int n, irmv_plate_patch *out);
/* out: IRMV_PATCH_W, IRMV_PATCH_H, span min, span max, light_rows max, top max, sizeof(irmv_plate_patch), 0 */
int irmv_patch_limits(int32_t out[8]);

/* ---- plate numbers: each plate patch read by a small MLP ----------------------------------------------------------------
 * The classic second opinion of an armor detector: a small multi-layer perceptron on the 560 values of the plate patch above,
 * giving a label and the logits a confidence follows from.  From the first irmv_engine_set_numbers on, a step runs it in a
 * kernel of its own directly behind the patch kernel, on the patch records where that kernel wrote them, and delivers one side
 * record per detection (irmv_engine_plate_numbers).  irmv_det, irmv_pose_alt, irmv_yaw_pose, irmv_plate_patch and irmv_tile_det
 * stay byte-identical whether or not it is on.  irmv_detection_amd/number_net.py (NumberModel.reference) states the model
 * operation for operation; the results are equal in bytes.
 *   Network.  n_layers = 1 .. 3 dense layers of widths dims[0] = 560 -> dims[1] -> .. -> dims[n_layers]: hidden widths
 *     1 .. 128, the last width C = 1 .. 16.  The input is the patch in row-major order, k = j * 20 + i for column i, row j.
 *     ReLU, r = a > 0 ? a : +0, behind every layer but the last.  No softmax on the device.
 *   Weights.  fp32, row-major [out][in] (a torch.nn.Linear weight, an ONNX Gemm with transB = 1), biases fp32 [out].  At set
 *     time every weight is rounded to fp16 (nearest even) and kept as fp16; biases stay fp32.  A non-finite weight or bias, or
 *     one of magnitude above 65504, is refused.  With that bound no logit can overflow --
 *     560 * 65504 * 128 * 65504 * 128 * 65504 ~ 2.6e21 < 3.4e38 --: logits are always finite.
 *   Input.  IRMV_NUM_IN_BINARY: x_k = gray_k > otsu ? 1.0f : 0.0f with the patch record's own otsu (Otsu binarisation and a
 *     scale by 1/255).  IRMV_NUM_IN_GRAY: x_k = (float)gray_k / 255.0f, one correctly rounded fp32 division.
 *   Arithmetic.  fp32, no fused multiply-add, denormals kept: every product w * x is rounded, then every sum.  The summation
 *     order is part of the model: a unit has FOUR chains, chain q takes the inputs k = q (mod 4) in ascending k,
 *       a_0 = bias, a_1 = a_2 = a_3 = +0;   a_q = a_q + (float)w[k] * x_k   for k = q, q + 4, q + 8, ...
 *       a = (a_0 + a_1) + (a_2 + a_3)
 *     (the same for every layer: k runs over the layer's inputs, x is the previous layer's ReLU output).
 *   Result.  label: the index of the largest logit, ties to the smaller index.  second: the same among the others, -1 where
 *     C = 1.  margin = logit[label] - logit[second] in fp32, 0 where C = 1.  ones: the number of inputs equal to 1 (binary),
 *     the integer sum of the 560 gray values (gray).  logits behind C are +0.  state 1: classified.  state 0, "no answer": all
 *     96 bytes zero, exactly where the patch record has state == 0.
 * Nothing is allocated and nothing new is launched until the first call below.  irmv_engine_set_number_model checks everything
 * first, waits for the engine and uploads the rounded weights to device ranges sized for the largest model, whose addresses
 * never move: a later model is live for the next step and re-captures nothing.  The first irmv_engine_set_numbers allocates
 * the records, appends the kernel to the steps and drops the captured graphs once; later calls rewrite the table the kernel
 * reads when it runs.  enable = 1 without a model: IRMV_ERR_ARG.  enable = 1 on an engine whose patches were never set turns
 * them on in the same call, with the patch defaults and enable = 1.  enable = 0: the kernel returns at once, and the call
 * zeroes the records.  Patches disabled while numbers stay enabled: the patch records are zero and every number record is "no
 * answer".  Tiled steps: the number of merged record r is irmv_engine_plate_numbers(first + r.tile)[r.index]. */
#define IRMV_NUM_IN_BINARY 0
#define IRMV_NUM_IN_GRAY 1
#define IRMV_NUM_CLASSES_MAX 16
typedef struct irmv_number_model {
    uint32_t struct_size;        /* = sizeof(irmv_number_model) */
    int32_t  n_layers;           /* 1 .. 3 */
    int32_t  dims[4];            /* dims[0] = 560, hidden 1 .. 128, dims[n_layers] = C = 1 .. 16; the rest 0 */
    int32_t  input;              /* IRMV_NUM_IN_* */
    const float *weight[3];      /* layer l: [dims[l + 1]][dims[l]] */
    const float *bias[3];        /* layer l: [dims[l + 1]] */
} irmv_number_model;
typedef struct irmv_number_opts {
    uint32_t struct_size;        /* = sizeof(irmv_number_opts) */
    int32_t  enable;             /* 0 | 1 */
    int32_t  reserved[3];        /* 0 */
} irmv_number_opts;
typedef struct irmv_plate_number {
    int32_t  state, label, second, ones;
    float    margin;
    int32_t  reserved[3];
    float    logits[IRMV_NUM_CLASSES_MAX];
} irmv_plate_number;   /* 96 bytes */
/* IRMV_ERR_ARG before the engine is looked at, leaving everything as it was: a null model, a wrong struct_size, n_layers,
 * dims or input outside the ranges above, a null weight or bias of a layer in use, a value refused above.  Then: a null engine. */
int irmv_engine_set_number_model(irmv_engine *e, const irmv_number_model *model);
/* A model file (.irmn; NumberModel.save writes one), little endian: "IRMN", uint32 version = 1, int32 n_layers, int32 dims[4],
 * int32 input -- 32 bytes --, then per layer its fp32 weights [out][in] and its fp32 biases [out].  Every length is checked
 * against the file's size before it is used; the file must end where the last bias does.  irmv_number_model_read fills
 * *model with pointers into buf (buf_floats floats; *need_floats, if not null: how many the file's model takes, at most
 * 90384); the values themselves are checked by irmv_engine_set_number_model. */
int irmv_number_model_read(const char *path, irmv_number_model *model, float *buf, int64_t buf_floats, int64_t *need_floats);
int irmv_engine_load_number_model(irmv_engine *e, const char *path);
/* IRMV_ERR_ARG before the engine is looked at: null opts, a wrong struct_size, enable outside {0, 1}, reserved != 0.  enable = 0
 * on an engine that never enabled them changes nothing and makes nothing. */
int irmv_engine_set_numbers(irmv_engine *e, const irmv_number_opts *opts);
int irmv_engine_get_numbers(const irmv_engine *e, irmv_number_opts *opts);   /* before the first set: enable = 0 */
/* Parallel to irmv_engine_results, as irmv_engine_plate_patches is.  IRMV_ERR_ARG before the first irmv_engine_set_numbers
 * with enable = 1. */
int irmv_engine_plate_numbers(irmv_engine *e, int slot, irmv_plate_number *out, int cap, int *n);
/* On demand, on any engine that has a model, enabled or not: the numbers of n explicit patch records, out [n],
 * 0 <= n <= IRMV_MAX_DET_CAP.  Reads no frame and no slot.  A patch whose state is not 0 or 1, or whose otsu is outside
 * 0 .. 255, is refused.  Waits for the engine's steps in flight. */
int irmv_engine_numbers_at(irmv_engine *e, const irmv_plate_patch *patches, int n, irmv_plate_number *out);
/* out: 560, hidden max, C max, layers max, sizeof(irmv_plate_number), weight halves kept on the device, 65504, 0 */
int irmv_number_limits(int32_t out[8]);
/* Host only: the softmax of the record's first C logits, computed in double (exp(l - max) / sum), out[C .. 15] = 0.  A "no
 * answer" record gives all zero.  (A device exp would end the byte parity of the records.) */
int irmv_number_softmax(const irmv_plate_number *rec, int C, float out[16]);

/* ---- stage-wise read-backs used by the parity tests -------------------- */
int irmv_engine_read_input(irmv_engine *e, int slot, float *chw);             /* [3][net_h][net_w], as the reference's input_buffer_ */
int irmv_engine_read_head(irmv_engine *e, int slot, float *head);             /* [A][64+nc+nk], A = irmv_engine_num_anchors(): levels
                                                                                 s = 8, 16, 32 in turn, each (net_h/s) x (net_w/s) row-major */
int irmv_engine_write_head(irmv_engine *e, int slot, const float *head);      /* inject a head tensor ... */
int irmv_engine_run_post(irmv_engine *e, int first_slot, int count);          /* ... and run decode->NMS->PnP only */
/* fault injection for the robustness test: overwrite every slot's candidate counter (the one piece of state a step leaves for
 * the next kernel of the same step) with `value`.  The next step must stay inside its buffers and reset the counter; the
 * step after it must be correct again.  IRMV_ERR_ARG for an engine that keeps no counters (IRMV_SPLIT_SCAN=0). */
int irmv_engine_debug_poke_candidate_counts(irmv_engine *e, int value);
/* Read-only (tests): the slot's candidate-anchor bitmap of the sparse head, one bit per anchor, ceil(num_anchors / 32) words
   (all zero between steps).  *sparse = 1 if this engine's steps store candidate head rows only (IRMV_SPARSE_HEAD=0, or a
   configuration without candidate emission: 0, and no words are kept: *n = 0).  words may be NULL to query *n. */
int irmv_engine_debug_read_cand_bits(irmv_engine *e, int slot, uint32_t *words, int cap, int *n, int *sparse);
/* Its counterpart (tests/test_gpu_gather_craft.py): waits, then copies n words over the slot's bitmap.  IRMV_ERR_ARG on an
   engine without a sparse head, for n other than the engine's word count, and for any set bit at or past num_anchors.  A
   step expects the bitmap all zero: write zeros back before the next one. */
int irmv_engine_debug_write_cand_bits(irmv_engine *e, int slot, const uint32_t *words, int n);
/* The candidate lists of Detect level `level` (0 .. 2, one with a boxg op) on slots [first, first + count), as
   cand_list_kernel leaves them: counts[count], and entries[count][H * W] of which image i's first counts[i] are its list
   (pixel = y * W + x).  Waits, then copies; irmv_engine_run_op with IRMV_RUN_WRITTEN_LISTS gathers from them.
   IRMV_ERR_ARG for a count outside [0, H * W] or ANY entry outside [0, H * W).  Reading: the ranges "boxg_list" (level l,
   slot s at int index lvl_base[l] * num_slots + s * H * W) and "boxg_count" ([3][num_slots]) of irmv_engine_debug_allocs,
   through irmv_engine_debug_read_mem. */
int irmv_engine_debug_write_cand_lists(irmv_engine *e, int level, int first_slot, int count, const int32_t *counts, const int32_t *entries);
/* Read-only (tests): the slot's head records as they lie in memory, with NO read-back step in front (read_head, read_tap and
   read_tensor first bring a sparse head to the dense state): [num_anchors][96] floats, box 64 | classes at 64 | keypoints at
   80; `bytes` must be num_anchors * 96 * 4.  After a step of a sparse engine only the rows the step stored are the step's. */
int irmv_engine_debug_read_head_rows(irmv_engine *e, int slot, float *rec, size_t bytes);
/* Read-only (tests): irmv_engine_read_head without the read-back step: [num_anchors][64 + nc + nk] floats as the last step or
   write_head left them.  Runs no kernel and does not change what a later read_head does.  The same memory as
   irmv_engine_debug_read_head_rows shows; the two differ in layout only (read_head's columns here, the 96-float records there). */
int irmv_engine_debug_read_head_raw(irmv_engine *e, int slot, float *head);
int irmv_engine_read_tap(irmv_engine *e, int slot, const char *name, float *nhwc, int shape[3]);   /* shape = {H, W, C}: a tensor of
                                                                                 level s is (net_h/s) x (net_w/s) */
int irmv_engine_read_raw(irmv_engine *e, int slot, irmv_raw_dets *out);
int irmv_engine_num_anchors(const irmv_engine *e);
int irmv_engine_head_channels(const irmv_engine *e);
/* The network input of this engine: *width = net_size, *height = net_height (net_size for a square engine). */
int irmv_engine_net_dims(const irmv_engine *e, int *width, int *height);

/* ---- per-layer conv test hooks (tests/test_gpu_conv_candidates.py) ------
 * Every conv layer of the engine, every tile candidate its autotuner timed, run one at a time on a slot range. */
typedef struct irmv_conv_seg {
    char tensor[32];            /* irmv_engine_read_tap name; "" = none */
    int32_t coff, C, shift;     /* channel offset and count in that tensor; shift 1: read as its nearest 2x upsample */
} irmv_conv_seg;

typedef struct irmv_conv_op {
    int32_t op;                 /* the engine's op index: the `op` argument of the calls below */
    char layer[32];             /* weight layer, as the blob names it */
    int32_t ks, stride, act, out_f32, cin, cout, cout_pad;
    int32_t Hin, Win, Hout, Wout;   /* rows x columns at the conv's input and output: (net_h/s) x (net_w/s) at stride s */
    irmv_conv_seg s0, s1;       /* input = concat(s0, s1) along channels */
    irmv_conv_seg res;          /* residual added after the activation (C = cout); tensor "" = none */
    char out_tensor[32];        /* output channels [out_coff, out_coff + cout_pad) of this tensor */
    int32_t out_coff;
    int32_t out_lazy;           /* a step does not write out_tensor (a fused kernel keeps it on chip) */
    int32_t fused;              /* a step runs this conv with its branch's final 1x1 in the epilogue ... */
    int32_t tune_fused;         /* ... and the autotuner listed candidates for that epilogue */
    char fuse_layer[32];        /* that 1x1: its layer, output tensor, channel offset and cout (fused or tune_fused) */
    char fuse_tensor[32];
    int32_t fuse_coff, fuse_cout, fuse_cout_pad;
    int32_t reserved;
    char kname[48], kname_one[48];   /* the tiles chosen for the stream share and for one slot */
} irmv_conv_op;

typedef struct irmv_conv_cand {
    char name[48];              /* kernel name, as irmv_engine_profile names it */
    int32_t mt, nt, flags, ipw; /* the tile as the tune cache stores it */
    int32_t forced, reserved;   /* forced: an IRMV_FORCE_* switch put the layer on it */
} irmv_conv_cand;

#define IRMV_DECLINED 1         /* irmv_engine_run_conv_candidate: no kernel instantiation runs that candidate */

/* One record per conv op, in step order; *n = their number (records beyond cap are not written). */
int irmv_engine_conv_ops(irmv_engine *e, irmv_conv_op *ops, int cap, int *n);
/* The candidate list the autotuner timed for conv op `op` at tune_count (the stream share of num_slots, or 1). */
int irmv_engine_conv_candidates(irmv_engine *e, int op, int tune_count, irmv_conv_cand *cands, int cap, int *n);
#define IRMV_RUN_POISON 1u       /* first fill the output channels the run must write (cout of them; for a run that carries
                                     the fused 1x1, that 1x1's head slice) on its slots with all-ones bytes, a NaN */
#define IRMV_RUN_POISON_ONLY 2u  /* ... and launch nothing (shows that a run which writes nothing is seen) */
/* Run candidate `cand` of that list (-1: the engine's own choice for tune_count) on slots [first, first + count) and
 * synchronize.  IRMV_DECLINED if no kernel runs it; IRMV_ERR_ARG for an op whose output overlaps one of its inputs. */
int irmv_engine_run_conv_candidate(irmv_engine *e, int op, int tune_count, int cand, int first_slot, int count, uint32_t flags);
/* The raw storage (fp16 bits at the activation scale, or fp32) of a tensor's slots [first, first + count); bytes must
 * equal its size.  Unlike irmv_engine_read_tap it never recomputes a tensor a step keeps on chip. */
int irmv_engine_read_tensor(irmv_engine *e, const char *name, int first_slot, int count, void *dst, size_t bytes);
/* The mirror of irmv_engine_read_tensor (tests/test_gpu_act_craft.py): copy raw storage (fp16 bits at the activation scale, or
 * fp32) over a tensor's slots [first, first + count); bytes must equal their size (IRMV_ERR_ARG otherwise).  It waits for the
 * engine and first brings the slots to the dense state a read-back leaves (the head rows a sparse step did not store, the
 * gated box branches); the slots stay marked as not stale, so a later irmv_engine_read_tensor, read_head or run_post never
 * recomputes over what was written.  irmv_engine_read_tap and irmv_engine_read_input of a tensor a step keeps on chip STILL
 * recompute it (and every other such tensor of the slot) from the slot's frame: read what was written with
 * irmv_engine_read_tensor only. */
int irmv_engine_write_tensor(irmv_engine *e, const char *name, int first_slot, int count, const void *src, size_t bytes);

/* ---- per-op test hooks (tests/test_gpu_graph_ops.py) ------------------------
 * Every op of the engine's graph, of any kind; the non-conv layer ops run one at a time on a slot range. */
typedef struct irmv_graph_op {
    int32_t op;                 /* the engine's op index (the `op` of irmv_engine_run_op and of the conv hooks above) */
    char kind[16];              /* conv conv0 pool dw shuffle front c2f2 c2f32 bneck kpt3 boxg pre demosaic crop scan nms light meter */
    char layer[48];             /* weight layer, or the op's own name (model.9.m, model.N.shuffle, preprocess, ...) */
    char kname[48];             /* kernel, as irmv_engine_profile names it */
    irmv_conv_seg s0, s1;       /* inputs (tensor "" = none; the pool's: channels [0, C) of its own tensor) */
    char out_tensor[32];        /* the op writes channels [out_coff, out_coff + out_C) of this tensor; "" = no activation tensor */
    int32_t out_coff, out_C;
    int32_t fused_away;         /* a step runs a fused kernel in its place (read-backs still run it) */
    int32_t reserved;
} irmv_graph_op;

/* One record per op of the graph, in step order; *n = their number (records beyond cap are not written). */
int irmv_engine_ops(irmv_engine *e, irmv_graph_op *ops, int cap, int *n);
/* Run the engine's own kernel of a conv0, pool, dw or shuffle op, or of a fused c2f2, c2f32, bneck, kpt3 or boxg op, on slots
 * [first, first + count), as a step of that count launches it, and synchronize.  A fused op runs as a plain launch: kpt3
 * without the sparse head's gate, every head row written.  flags: IRMV_RUN_POISON / IRMV_RUN_POISON_ONLY over the op's
 * output channels on those slots (the pool: channels [C, 4C) of its tensor; [0, C) is its input; a fused op: every range
 * irmv_engine_op_io lists as written).  IRMV_ERR_ARG for any other kind, and for a flag below on an op that is no boxg op.
 *
 * A boxg op (the candidate gather of a Detect level, on an engine with the sparse head): cand_list_kernel turns the
 * candidate bitmap of the slots (irmv_engine_debug_write_cand_bits) into every level's lists, then the level's gather
 * stores the box channels of the head rows at its candidate anchors -- and the keypoint channels (the final's padding
 * included) where a batched step's launch of the op carries the level's keypoint branch.  count: 1 .. num_slots, whatever
 * the step plans launch.  The poison flags cover the box channels of EVERY row of the range, and the keypoint channels
 * when that branch rides. */
#define IRMV_RUN_BOX_ONLY 4u        /* boxg: the box-only instantiation also where the keypoint branch would ride */
#define IRMV_RUN_WRITTEN_LISTS 8u   /* boxg: no cand_list_kernel; the gather runs on what irmv_engine_debug_write_cand_lists wrote */
#define IRMV_RUN_GRID(n) ((uint32_t)(n) << 16)   /* boxg: n = 1 .. 65535 persistent workgroups; 0: the engine's own grid (one per CU) */
int irmv_engine_run_op(irmv_engine *e, int op, int first_slot, int count, uint32_t flags);
/* What a fused op (c2f2, c2f32, bneck, kpt3, boxg) stands for: the conv ops whose layers it computes, in the order a step
 * without it runs them, every channel range its launch writes, and every channel range it reads (a residual included; a
 * segment with shift 1 is read as its nearest 2x upsample).  Nothing else of any activation tensor reaches its output.  No conv
 * or fused kernel reads channels beyond a segment's C: K positions past Cin are clamped onto the segment's own last channels.
 * boxg: sub = the three box convs; writes = the head's box channels, then the keypoint final's cout_pad channels where the
 * branch rides (its three convs: the sub-ops of the level's kpt3 op); it writes them at the candidate anchors only.
 * IRMV_ERR_ARG for an op of any other kind. */
typedef struct irmv_op_io {
    int32_t op;
    int32_t n_sub, sub[4];      /* engine op indices of its conv ops (records of irmv_engine_conv_ops) */
    int32_t n_writes, n_reads;
    irmv_conv_seg writes[2], reads[2];
    int32_t reserved;
} irmv_op_io;
int irmv_engine_op_io(irmv_engine *e, int op, irmv_op_io *io);
/* ---- light-extraction test hook (tests/test_gpu_light_shapes.py) ----------------
 * What light_extract_kernel saw in one box, stage by stage. */
#define IRMV_LIGHT_MAX_CONTOURS 1024   /* contours per box; more: armor_valid = -1 */
#define IRMV_LIGHT_POINTS_CAP 4096     /* contour points per box; more: armor_valid = -1 */
typedef struct irmv_light_rec {
    float corners[8];           /* the minimum-area rectangle's four corners, box coordinates, before Light sorts them by y */
    float top[2], bottom[2], center[2];   /* frame coordinates when ok, box coordinates otherwise */
    double length;
    int32_t measured;           /* 0: the contour has fewer than 5 points (or the box got no answer): nothing else is set */
    int32_t ok;                 /* passed is_light() */
    int32_t hull_edges;         /* edges of the convex hull; 0: one or two distinct points, or all collinear */
    int32_t in_lds;             /* measured in LDS (up to lds_points points) or in global memory */
} irmv_light_rec;
typedef struct irmv_light_trace {
    int32_t n_contours;         /* contours kept, at most max_contours */
    int32_t n_found;            /* as the scan counted them; max_contours + 1 = more than that */
    int32_t n_points;           /* points of the kept contours, counted past points_cap */
    int32_t too_large;          /* 1: the box gets armor_valid = -1 */
    int32_t pool_fit, in_lds;   /* the label image got its slice of the pool; it lived in LDS */
    int32_t rx, ry, rw, rh;     /* the box as the kernel cut it out of the frame */
    int32_t max_contours, points_cap, lds_image, lds_points;   /* the kernel's limits: contours, points, LDS label image bytes, LDS contour points */
    uint64_t label_pool, pool_offset;   /* bytes of the pool; bytes handed to the boxes before this one */
    int32_t starts[IRMV_LIGHT_MAX_CONTOURS + 1];   /* contour i: points [starts[i], starts[i + 1]), discovery order */
    int16_t points[IRMV_LIGHT_POINTS_CAP][2];      /* (x, y) in box coordinates, as the border following emitted them */
    int32_t reserved;
    irmv_light_rec recs[IRMV_LIGHT_MAX_CONTOURS];  /* per contour, discovery order */
} irmv_light_trace;
/* irmv_engine_extract_armors with a record of the kernel's stages: the same launch on the same scratch, plus trace[n].
 * out receives exactly what irmv_engine_extract_armors gives. */
int irmv_engine_light_trace(irmv_engine *e, int slot, const float *xyxy, int n, irmv_light_trace *trace, irmv_det *out);
/* The guided extraction on n explicit boxes (xyxy) and their keypoints (kpts[n][8]: LB, LT, RT, RB) on the slot's current
 * frame, on an engine of any point source; coordinates, window and view as irmv_engine_extract_armors.  out[i]: kpts, the
 * pose (plate cfg.armor_size), n_lights and reserved = the flag; where the flag is not 1, kpts are the inputs and the pose is
 * theirs.  trace: NULL, or trace[n] as irmv_engine_light_trace fills it (rx..rh: the guided ROI). */
int irmv_engine_refine_points(irmv_engine *e, int slot, const float *xyxy, const float *kpts, int n, irmv_light_trace *trace, irmv_det *out);
/* Host only: out = {max_contours, points_cap, lds_image, lds_points} without an engine. */
int irmv_light_limits(int32_t out[4]);
/* Host only: the candidate counts at which the post stage (decode + NMS, k_post.hip) changes its code path, and the tile
 * merge's capacities, as the library is compiled.  out = {rank_use (rank sort / class-walk / full suppression matrix up to
 * here, bitonic sort above), rank_max (the prefilter's compaction buffer), lazy_n (lazy suppression matrix up to here),
 * sup_cap (precomputed block masks), cand_cap (LDS sort up to here, exact radix select above), pre_hi, pre_lo (the
 * prefilter's window: it runs above pre_hi candidates), max_tiles, max_det_cap (tile merge: tiles, records per tile),
 * scan_blocks, scan_step, scan_lds_max (scan_decode_kernel: workgroups per frame, quads per round, LDS bytes that bound
 * a workgroup's range), inscan_chunk (quads per round of the scan inside nms_pnp_kernel), mat_n (rows of the full
 * suppression matrix), 0, 0}.  The count ladders of tests/post_ladder.py are computed from it. */
int irmv_post_limits(int32_t out[16]);

/* ---- the front's plan (tests/test_input_geometry.py) -----------------------------------------------------------------
 * Host only: every geometry decision between a source frame and model.1's output that irmv_engine_create derives from the
 * configuration -- the letterbox box, whether the fused front kernel (front_fused) runs and on which of its paths.  It is
 * the function the engine itself builds from -- box, fastx, tile_y, the tile counts, stage_bytes, fx_i0 / fx_step and
 * upload_kernel are the values the engine launches with; the engine's environment switches (IRMV_FUSED_FRONT, IRMV_FRONT_*)
 * come on top.  pair_cases and the four tile class counts are NOT consumed by the engine: they restate on the host what
 * front_kernel derives per tile from those values (its tile_inside test and the column pairing mq / de of a direct tile),
 * so that a test can say which of the kernel's paths a configuration reaches.  Runs the same checks of the geometry fields as irmv_engine_create (IRMV_ERR_ARG) and touches no GPU. */
#define IRMV_MAX_FRAME_BYTES 4294967296ull   /* 3 * src_width * src_height: kernels hold byte offsets into a frame in 32 bits */
enum {
    IRMV_FRONT_FUSED = 0,        /* the fused kernel runs */
    IRMV_FRONT_WIDTH_MOD4 = 1,   /* src_width is not a multiple of 4 (the source is read in groups of 4 pixels) */
    IRMV_FRONT_TAP_RANGE = 2,    /* a tile's source region has a pitch or a row count over 1023 (taps are packed in 10 bits) */
    IRMV_FRONT_STAGE_LIMIT = 3   /* a tile's source region is over the LDS stage limit */
};
typedef struct irmv_front_plan_t {
    int32_t fused;           /* 1: preprocess + model.0 + model.1 run as front_fused; 0: as three kernels, `reason` says why */
    int32_t reason;          /* IRMV_FRONT_* */
    int32_t fastx;           /* bit 0: every column tap is an aligned source pair at 1/2 : 1/2 (exactly 2 : 1); bit 1: direct tiles */
    int32_t tile_y;          /* model.1 output rows of a tile: 4, or 8 when every tile is direct */
    int32_t tiles_x, tiles_y;
    int32_t stage_bytes;     /* dynamic LDS of the fused kernel */
    int32_t box[4];          /* net-input columns [box[0], box[1]) and rows [box[2], box[3]) that have a source; the rest is padding */
    int32_t fx_i0, fx_step;  /* fastx: source pair of column box[0], and the pair's step per column (+2, or -2 under rotate180) */
    int32_t pair_cases;      /* direct tiles: which column pairings the tile columns hit.  bit 0: step +2, pair % 4 == 0;
                                bit 1: step +2, pair % 4 == 2; bit 2: step -2, pair % 4 == 0; bit 3: step -2, pair % 4 == 2 */
    int32_t tiles_inside;    /* tiles whose net-input pixels, halo included, all have a source ... */
    int32_t tiles_x_edge;    /* ... all rows, not all columns (padding or the net input's edge in x only) */
    int32_t tiles_y_edge;    /* ... all columns, not all rows */
    int32_t tiles_corner;    /* ... neither */
    int32_t max_pitch, max_rows;   /* the largest staged source region of a tile, in pixels (0 where src_width % 4 != 0) */
    int32_t upload_kernel;   /* 1: a single frame's upload may ride the upload kernel (slot bases and sizes are multiples of 16) */
    int32_t reserved[3];
} irmv_front_plan_t;
int irmv_front_plan(const irmv_engine_cfg *cfg, irmv_front_plan_t *out);

/* Host only: the channel slab of the SPPF LDS kernel for a launch of `batch` frames of [H][W][4C] (8, 16 or 32), or 0
 * for the global-memory kernel -- the rule the step's launch follows.  IRMV_ERR_ARG for a shape no engine has. */
int irmv_sppf_slab(int batch, int H, int W, int C);

/* Run one step eagerly with a HIP event pair around every kernel launch. */
int irmv_engine_profile(irmv_engine *e, int first_slot, int count, irmv_kernel_stat *stats, int cap, int *n);

/* ---- LDS residue test hooks (tests/test_gpu_lds_residue.py) ----------------
 * LDS keeps its contents from one kernel to the next: a kernel that reads a word it has not written gets the previous
 * workgroup's data.  These two choose and measure that residue on the calling thread's current device; no production
 * path uses them. */
#define IRMV_DEBUG_LDS_WORDS 40960      /* words of one workgroup's allocation: 160 KiB, the most a workgroup may have */
/* Launch several workgroups per CU that each claim IRMV_DEBUG_LDS_WORDS words of LDS and write pattern32 to every one,
 * then synchronize the device. */
int irmv_debug_lds_fill(uint32_t pattern32);
/* The same geometry, writing no LDS: out[4 w] = the number of words of workgroup w that hold pattern32, out[4 w + 1] = the
 * value it found in word `word` (an unwritten word flowing into an output: the bug class the residue test looks for),
 * out[4 w + 2], out[4 w + 3] = the HW_ID and XCC_ID registers of the CU it ran on.  *n = workgroups launched; out holds
 * 4 * cap words (IRMV_ERR_ARG if cap is smaller than that number; out NULL queries *n alone). */
int irmv_debug_lds_probe(uint32_t pattern32, uint32_t word, uint32_t *out, int cap, int *n);

/* ---- device-memory residue test hooks (tests/test_gpu_mem_residue.py) ------
 * Global memory keeps its contents from one step to the next too.  Every device range of an engine carries a class -- what
 * a step may rely on in it -- and a kind -- how its words are used ("device memory a step may rely on"); these
 * two list the ranges and choose the residue a step finds.  No production path uses them. */
#define IRMV_MEM_CONST   0   /* uploaded by the host, written by no step; a fill never touches it */
#define IRMV_MEM_ACT     1   /* activation tensor / head: a fill covers the channels some op of the step declares as written */
#define IRMV_MEM_CARRIED 2   /* a documented step-boundary invariant; a fill never touches it */
#define IRMV_MEM_SCRATCH 3   /* a step writes it before it reads it; a fill covers all of it */
#define IRMV_MEM_U8    0     /* plain data by width ... */
#define IRMV_MEM_F16   1
#define IRMV_MEM_F32   2
#define IRMV_MEM_F64   3
#define IRMV_MEM_INDEX 4     /* some kernel uses a word as an index, count, offset or label: index_max is the largest value valid there */
typedef struct irmv_mem_range {
    char name[48];
    int32_t mem_class, kind;     /* IRMV_MEM_* */
    uint32_t index_max;          /* IRMV_MEM_INDEX only */
    int32_t reserved;
    uint64_t bytes;
    uint64_t base;               /* the device address (tests read a CARRIED range through it; nothing else may) */
} irmv_mem_range;
/* The engine's device ranges in allocation order.  *n = their number; recs NULL queries *n alone, else IRMV_ERR_ARG if cap
 * is smaller. */
int irmv_engine_debug_allocs(irmv_engine *e, irmv_mem_range *recs, int cap, int *n);
/* Waits for the engine, then writes pattern32 over every SCRATCH range and over the written channel ranges of every ACT tensor
 * -- the union of what irmv_engine_ops and irmv_engine_op_io declare as written -- on all slots.  A range of kind INDEX gets
 * pattern32 == 0 ? 0 : index_max in every word instead, so no fill puts an out-of-range value where a kernel would use it as
 * an address.  The two halfwords of pattern32 must be equal (a fill has no phase).  *filled = the bytes written.  Touches no
 * CONST or CARRIED byte, no stale flag and no host memory. */
int irmv_engine_debug_fill_mem(irmv_engine *e, uint32_t pattern32, uint64_t *filled);
/* (tests) `bytes` of range `range` (its index in irmv_engine_debug_allocs' list) from `offset` on, as they lie in memory: waits
 * for the engine, runs no kernel and no read-back step, changes no flag.  IRMV_ERR_ARG outside the range. */
int irmv_engine_debug_read_mem(irmv_engine *e, int range, uint64_t offset, void *dst, uint64_t bytes);
/* (tests) the per-slot candidate counters as they lie in memory, one of the two CARRIED ranges (the other:
 * irmv_engine_debug_read_cand_bits).  *n = num_slots, or 0 on an engine that keeps none. */
int irmv_engine_debug_read_cand_counts(irmv_engine *e, int32_t *counts, int cap, int *n);

/* ---- frame metering: histograms inside the step, white balance from them ------------------------------------------------
 * The measuring half of the ISP.  A Bayer producer has bypassed the camera SDK's auto white balance and exposure, and the frame
 * it would meter exists only in device memory.  Metering is a per-frame record of four 256-bin integer histograms, computed on
 * the GPU (k_meter.hip) as one op of the captured step and delivered beside the slot's detections, or on demand for any
 * rectangle; small host functions turn a record into white-balance gains, a percentile and an exposure ratio.  Everything is an
 * integer count; irmv_detection_amd/metering.py is the host reference, bit for bit.
 *   rectangle   x0, y0, w, h in VIEW-LOCAL result coordinates: the frame of the slot's current view as detections see it
 *               (rotated under cfg.rotate180); a window slot's corner is NOT added.  w == h == 0: the whole view; otherwise
 *               w, h >= 1.  The rectangle is clipped to the view; an empty intersection is legal: all-zero histograms, n and rect
 *   VIEW        the samples are the pixels (x, y) of the clipped rectangle with (x - rx0) % step == 0 and (y - ry0) % step == 0,
 *               (rx0, ry0) the clipped corner, step 1, 2 or 4.  hist rows 0, 1, 2: the three channels as stored; row 3:
 *               gray = (p0*3735 + p1*19235 + p2*9798 + (1<<14)) >> 15, the light extraction's
 *   RAW         Bayer engines only: the raw CFA frame in front of gains and tone LUT -- what white balance must look at, or the
 *               loop chases its own gains.  The clipped rectangle is mapped to buffer coordinates (flipped under rotate180; a
 *               window slot in the window view: plus the buffer corner irmv_window_map gives) and shrunk inward to even bounds:
 *               a grid of 2 x 2 CFA cells.  Cell (i, j), counted from the shrunk region's corner in BUFFER coordinates, is
 *               sampled iff i % step == 0 and j % step == 0; all four sites of a sampled cell count.  Rows 0, 1, 2: the R, G, B
 *               sites by the engine's pattern in buffer coordinates; row 3: every sampled site
 *   record      n[r] = the samples of row r (= the sum of hist[r]); rect = the clipped rectangle (RAW: after shrinking) back in
 *               view-local result coordinates */
#define IRMV_METER_VIEW 0
#define IRMV_METER_RAW  1
typedef struct irmv_meter_opts {
    uint32_t struct_size;      /* = sizeof(irmv_meter_opts) */
    int32_t domain;            /* IRMV_METER_* */
    int32_t x0, y0, w, h;
    int32_t step;              /* 1, 2 or 4 */
    int32_t reserved[2];       /* must be 0 */
} irmv_meter_opts;
typedef struct irmv_frame_stats {
    uint32_t hist[4][256];
    uint32_t n[4];
    int32_t rect[4];           /* x, y, w, h */
    int32_t domain, step;      /* as metered; both 0 in the record of a step that ran with metering off */
    int32_t reserved[2];       /* 0 (the record is a multiple of 16 bytes) */
} irmv_frame_stats;
/* Host only, no GPU: where a rectangle lies in `view` (IRMV_VIEW_*) of an engine of this configuration, with the window (if
 * there is one) at (win_x0, win_y0) in result coordinates -- the function the engine and its kernels build from, like
 * irmv_window_map and irmv_front_plan -- and every argument check: IRMV_ERR_ARG for a wrong struct_size, an unknown domain,
 * IRMV_METER_RAW on IRMV_SRC_HWC8, a step other than 1, 2, 4, a negative size, exactly one of w, h zero, non-zero reserved
 * fields; also for IRMV_VIEW_FRAME without a window in cfg and for a window not inside the frame. */
typedef struct irmv_meter_map_t {
    int32_t rect[4];           /* the record's rect */
    int32_t region[4];         /* the same region x, y, w, h in the buffer that is read: the view's HWC frame as stored (pixels), or the
                                  raw frame (CFA sites, all four even) */
    int32_t phase[2];          /* VIEW: the first sampled column / row of the region, counted from its corner (non-zero under
                                  rotate180 only: the sample grid hangs at the rectangle's corner in result coordinates); RAW: 0 */
    int32_t grid[2];           /* sampled columns and rows: pixels, or 2 x 2 cells */
    uint32_t n[4];             /* the record's n */
    int32_t reserved[4];
} irmv_meter_map_t;
int irmv_meter_map(const irmv_engine_cfg *cfg, const irmv_meter_opts *opts, int view, int win_x0, int win_y0, irmv_meter_map_t *out);
/* Host only: out = {rows of the view's frame per partial workgroup, the most partial workgroups per frame, LDS bytes of the
 * histogram kernel, its threads, batch, the most per frame in a launch of more than `batch` frames, 0, 0}: a launch takes
 * min(out[1] or out[5], ceil(view rows / out[0])) workgroups per frame. */
int irmv_meter_limits(int32_t out[8]);
/* On demand, like irmv_engine_render, on any engine whether metering is enabled or not: waits for what is in flight, loads the
 * slot's current frame, launches once with THESE options, copies the record back and synchronizes.  Its scratch is made by the
 * first metering call of the engine; it captures and drops no graph and leaves the slot's step record alone. */
int irmv_engine_meter(irmv_engine *e, int slot, const irmv_meter_opts *opts, irmv_frame_stats *out);
/* Metering inside the step.  The first call with opts != NULL waits for everything in flight, allocates the per-slot records
 * (device, and pinned the way the irmv_det records are), the partials scratch and the device parameter record, and drops the
 * captured graphs once: from then on every ordinary step carries one more op (kind "meter" in irmv_engine_ops, appended to its
 * records; "frame_meter" in irmv_engine_profile) behind whatever produces the view's frame -- the demosaic, the crop -- or
 * first.  Later calls wait for the steps in flight and rewrite the parameter record, which the kernels read when they run: a
 * new rectangle, step or domain re-captures nothing, and neither does NULL, which sets "off" -- the kernel returns at once and
 * the step's record is all zero.  Options are per engine; clipping is per slot view when the step runs.  Tiled steps
 * (irmv_engine_submit_tiles) do not meter and leave the slots' records as they were; irmv_engine_run_post and the read-backs
 * do not meter either.  An engine on which this is never called allocates, captures, launches and returns what it always did.
 * IRMV_ERR_ARG (the checks of irmv_meter_map, before the GPU is touched) leaves the engine as it was.
 * irmv_engine_get_metering: *on = 0 and opts untouched while off or never set. */
int irmv_engine_set_metering(irmv_engine *e, const irmv_meter_opts *opts);
int irmv_engine_get_metering(const irmv_engine *e, irmv_meter_opts *opts, int *on);
/* The record of the slot's last ordinary step, valid after its wait; it reaches the host the way the slot's detections do.
 * IRMV_ERR_ARG before the first irmv_engine_set_metering with opts != NULL. */
int irmv_engine_frame_stats(irmv_engine *e, int slot, irmv_frame_stats *out);
/* Host only: what a record says.  Sums that can pass 2^64 are taken in 128 bits.
 * mean_q8: with S = sum v * hist[row][v] and N = sum hist[row][v] over lo <= v <= hi: *mean_q8 = (256 S + N / 2) / N, *count =
 *   N; N == 0 (an empty range too): both 0.  IRMV_ERR_ARG: a row outside 0..3, lo or hi outside 0..255.
 * percentile: the smallest v with cum(v) * den >= num * n[row], cum(v) = hist[row][0] + ... + hist[row][v].  IRMV_ERR_ARG:
 *   n[row] == 0, den == 0, num > den.
 * gray_world: IRMV_METER_RAW records only.  With S_c, N_c the sums of mean_q8 over [lo, hi] for c = R, G, B: gain_q8[1] = 256
 *   and for c = R, B gain_q8[c] = min(1023, (256 S_G N_c + S_c N_G / 2) / (S_c N_G)).  IRMV_ERR_ARG where S_c N_G == 0 for
 *   either, and gain_q8 is left alone.
 * exposure_q8: with p that percentile, *ratio_q8 = clamp((256 target + p / 2) / max(p, 1), 16, 4096): the factor (Q8) by which
 *   the exposure time should change.  The camera is the caller's.  IRMV_ERR_ARG: the percentile's, a target outside 0..255. */
int irmv_stats_mean_q8(const irmv_frame_stats *s, int row, int lo, int hi, uint64_t *mean_q8, uint64_t *count);
int irmv_stats_percentile(const irmv_frame_stats *s, int row, uint64_t num, uint64_t den, int *value);
int irmv_stats_gray_world(const irmv_frame_stats *s, int lo, int hi, uint16_t gain_q8[3]);
int irmv_stats_exposure_q8(const irmv_frame_stats *s, int row, uint64_t num, uint64_t den, int target, int *ratio_q8);

/* ---- PnPSolver (include/irmv_detection/pnp_solver.hpp:15-23) ------------ */
typedef struct irmv_pnp irmv_pnp;
int irmv_pnp_create(int device, const double camera_matrix[9], const double dist_coeffs[5], irmv_pnp **out);
void irmv_pnp_destroy(irmv_pnp *p);
/* img_pts [n][8] (LB, LT, RT, RB; pixels) -> rvec [n][3], tvec [n][3], ok [n];
 * IPPE on the GPU, one lane per armor (cv::solvePnP(..., SOLVEPNP_IPPE), src/pnp_solver.cpp:49-51). */
int irmv_pnp_solve(irmv_pnp *p, const float *img_pts, int n, int armor_size, double *rvec, double *tvec, int32_t *ok);
/* Both IPPE solutions (cv::solvePnPGeneric): rvec [n][2][3], tvec [n][2][3], err [n][2] (rms normalised residual), A first --
 * entry 0 is bit-identical to irmv_pnp_solve's answer, entry 1 the solution it throws away ("pose ambiguity" above).
 * ok [n]: bit 0 = irmv_pnp_solve's ok; bit 1 = entry 1 passed its own finiteness check.  Where bit 0 is clear, entry 1 and
 * both errors are zero. */
int irmv_pnp_solve2(irmv_pnp *p, const float *img_pts, int n, int armor_size, double *rvec, double *tvec, double *err, int32_t *ok);
/* The constrained pose ("constrained pose" above) of n quads with one up vector (normalised as irmv_engine_set_up does) and
 * one tilt normal_up in [-1, 1]: out [n].  Every quad is taken as solved input: state is 1 or -1, or 0 for a quad with a
 * non-finite or >= 2^24 coordinate.  opts->enable is not read.  IRMV_ERR_ARG: what the engine calls refuse. */
int irmv_pnp_solve_yaw(irmv_pnp *p, const float *img_pts, int n, int armor_size, const double up[3], double normal_up,
                       const irmv_yaw_opts *opts, irmv_yaw_pose *out);
/* The pose uncertainty ("pose uncertainty" above) of n quads at explicit poses rvec [n][3], tvec [n][3]: out [n].  This is also
 * how a caller gets the covariance of the alt pose.  up != NULL (normalised as irmv_engine_set_up does): the poses are taken
 * as constrained poses about it and the yaw block is computed too; NULL: yaw_state = 0.  Every quad is taken as solved
 * input: state is 1 or -1.  IRMV_ERR_ARG before the GPU is touched: a null argument, n < 0, a bad armor_size, sigma_px outside
 * (0, 64] or NaN, an up vector that is zero or not finite. */
int irmv_pnp_pose_cov(irmv_pnp *p, const float *img_pts, int n, int armor_size, const double *rvec, const double *tvec,
                      const double up[3], double sigma_px, irmv_pose_cov *out);

#ifdef __cplusplus
}
#endif
#endif /* IRMV_HIP_H */
