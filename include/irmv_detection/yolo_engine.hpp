// irmv_detection::YoloEngine on MI355X -- header-only facade over the C ABI of
// libirmv_hip.so with the reference's public interface (reference
// include/irmv_detection/yolo_engine.hpp:16-73): same constructor arguments,
// detect(), visualize_bboxes(), get_profiling_time(), get_rotated_image(),
// get_src_image_buffer().  Code written against the reference class
// (src/irm_detector.cpp:35-38,181-183; test/yolo_test.cpp:19-30,58-82) compiles
// unchanged against this one.
//
// Deliberate deviations (documented in DESIGN.md):
//  * HIP failures throw std::runtime_error (the reference checks no return code);
//  * the per-instance scale factors are per instance (the reference's are
//    function-local statics, src/yolo_engine.cpp:155-156);
//  * the source slot is never modified: rotation is folded into the sampling, so
//    get_rotated_image() materialises the rotated frame on demand (GPU kernel);
//  * a missing model file prints the reference's message and exit(0)s like
//    src/yolo_engine.cpp:38-39, but the file looked for is "<stem>.irmw".
#pragma once

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <iostream>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "irmv_detection/armor.hpp"
#include "irmv_detection/cv_compat.hpp"
#if IRMV_HAVE_OPENCV
#include <opencv2/imgproc.hpp>   // cv::rectangle, cv::putText (visualize_bboxes)
#endif
#include "irmv_hip.h"

namespace irmv_detection
{
class YoloEngine
{
public:
  struct bbox
  {
    std::array<float, 4> xyxy;
    float score;
    ArmorClass class_id;

    bool operator==(const bbox & o) const { return xyxy == o.xyxy && score == o.score && class_id == o.class_id; }
  };

  // HIP device used when none is given: IRMV_DEVICE (one process or thread per GPU sets it), else 0
  static int default_device()
  {
    const char * v = std::getenv("IRMV_DEVICE");
    return v ? std::atoi(v) : 0;
  }

  // Network input size when none is given: IRMV_NET_SIZE (a multiple of 32), else the reference's hard-coded 640
  // (src/yolo_engine.cpp:98-99); BASELINE configs[4] runs its model at 416.
  static int default_net_size()
  {
    const char * v = std::getenv("IRMV_NET_SIZE");
    return v ? std::atoi(v) : 640;
  }

  // The reference's constructor (yolo_engine.hpp:28-30).  Extension arguments: `device` (HIP ordinal, -1 = default_device()),
  // `warm_up_now` (false: the owner calls warm_up() itself, e.g. after building several engines) and `net_size`
  // (-1 = default_net_size()).  The model file decides the architecture (YOLOv8n or its ShuffleNetV2-backbone variant).
  // `src_format` (IRMV_SRC_*): what get_src_image_buffer() takes -- the reference's RGB8 frame (IRMV_SRC_HWC8), or the camera's
  // raw 8-bit Bayer frame of src_image_bytes() = width * height bytes (IRMV_SRC_BAYER_*8), demosaiced on the GPU with the Q8
  // white-balance gains `bayer_gain_q8` (R, G, B; 256 = 1.0).  get_rotated_image() is a CV_8UC3 frame either way.
  // `net_height` (-1 = square): the network input is net_size wide and net_height tall, e.g. 640 x 512 for the 1280 x 1024
  // camera (include/irmv_hip.h, irmv_engine_cfg::net_height); net_input_size() returns what the engine runs.
  // `bayer_demosaic` (IRMV_DEMOSAIC_*): the interpolation of a Bayer engine, bilinear or the 5 x 5 Malvar-He-Cutler filters.
  // `window` ({} = none): a tracking window -- detect() runs on a window.width x window.height crop of the frame at the
  // sensor's resolution (include/irmv_hip.h, irmv_engine_cfg::win_width).  src_image_size stays the full frame the producer
  // writes and bboxes come back in its coordinates; set_window() / set_window_center() move the window between detect()
  // calls; get_rotated_image() is then the rotated window.  set_view(View::Frame) runs detect() on the whole frame instead
  // (the search after a lost target), set_view(View::Window) goes back; get_rotated_image() follows the view.
  // `tile_overlap` (a negative value = off; needs a window): the tiled search.  The engine gets 1 + nx * ny slots: slot 0 stays
  // the tracking slot and owns the frame, slots 1.. hold the grid irmv_tile_grid gives for that least overlap of neighbouring
  // windows, set once.  detect_tiles() then searches the frame already in get_src_image_buffer() at the sensor's resolution:
  // every tile runs its window of that frame in ONE step and the step merges their lists (include/irmv_hip.h, "tiled search").
  // `point_source` (IRMV_POINTS_*): IRMV_POINTS_REFINED snaps the keypoint head's points to the light bars found at them, inside
  // the step (include/irmv_hip.h, "refined point source"); set_refine() changes its two parameters live.
  YoloEngine(const std::string & onnx_file_path, cv::Size src_image_size, bool enable_profiling = false, int device = -1,
             bool warm_up_now = true, int net_size = -1, int src_format = IRMV_SRC_HWC8,
             std::array<uint16_t, 3> bayer_gain_q8 = {256, 256, 256}, int net_height = -1,
             int bayer_demosaic = IRMV_DEMOSAIC_BILINEAR, cv::Size window = {}, cv::Size tile_overlap = cv::Size(-1, -1),
             int point_source = IRMV_POINTS_AUTO)
  : src_image_size_(src_image_size), window_size_(window), enable_profiling_(enable_profiling)
  {
    irmv_engine_cfg cfg;
    irmv_engine_cfg_default(&cfg);
    cfg.src_format = src_format;
    for (int i = 0; i < 3; i++) cfg.bayer_gain_q8[i] = bayer_gain_q8[static_cast<size_t>(i)];
    cfg.bayer_demosaic = static_cast<uint16_t>(bayer_demosaic);
    cfg.net_size = net_size > 0 ? net_size : default_net_size();
    cfg.net_height = net_height > 0 ? net_height : 0;
    cfg.device = device >= 0 ? device : default_device();
    cfg.src_width = src_image_size.width;
    cfg.src_height = src_image_size.height;
    cfg.win_width = window.width;
    cfg.win_height = window.height;
    cfg.num_slots = 1;  // one engine per TripleBuffer slot, like the reference node
    cfg.point_source = point_source;
    std::vector<int32_t> tile_xy;
    if (tile_overlap.width >= 0 && tile_overlap.height >= 0) {
      int nx = 0, ny = 0;
      tile_xy.resize(2 * IRMV_MAX_TILES);
      if (irmv_tile_grid(&cfg, tile_overlap.width, tile_overlap.height, tile_xy.data(), IRMV_MAX_TILES, &num_tiles_, &nx, &ny) != IRMV_OK)
        throw std::runtime_error(std::string("YoloEngine: tile_overlap: ") + irmv_last_error());
      cfg.num_slots = 1 + num_tiles_;
      tile_grid_ = cv::Size(nx, ny);
    }
    cfg.weights_path = onnx_file_path.c_str();
    const int rc = irmv_engine_create(&cfg, &engine_);
    if (rc == IRMV_ERR_MODEL) {
      std::cout << "Please convert the model to <stem>.irmw first (" << irmv_last_error() << ")." << std::endl;
      std::exit(0);
    }
    if (rc != IRMV_OK) throw std::runtime_error(std::string("YoloEngine: ") + irmv_last_error());
    src_image_buffer_ = irmv_engine_src_buffer(engine_, 0);
    rotated_ = has_window() ? cv::Mat(window.height, window.width, CV_8UC3) : cv::Mat(src_image_size.height, src_image_size.width, CV_8UC3);
    dets_.resize(static_cast<size_t>(irmv_engine_max_det(engine_)));
    for (int t = 0; t < num_tiles_; t++)
      if (irmv_engine_set_window(engine_, 1 + t, tile_xy[static_cast<size_t>(2 * t)], tile_xy[static_cast<size_t>(2 * t + 1)]) != IRMV_OK)
        throw std::runtime_error(std::string("YoloEngine: tile grid: ") + irmv_last_error());
    tile_dets_.resize(num_tiles_ > 0 ? dets_.size() : 0);
    irmv_engine_get_class_policy(engine_, &base_policy_);   // the uniform policy of the engine's score threshold and plate
    user_policy_ = base_policy_;
    if (warm_up_now) warm_up();
  }

  // width x height of the network input
  cv::Size net_input_size() const
  {
    int w = 0, h = 0;
    irmv_engine_net_dims(engine_, &w, &h);
    return cv::Size(w, h);
  }

  void warm_up()
  {
    for (int i = 0; i < 50; i++) detect();  // as src/yolo_engine.cpp:114-116
  }

  // true: the model has a keypoint head and every detection carries its four armor points and pose (irmv_det);
  // false: a bbox-only model like the reference's -- the points come from extract_armors()
  // (a refined engine is a keypoint engine whose points were snapped to the light bars)
  bool has_keypoint_head() const { return irmv_engine_point_source(engine_) == IRMV_POINTS_KEYPOINT_HEAD || refines_points(); }
  bool refines_points() const { return irmv_engine_point_source(engine_) == IRMV_POINTS_REFINED; }

  // The refined point source's two live parameters (irmv_engine_set_refine): defaults 0.5 and 4 source pixels, neither
  // validated on a trained model.  Waits for the steps in flight; re-captures nothing.
  void set_refine(float snap, float roi_margin)
  {
    if (irmv_engine_set_refine(engine_, snap, roi_margin) != IRMV_OK)
      throw std::runtime_error(std::string("YoloEngine::set_refine: ") + irmv_last_error());
  }

  // The node's live parameters of the classical extraction (src/irm_detector.cpp:372-403)
  void set_extract_params(int binary_threshold, float light_min_ratio, float light_max_ratio, float light_max_angle, double min_small_cd,
                          double max_small_cd, double min_large_cd, double max_large_cd)
  {
    const double cd[4] = {min_small_cd, max_small_cd, min_large_cd, max_large_cd};
    if (irmv_engine_set_extract_params(engine_, binary_threshold, light_min_ratio, light_max_ratio, light_max_angle, cd) != IRMV_OK)
      throw std::runtime_error(std::string("YoloEngine::set_extract_params: ") + irmv_last_error());
  }

  // The camera ISP's white balance and tone curve of a Bayer engine, retuned while it lives: Q8 gains (R, G, B; 256 = 1.0) and
  // a [3][256] byte LUT (rows R, G, B; nullptr = identity), out = lut[c][min(255, (v * gain[c] + 128) >> 8)].  Waits for the
  // steps in flight; every later detect() / get_rotated_image() uses the new values (irmv_engine_set_bayer_isp).
  void set_bayer_isp(std::array<uint16_t, 3> gain_q8, const uint8_t * lut = nullptr)
  {
    if (irmv_engine_set_bayer_isp(engine_, gain_q8.data(), lut) != IRMV_OK)
      throw std::runtime_error(std::string("YoloEngine::set_bayer_isp: ") + irmv_last_error());
    rotated_valid_ = false;
  }
  bool is_bayer() const { return irmv_engine_src_format(engine_) != IRMV_SRC_HWC8; }
  // the gains in force, and (lut != nullptr) the [3][256] tone LUT behind them
  std::array<uint16_t, 3> bayer_gains(std::vector<uint8_t> * lut = nullptr) const
  {
    std::array<uint16_t, 3> g{256, 256, 256};
    if (lut) lut->resize(3 * 256);
    if (irmv_engine_get_bayer_isp(engine_, g.data(), lut ? lut->data() : nullptr) != IRMV_OK)
      throw std::runtime_error(std::string("YoloEngine::bayer_gains: ") + irmv_last_error());
    return g;
  }

  // ---- frame metering (include/irmv_hip.h, "frame metering") ----
  // set_metering: from the next detect() on every step also computes four 256-bin histograms of the rectangle (view-local
  // result coordinates; w == h == 0: the whole view), sampled every `step` pixels: IRMV_METER_VIEW = the frame the network
  // sees (three channels and gray), IRMV_METER_RAW = a Bayer engine's raw frame in front of gains and LUT (R, G, B sites and
  // all).  nullptr: off.  The first enabling call re-captures the steps once; later ones, nullptr included, none.
  // frame_stats(): the record of the last detect().  meter(): the frame in the buffer now, on demand, on any engine.
  // irmv_stats_mean_q8 / _percentile / _gray_world / _exposure_q8 read a record.
  static irmv_meter_opts meter_opts(int domain = IRMV_METER_VIEW, cv::Point corner = {}, cv::Size size = {}, int step = 1)
  {
    irmv_meter_opts o{};
    o.struct_size = sizeof o;
    o.domain = domain;
    o.x0 = corner.x; o.y0 = corner.y; o.w = size.width; o.h = size.height;
    o.step = step;
    return o;
  }
  void set_metering(const irmv_meter_opts * o)
  {
    if (irmv_engine_set_metering(engine_, o) != IRMV_OK) throw std::runtime_error(std::string("YoloEngine::set_metering: ") + irmv_last_error());
  }
  void set_metering(int domain, cv::Point corner = {}, cv::Size size = {}, int step = 1)
  {
    const irmv_meter_opts o = meter_opts(domain, corner, size, step);
    set_metering(&o);
  }
  // the options in force; false: off (or never set)
  bool metering(irmv_meter_opts * o = nullptr) const
  {
    int on = 0;
    irmv_engine_get_metering(engine_, o, &on);
    return on != 0;
  }
  irmv_frame_stats frame_stats() const
  {
    irmv_frame_stats s;
    if (irmv_engine_frame_stats(engine_, 0, &s) != IRMV_OK) throw std::runtime_error(std::string("YoloEngine::frame_stats: ") + irmv_last_error());
    return s;
  }
  irmv_frame_stats meter(int domain = IRMV_METER_VIEW, cv::Point corner = {}, cv::Size size = {}, int step = 1)
  {
    const irmv_meter_opts o = meter_opts(domain, corner, size, step);
    irmv_frame_stats s;
    if (irmv_engine_meter(engine_, 0, &o, &s) != IRMV_OK) throw std::runtime_error(std::string("YoloEngine::meter: ") + irmv_last_error());
    return s;
  }

  // ---- class policy: per-class score thresholds, colour mask, plate size (include/irmv_hip.h, irmv_class_policy) ----
  // Two things the caller sets independently, one table in the engine: the caller's policy (score_thr[c] >= 1 switches
  // class c off where candidates are emitted; plate[c] is IRMV_ARMOR_SMALL / _LARGE, the object points PnP uses for a
  // detection of class c) and the enemy colour, which switches the own colour's classes off on top of it.  Every call here
  // waits for the steps in flight, uploads the table ONCE, holds from the next detect() on and re-captures nothing.  A
  // refused argument throws and leaves both as they were.
  void set_class_policy(const irmv_class_policy & p) { apply_class_policy(p, enemy_color_, "YoloEngine::set_class_policy: "); }
  // ... and the colour in the same upload
  void set_class_policy(const irmv_class_policy & p, int enemy_color) { apply_class_policy(p, enemy_color, "YoloEngine::set_class_policy: "); }
  // The reference node's enemy_color ("0 for blue, 1 for red", src/irm_detector.cpp:154-160; declared there, never used):
  // 0 = the enemy is blue, B1..BS stay on and R1..RS are off; 1 = the enemy is red; -1 = no filter.  The caller's thresholds
  // and plates stay: a class with its own threshold keeps it whenever its colour is on.
  void set_enemy_color(int enemy_color) { apply_class_policy(user_policy_, enemy_color, "YoloEngine::set_enemy_color: "); }
  // Back to the engine's one score threshold and one plate model for every class, and no colour filter.
  void reset_class_policy() { apply_class_policy(base_policy_, -1, "YoloEngine::reset_class_policy: "); }
  // The caller's policy (without the colour mask) and the colour; class_policy() is what the engine holds: both combined.
  const irmv_class_policy & user_class_policy() const { return user_policy_; }
  int enemy_color() const { return enemy_color_; }
  irmv_class_policy class_policy() const
  {
    irmv_class_policy p;
    if (irmv_engine_get_class_policy(engine_, &p) != IRMV_OK)
      throw std::runtime_error(std::string("YoloEngine::class_policy: ") + irmv_last_error());
    return p;
  }

  // ---- pose ambiguity: both IPPE solutions per armor, and a gravity prior (include/irmv_hip.h, "pose ambiguity") ----
  // From the first set_pose_prior on every detect() also delivers the solution its records do not report (pose_alts()); mode
  // IRMV_POSE_PRIOR lets the per-class tilt prior choose between the two.  nullptr: IRMV_POSE_MIN_ERR with the defaults.  The
  // first call re-captures the steps once; later calls and set_up re-capture nothing.  A refused value throws, nothing changes.
  void set_pose_prior(const irmv_pose_prior * p)
  {
    if (irmv_engine_set_pose_prior(engine_, p) != IRMV_OK)
      throw std::runtime_error(std::string("YoloEngine::set_pose_prior: ") + irmv_last_error());
    pose_alts_on_ = true;
  }
  void set_pose_prior(int mode, double ambiguity_ratio = 8.0, double normal_up = -0.25881904510252074)
  {
    irmv_pose_prior p{};
    p.struct_size = sizeof p; p.mode = mode; p.ambiguity_ratio = ambiguity_ratio;
    for (double & s : p.normal_up) s = normal_up;
    p.normal_up_default = normal_up;
    set_pose_prior(&p);
  }
  irmv_pose_prior pose_prior() const
  {
    irmv_pose_prior p;
    if (irmv_engine_get_pose_prior(engine_, &p) != IRMV_OK)
      throw std::runtime_error(std::string("YoloEngine::pose_prior: ") + irmv_last_error());
    return p;
  }
  bool delivers_pose_alts() const { return pose_alts_on_; }
  // The gimbal's up vector in the camera frame PnP sees (any length; default (0, -1, 0)): per frame, before detect()
  void set_up(const std::array<double, 3> & up)
  {
    if (irmv_engine_set_up(engine_, 0, up.data()) != IRMV_OK)
      throw std::runtime_error(std::string("YoloEngine::set_up: ") + irmv_last_error());
  }
  std::array<double, 3> up() const
  {
    std::array<double, 3> u{};
    if (irmv_engine_get_up(engine_, 0, u.data()) != IRMV_OK)
      throw std::runtime_error(std::string("YoloEngine::up: ") + irmv_last_error());
    return u;
  }
  // Parallel to last_detections(): entry i is the other solution of record i (empty before the first set_pose_prior)
  std::vector<irmv_pose_alt> pose_alts() const { return side_records<irmv_pose_alt>(pose_alts_on_, irmv_engine_pose_alts, "pose_alts"); }

  // ---- constrained pose (include/irmv_hip.h, "constrained pose") ----
  // From the first set_yaw_solve on every detect() also solves, per solved record, the plate's yaw at the class's known tilt
  // (set_pose_prior's normal_up) and the up vector (set_up): yaw_poses().  The first call re-captures the steps once; later
  // calls, set_up and set_pose_prior re-capture nothing.  A refused value throws, nothing changes.
  static irmv_yaw_opts yaw_opts(bool enable = true, int rounds = 4, double tau_max = 1.0, double horizon_min = 1e-4)
  {
    irmv_yaw_opts o{};
    o.struct_size = sizeof o; o.enable = enable ? 1 : 0; o.rounds = rounds; o.tau_max = tau_max; o.horizon_min = horizon_min;
    return o;
  }
  void set_yaw_solve(const irmv_yaw_opts & o = yaw_opts())
  {
    if (irmv_engine_set_yaw_solve(engine_, &o) != IRMV_OK)
      throw std::runtime_error(std::string("YoloEngine::set_yaw_solve: ") + irmv_last_error());
    yaw_on_ = true;
  }
  irmv_yaw_opts yaw_solve() const
  {
    irmv_yaw_opts o;
    if (irmv_engine_get_yaw_solve(engine_, &o) != IRMV_OK)
      throw std::runtime_error(std::string("YoloEngine::yaw_solve: ") + irmv_last_error());
    return o;
  }
  // Parallel to last_detections(): entry i is the constrained pose of record i (empty before the first set_yaw_solve)
  std::vector<irmv_yaw_pose> yaw_poses() const { return side_records<irmv_yaw_pose>(yaw_on_, irmv_engine_yaw_poses, "yaw_poses"); }

  // ---- pose uncertainty (include/irmv_hip.h, "pose uncertainty") ----
  // From the first set_pose_cov on every detect() also computes, per solved record, the first-order covariance of its IPPE
  // pose and -- where yaws are solved -- of its constrained pose under corner noise of sigma_px pixels: pose_covs().  The
  // first call re-captures the steps once; later calls re-capture nothing.  A refused value throws, nothing changes.
  static irmv_pose_cov_opts pose_cov_opts(bool enable = true, double sigma_px = 1.0)
  {
    irmv_pose_cov_opts o{};
    o.struct_size = sizeof o; o.enable = enable ? 1 : 0; o.sigma_px = sigma_px;
    return o;
  }
  void set_pose_cov(const irmv_pose_cov_opts & o = pose_cov_opts())
  {
    if (irmv_engine_set_pose_cov(engine_, &o) != IRMV_OK)
      throw std::runtime_error(std::string("YoloEngine::set_pose_cov: ") + irmv_last_error());
    pose_cov_on_ = true;
  }
  irmv_pose_cov_opts pose_cov() const
  {
    irmv_pose_cov_opts o;
    if (irmv_engine_get_pose_cov(engine_, &o) != IRMV_OK)
      throw std::runtime_error(std::string("YoloEngine::pose_cov: ") + irmv_last_error());
    return o;
  }
  // Parallel to last_detections(): entry i is the covariance of record i (empty before the first set_pose_cov)
  std::vector<irmv_pose_cov> pose_covs() const { return side_records<irmv_pose_cov>(pose_cov_on_, irmv_engine_pose_covs, "pose_covs"); }

  // ---- armor tracks (include/irmv_hip.h, "armor tracks") ----
  // From the first set_tracking on every detect() also advances the engine's track table over its detections, in submit
  // order: det_tracks() and tracks().  Nothing is re-captured.  A refused value throws, nothing changes.
  static irmv_track_opts track_opts(bool enable = true)
  {
    irmv_track_opts o{};
    irmv_track_default_opts(&o);   // the library's defaults
    o.enable = enable ? 1 : 0;
    return o;
  }
  void set_tracking(const irmv_track_opts & o = track_opts())
  {
    if (irmv_engine_set_tracking(engine_, &o) != IRMV_OK)
      throw std::runtime_error(std::string("YoloEngine::set_tracking: ") + irmv_last_error());
    tracking_on_ = true;
  }
  irmv_track_opts tracking() const
  {
    irmv_track_opts o;
    if (irmv_engine_get_tracking(engine_, &o) != IRMV_OK)
      throw std::runtime_error(std::string("YoloEngine::tracking: ") + irmv_last_error());
    return o;
  }
  // The stamp (seconds) and the camera pose in the world of the frames to come, live as set_up is
  void set_stamp(double t)
  {
    if (irmv_engine_set_stamp(engine_, 0, t) != IRMV_OK) throw std::runtime_error(std::string("YoloEngine::set_stamp: ") + irmv_last_error());
  }
  void set_camera_pose(const std::array<double, 9> & R_wc, const std::array<double, 3> & t_wc)
  {
    if (irmv_engine_set_camera_pose(engine_, 0, R_wc.data(), t_wc.data()) != IRMV_OK)
      throw std::runtime_error(std::string("YoloEngine::set_camera_pose: ") + irmv_last_error());
  }
  // Parallel to last_detections(): entry i is what the tracker made of record i (empty before the first set_tracking)
  std::vector<irmv_det_track> det_tracks() const { return side_records<irmv_det_track>(tracking_on_, irmv_engine_det_tracks, "det_tracks"); }
  // The table as the last detect() left it: IRMV_TRACK_CAP entries, free ones included (empty before the first set_tracking)
  std::vector<irmv_track> tracks(irmv_track_frame * frame = nullptr) const
  {
    std::vector<irmv_track> a;
    if (!tracking_on_) return a;
    a.resize(IRMV_TRACK_CAP);
    int n = 0;
    if (irmv_engine_tracks(engine_, 0, frame, a.data(), IRMV_TRACK_CAP, &n) != IRMV_OK)
      throw std::runtime_error(std::string("YoloEngine::tracks: ") + irmv_last_error());
    a.resize(static_cast<size_t>(n));
    return a;
  }
  void reset_tracks()
  {
    if (irmv_engine_reset_tracks(engine_) != IRMV_OK) throw std::runtime_error(std::string("YoloEngine::reset_tracks: ") + irmv_last_error());
  }

  // ---- plate patches (include/irmv_hip.h, "plate patches") ----
  // From the first set_patches on every detect() also rectifies, per record with armor_valid == 1, the 20 x 28 gray number
  // image between the light bars out of the slot's frame: plate_patches().  The first call re-captures the steps once; later
  // calls re-capture nothing.  A refused value throws, nothing changes.
  static irmv_patch_opts patch_opts(bool enable = true, int span_small = 32, int span_large = 54, int light_rows = 12, int top = 7)
  {
    irmv_patch_opts o{};
    o.struct_size = sizeof o; o.enable = enable ? 1 : 0; o.span[0] = span_small; o.span[1] = span_large; o.light_rows = light_rows; o.top = top;
    return o;
  }
  void set_patches(const irmv_patch_opts & o = patch_opts())
  {
    if (irmv_engine_set_patches(engine_, &o) != IRMV_OK)
      throw std::runtime_error(std::string("YoloEngine::set_patches: ") + irmv_last_error());
    patches_on_ = true;
  }
  irmv_patch_opts patches() const
  {
    irmv_patch_opts o;
    if (irmv_engine_get_patches(engine_, &o) != IRMV_OK)
      throw std::runtime_error(std::string("YoloEngine::patches: ") + irmv_last_error());
    return o;
  }
  // Parallel to last_detections(): entry i is the patch of record i (empty before the first set_patches)
  std::vector<irmv_plate_patch> plate_patches() const { return side_records<irmv_plate_patch>(patches_on_, irmv_engine_plate_patches, "plate_patches"); }

  // ---- plate numbers (include/irmv_hip.h, "plate numbers") ----
  // A small MLP reads each plate patch: set_number_model (an .irmn file, as irmv_detection_amd/number_net.py writes one, or a
  // model in memory), then set_numbers -- from then on every detect() also delivers label, runner-up, margin and logits beside
  // each record: plate_numbers().  set_numbers(true) needs a model and turns the patches on, with their defaults, where they
  // were never set.  The first enabling call re-captures the steps once; later calls and a new model re-capture nothing.  A
  // refused model or call throws, nothing changes.
  void set_number_model(const std::string & irmn_path)
  {
    if (irmv_engine_load_number_model(engine_, irmn_path.c_str()) != IRMV_OK)
      throw std::runtime_error(std::string("YoloEngine::set_number_model: ") + irmv_last_error());
  }
  void set_number_model(const irmv_number_model & m)
  {
    if (irmv_engine_set_number_model(engine_, &m) != IRMV_OK)
      throw std::runtime_error(std::string("YoloEngine::set_number_model: ") + irmv_last_error());
  }
  void set_numbers(bool enable = true)
  {
    irmv_number_opts o{};
    o.struct_size = sizeof o; o.enable = enable ? 1 : 0;
    if (irmv_engine_set_numbers(engine_, &o) != IRMV_OK)
      throw std::runtime_error(std::string("YoloEngine::set_numbers: ") + irmv_last_error());
    if (enable) numbers_on_ = patches_on_ = true;   // (a first call with enable = false changes nothing)
  }
  bool numbers() const
  {
    irmv_number_opts o;
    if (irmv_engine_get_numbers(engine_, &o) != IRMV_OK)
      throw std::runtime_error(std::string("YoloEngine::numbers: ") + irmv_last_error());
    return o.enable != 0;
  }
  // Parallel to last_detections(): entry i is the number of record i (empty before the first set_numbers(true))
  std::vector<irmv_plate_number> plate_numbers() const { return side_records<irmv_plate_number>(numbers_on_, irmv_engine_plate_numbers, "plate_numbers"); }
  // On demand, enabled or not: the numbers of explicit patch records under the engine's model
  std::vector<irmv_plate_number> numbers_at(const std::vector<irmv_plate_patch> & patches) const
  {
    std::vector<irmv_plate_number> out(patches.size());
    if (irmv_engine_numbers_at(engine_, patches.data(), static_cast<int>(patches.size()), out.data()) != IRMV_OK)
      throw std::runtime_error(std::string("YoloEngine::numbers_at: ") + irmv_last_error());
    return out;
  }
  // The softmax of a record's first n_classes logits (host, in double); all zero for a "no answer" record
  static std::array<float, 16> number_softmax(const irmv_plate_number & r, int n_classes)
  {
    std::array<float, 16> p{};
    if (irmv_number_softmax(&r, n_classes, p.data()) != IRMV_OK)
      throw std::runtime_error(std::string("YoloEngine::number_softmax: ") + irmv_last_error());
    return p;
  }

  // ---- tracking window ----
  bool has_window() const { return window_size_.width > 0 && window_size_.height > 0; }
  // The window's top-left corner in the coordinates bboxes come back in (the rotated frame); from the next detect() on.
  void set_window(cv::Point top_left)
  {
    if (irmv_engine_set_window(engine_, 0, top_left.x, top_left.y) != IRMV_OK)
      throw std::runtime_error(std::string("YoloEngine::set_window: ") + irmv_last_error());
    rotated_valid_ = false;
  }
  // Centre the window on a point -- the last detection's box centre --, clamped into the frame.  Returns the corner it set.
  cv::Point set_window_center(cv::Point2f center)
  {
    const int x0 = std::clamp(static_cast<int>(std::floor(center.x - window_size_.width / 2.0 + 0.5)), 0, src_image_size_.width - window_size_.width);
    const int y0 = std::clamp(static_cast<int>(std::floor(center.y - window_size_.height / 2.0 + 0.5)), 0, src_image_size_.height - window_size_.height);
    set_window(cv::Point(x0, y0));
    return cv::Point(x0, y0);
  }
  // The current window as (top-left corner, size)
  std::pair<cv::Point, cv::Size> window() const
  {
    int x0 = 0, y0 = 0, w = 0, h = 0;
    if (irmv_engine_get_window(engine_, 0, &x0, &y0, &w, &h) != IRMV_OK)
      throw std::runtime_error(std::string("YoloEngine::window: ") + irmv_last_error());
    return {cv::Point(x0, y0), cv::Size(w, h)};
  }

  // ---- search view (window engines): detect() on the window, or on the whole frame after the target is lost ----
  enum class View { Window, Frame };
  // From the next detect() on.  Frame: what an engine without a window on the same frame computes -- no crop, no offset, the
  // configured camera; the frame already in the pinned buffer can be run again without touching it.  The first Frame of an
  // engine builds that view (call it once at start-up); switching back and forth afterwards re-captures nothing.
  void set_view(View v)
  {
    if (irmv_engine_set_view(engine_, 0, v == View::Frame ? IRMV_VIEW_FRAME : IRMV_VIEW_WINDOW) != IRMV_OK)
      throw std::runtime_error(std::string("YoloEngine::set_view: ") + irmv_last_error());
    const cv::Size sz = v == View::Frame ? src_image_size_ : window_size_;
    if (rotated_.cols != sz.width || rotated_.rows != sz.height) rotated_ = cv::Mat(sz.height, sz.width, CV_8UC3);   // get_rotated_image(): the view's frame
    rotated_valid_ = false;
  }
  View view() const
  {
    int v = IRMV_VIEW_WINDOW;
    if (irmv_engine_get_view(engine_, 0, &v, nullptr, nullptr) != IRMV_OK)
      throw std::runtime_error(std::string("YoloEngine::view: ") + irmv_last_error());
    return v == IRMV_VIEW_FRAME ? View::Frame : View::Window;
  }

  ~YoloEngine() { irmv_engine_destroy(engine_); }
  YoloEngine(const YoloEngine &) = delete;
  YoloEngine & operator=(const YoloEngine &) = delete;

  std::vector<bbox> detect()
  {
    int n = 0;
    const int rc = irmv_engine_detect(engine_, 0, dets_.data(), static_cast<int>(dets_.size()), &n);
    if (rc != IRMV_OK) throw std::runtime_error(std::string("YoloEngine::detect: ") + irmv_last_error());
    rotated_valid_ = false;
    std::vector<bbox> out;
    out.reserve(static_cast<size_t>(n));
    for (int i = 0; i < n; i++) {
      const irmv_det & d = dets_[static_cast<size_t>(i)];
      out.push_back(bbox{{d.xyxy[0], d.xyxy[1], d.xyxy[2], d.xyxy[3]}, d.score, static_cast<ArmorClass>(d.class_id)});
    }
    n_last_ = n;
    return out;
  }

  // ---- tiled search (constructor argument tile_overlap) ----
  int num_tiles() const { return num_tiles_; }
  cv::Size tile_grid() const { return tile_grid_; }   // tiles per row x per column
  // The frame already in get_src_image_buffer(), searched at the sensor's resolution: one step of all tiles, merged on the GPU
  // into one list in full-frame coordinates (at most max_det boxes: whole boxes first, by score).  The tracking slot's window,
  // view and last results stay as they are.
  std::vector<bbox> detect_tiles()
  {
    if (num_tiles_ < 1) throw std::runtime_error("YoloEngine::detect_tiles: the engine was built without tile_overlap");
    int n = 0;
    if (irmv_engine_submit_tiles(engine_, 0, 1, num_tiles_, IRMV_SUBMIT_H2D) != IRMV_OK || irmv_engine_wait_slots(engine_, 1, num_tiles_) != IRMV_OK ||
        irmv_engine_tile_results(engine_, 1, tile_dets_.data(), static_cast<int>(tile_dets_.size()), &n, nullptr) != IRMV_OK)
      throw std::runtime_error(std::string("YoloEngine::detect_tiles: ") + irmv_last_error());
    std::vector<bbox> out;
    out.reserve(static_cast<size_t>(n));
    for (int i = 0; i < n; i++) {
      const irmv_det & d = tile_dets_[static_cast<size_t>(i)].det;
      out.push_back(bbox{{d.xyxy[0], d.xyxy[1], d.xyxy[2], d.xyxy[3]}, d.score, static_cast<ArmorClass>(d.class_id)});
    }
    n_last_tiles_ = n;
    return out;
  }
  // The records of the last detect_tiles(): each detection with its pose, the tile it came from and whether a seam cut it.
  const irmv_tile_det * last_tile_detections(int * n) const
  {
    *n = n_last_tiles_;
    return tile_dets_.data();
  }
  // The merge's two live parameters (irmv_engine_set_tile_merge): defaults 0.5 and 2 source pixels, neither validated on a
  // trained model.
  void set_tile_merge(float ios_thr, float edge_margin)
  {
    if (irmv_engine_set_tile_merge(engine_, ios_thr, edge_margin) != IRMV_OK)
      throw std::runtime_error(std::string("YoloEngine::set_tile_merge: ") + irmv_last_error());
  }

  // The full per-armor result of the last detect(): keypoints and pose, computed on the GPU.
  const irmv_det * last_detections(int * n) const
  {
    *n = n_last_;
    return dets_.data();
  }

  // Extension: the node's IrmDetector::extract_armors(get_rotated_image(), bboxes) (reference src/irm_detector.cpp:183,
  // 292-355) on the GPU, on the frame of the last detect().  One Armor per bbox in which two gated lights were found,
  // in bbox order, like the reference; `poses`, if given, receives the IPPE pose of each returned armor.
  std::vector<Armor> extract_armors(const std::vector<bbox> & bboxes, std::vector<irmv_det> * poses = nullptr)
  {
    std::vector<Armor> armors;
    if (bboxes.empty()) return armors;
    std::vector<float> xyxy;
    xyxy.reserve(bboxes.size() * 4);
    for (const auto & b : bboxes) xyxy.insert(xyxy.end(), b.xyxy.begin(), b.xyxy.end());
    std::vector<irmv_det> out(bboxes.size());
    if (irmv_engine_extract_armors(engine_, 0, xyxy.data(), static_cast<int>(bboxes.size()), out.data()) != IRMV_OK)
      throw std::runtime_error(std::string("YoloEngine::extract_armors: ") + irmv_last_error());
    for (size_t i = 0; i < out.size(); i++) {
      const irmv_det & d = out[i];
      if (d.armor_valid != 1) continue;   // no pair of lights (0) or scratch exhausted (-1): the reference emits nothing either
      Armor a(Light(cv::Point2f(d.kpts[2], d.kpts[3]), cv::Point2f(d.kpts[0], d.kpts[1])),
              Light(cv::Point2f(d.kpts[4], d.kpts[5]), cv::Point2f(d.kpts[6], d.kpts[7])));
      a.size = d.armor_size == IRMV_ARMOR_LARGE ? ArmorSize::LARGE : ArmorSize::SMALL;
      a.armor_class = bboxes[i].class_id;
      a.confidence = bboxes[i].score;
      armors.push_back(a);
      if (poses) poses->push_back(d);
    }
    return armors;
  }

  void visualize_bboxes(cv::Mat & image, const std::vector<bbox> & bboxes) const
  {
    if (image.cols != src_image_size_.width || image.rows != src_image_size_.height) {
      std::cerr << "[YoloEngine::visualize_bboxes] Image size mismatch" << std::endl;
      return;
    }
    for (const auto & b : bboxes) {
      const std::string name(armor_class_name(b.class_id));
      const bool blue = name[0] == 'B';
#if IRMV_HAVE_OPENCV
      // the reference's own calls (src/yolo_engine.cpp:229-241)
      const cv::Point p1(int(b.xyxy[0]), int(b.xyxy[1])), p2(int(b.xyxy[2]), int(b.xyxy[3]));
      const cv::Scalar color = blue ? cv::Scalar(0, 0, 255) : cv::Scalar(255, 0, 0);
      cv::rectangle(image, p1, p2, color, 2);
      cv::putText(image, name, p1, cv::FONT_HERSHEY_SIMPLEX, 1, color, 2);
#else
      draw_rect(image, int(b.xyxy[0]), int(b.xyxy[1]), int(b.xyxy[2]), int(b.xyxy[3]), blue ? 0 : 255, 0, blue ? 255 : 0);
      draw_label(image, name, int(b.xyxy[0]), int(b.xyxy[1]), blue ? 0 : 255, 0, blue ? 255 : 0);
#endif
    }
  }

  double get_profiling_time() const { return enable_profiling_ ? irmv_engine_last_detect_ms(engine_) : 0.0; }

  const cv::Mat & get_rotated_image() const
  {
    if (!rotated_valid_) {
      if (irmv_engine_rotated_image(engine_, 0, rotated_.data) != IRMV_OK)
        throw std::runtime_error(std::string("YoloEngine::get_rotated_image: ") + irmv_last_error());
      rotated_valid_ = true;
    }
    return rotated_;
  }

  // The node's debug images (src/irm_detector.cpp:259-280), rendered on the GPU from the frame of the last detect() -- a Bayer
  // engine's demosaiced frame, a window engine's window (View::Frame: the whole frame): kind IRMV_RENDER_COLOR is the frame,
  // IRMV_RENDER_BINARY gray > binary_threshold on three channels (-1: the threshold set with set_extract_params); scale 1, 2
  // or 4 shrinks it for a radio link; marks (IRMV_MARK_BOXES | _LABELS | _ARMORS) of `dets` are drawn on it, nullptr = the
  // last detect()'s own records.  Only the finished CV_8UC3 picture crosses PCIe (include/irmv_hip.h, "debug images").  The
  // drawing is this project's own rasteriser and 5 x 7 font, not OpenCV's: at scale 1 boxes and labels are the pixels
  // visualize_bboxes draws without OpenCV.
  cv::Mat render(int kind = IRMV_RENDER_COLOR, int scale = 1, uint32_t marks = IRMV_MARK_BOXES | IRMV_MARK_LABELS | IRMV_MARK_ARMORS,
                 const std::vector<irmv_det> * dets = nullptr, int binary_threshold = -1)
  {
    irmv_render_opts o{};
    o.struct_size = sizeof o;
    o.kind = kind;
    o.scale = scale;
    o.marks = marks;
    o.binary_threshold = binary_threshold;
    int w = 0, h = 0;
    if (irmv_engine_render_dims(engine_, 0, scale, &w, &h) != IRMV_OK) throw std::runtime_error(std::string("YoloEngine::render: ") + irmv_last_error());
    cv::Mat out(h, w, CV_8UC3);
    if (irmv_engine_render(engine_, 0, &o, dets ? dets->data() : nullptr, dets ? static_cast<int>(dets->size()) : -1, out.data) != IRMV_OK)
      throw std::runtime_error(std::string("YoloEngine::render: ") + irmv_last_error());
    return out;
  }

  size_t max_det() const { return dets_.size(); }

  uint8_t * get_src_image_buffer() const { return src_image_buffer_; }
  // bytes a producer writes into get_src_image_buffer() per frame: width * height * 3 (HWC8) or width * height (Bayer)
  size_t src_image_bytes() const { return irmv_engine_src_bytes(engine_); }

private:
  static void draw_rect(cv::Mat & img, int x1, int y1, int x2, int y2, int c0, int c1, int c2)
  {
    auto put = [&](int x, int y) {
      if (x < 0 || y < 0 || x >= img.cols || y >= img.rows) return;
      uint8_t * p = img.data + (size_t(y) * img.cols + x) * 3;
      p[0] = uint8_t(c0); p[1] = uint8_t(c1); p[2] = uint8_t(c2);
    };
    for (int t = 0; t < 2; t++) {
      for (int x = x1; x <= x2; x++) { put(x, y1 + t); put(x, y2 - t); }
      for (int y = y1; y <= y2; y++) { put(x1 + t, y); put(x2 - t, y); }
    }
  }

  // Class label without OpenCV: the ArmorClass names (B1..B5, BO, BS, R1..R5, RO, RS, UNKNOWN) in a 5 x 7 bitmap font at
  // scale 3 (glyphs 15 x 21 px, 18 px advance: the size of FONT_HERSHEY_SIMPLEX at scale 1), text origin = bottom-left
  // corner at (x, y) like cv::putText (src/yolo_engine.cpp:238-241).
  // The glyphs are the library's (irmv_render_glyph): the table the GPU's debug images are drawn from.
  static void draw_label(cv::Mat & img, const std::string & text, int x, int y, int c0, int c1, int c2)
  {
    constexpr int S = 3;
    for (size_t k = 0; k < text.size(); k++) {
      uint8_t g[7];
      if (irmv_render_glyph(text[k], g) != IRMV_OK) continue;
      for (int r = 0; r < 7; r++)
        for (int c = 0; c < 5; c++) {
          if (!((g[r] >> (4 - c)) & 1)) continue;
          for (int dy = 0; dy < S; dy++)
            for (int dx = 0; dx < S; dx++) {
              const int px = x + int(k) * 6 * S + c * S + dx, py = y - 7 * S + r * S + dy;
              if (px < 0 || py < 0 || px >= img.cols || py >= img.rows) continue;
              uint8_t * p = img.data + (size_t(py) * img.cols + px) * 3;
              p[0] = uint8_t(c0); p[1] = uint8_t(c1); p[2] = uint8_t(c2);
            }
        }
    }
  }

  irmv_engine * engine_ = nullptr;
  // Slot 0's side records of one kind, parallel to last_detections(): empty until the feature's first set (`on`), then what
  // the library's call `get` delivers; `who` names the caller in a thrown error.
  template <typename R>
  std::vector<R> side_records(bool on, int (*get)(irmv_engine *, int, R *, int, int *), const char * who) const
  {
    std::vector<R> a;
    if (!on) return a;
    a.resize(dets_.size());
    int n = 0;
    if (get(engine_, 0, a.data(), static_cast<int>(a.size()), &n) != IRMV_OK)
      throw std::runtime_error(std::string("YoloEngine::") + who + ": " + irmv_last_error());
    a.resize(static_cast<size_t>(n));
    return a;
  }
  // caller's policy + colour -> one table upload; on a refusal nothing is stored
  void apply_class_policy(const irmv_class_policy & p, int enemy_color, const char * who)
  {
    irmv_class_policy mask, eff = p;
    if (irmv_class_policy_enemy(enemy_color, 0.5f, IRMV_ARMOR_SMALL, &mask) != IRMV_OK) throw std::runtime_error(std::string(who) + irmv_last_error());
    for (int c = 0; c < 16; c++)
      if (mask.score_thr[c] >= 1.f) eff.score_thr[c] = 1.f;   // the own colour's classes, as irmv_class_policy_enemy names them
    if (irmv_engine_set_class_policy(engine_, &eff) != IRMV_OK) throw std::runtime_error(std::string(who) + irmv_last_error());
    user_policy_ = p;
    enemy_color_ = enemy_color;
  }

  irmv_class_policy base_policy_{};   // the uniform policy the engine was created with
  irmv_class_policy user_policy_{};   // the caller's thresholds and plates, without the colour mask
  int enemy_color_ = -1;
  bool pose_alts_on_ = false;         // set_pose_prior has been called: the engine delivers alt records
  bool yaw_on_ = false;               // set_yaw_solve has been called: the engine delivers constrained poses
  bool pose_cov_on_ = false;          // set_pose_cov has been called: the engine delivers pose covariances
  bool tracking_on_ = false;          // set_tracking has been called: the engine delivers track records
  bool patches_on_ = false;           // set_patches has been called: the engine delivers plate patches
  bool numbers_on_ = false;           // set_numbers(true) has been called: the engine delivers plate numbers
  cv::Size src_image_size_;
  cv::Size window_size_;
  bool enable_profiling_ = false;
  uint8_t * src_image_buffer_ = nullptr;
  mutable cv::Mat rotated_;
  mutable bool rotated_valid_ = false;
  std::vector<irmv_det> dets_;
  int n_last_ = 0;
  std::vector<irmv_tile_det> tile_dets_;   // detect_tiles()
  int num_tiles_ = 0, n_last_tiles_ = 0;
  cv::Size tile_grid_{0, 0};
};
}  // namespace irmv_detection
