// irmv_detection::IrmDetectorCore -- the ROS-free body of the reference's detector node
// (reference src/irm_detector.cpp): what IrmDetector::IrmDetector (:25-78) builds and what
// IrmDetector::message_callback (:176-245) computes per frame, with every rclcpp / cv_bridge /
// tf2 / auto_aim_interfaces type replaced by a plain struct of the same fields, so that the
// hot path of the node compiles and is tested without a ROS2 installation.  The optional ROS2
// target (ros2/irm_detector_node.cpp, built only where ament_cmake is found) is a thin shell
// around this class: it copies ArmorsMsg into auto_aim_interfaces::msg::Armors and publishes.
//
//   frame in slot `id`  ->  YoloEngine::detect()                        (:181)
//                       ->  extract_armors(get_rotated_image(), bboxes) (:183, :292-355)  [GPU]
//                       ->  per armor: solvePnP (IPPE, small armor)      (:204-209)        [GPU, fused]
//                           Rodrigues -> rotation matrix -> quaternion   (:218-226)        [GPU, fused]
//                           distance_to_image_center                     (:229)
//                       ->  ArmorsMsg                                    (:245 publishes it)
//
// Two sources of the four armor points, like the engine (irmv_hip.h, point_source): a pose-style
// model carries them in its keypoint head (then every detection is an armor); a bbox-only model
// gets them from the reference's classical light extraction, run on the GPU.  Either way the pose
// arrives with the detection: no per-armor host round trip.
#pragma once

#include <array>
#include <chrono>
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "irmv_detection/armor.hpp"
#include "irmv_detection/pnp_solver.hpp"
#include "irmv_detection/tracker.hpp"
#include "irmv_detection/yolo_engine.hpp"

namespace irmv_detection
{
// geometry_msgs::msg::Pose
struct PoseMsg
{
  struct { double x = 0, y = 0, z = 0; } position;
  struct { double x = 0, y = 0, z = 0, w = 1; } orientation;
};

// auto_aim_interfaces::msg::Armor (string number, string type, float32 distance_to_image_center,
// geometry_msgs/Pose pose).  Like the reference (:211-230) only the pose and the distance are filled;
// `number` / `type` stay empty there too.  armor_class / size ride along for consumers that want them.
struct ArmorMsg
{
  std::string number;
  std::string type;
  float distance_to_image_center = 0.f;
  PoseMsg pose;
  ArmorClass armor_class = ArmorClass::UNKNOWN;   // extension (not a field of the ROS message)
  ArmorSize size = ArmorSize::SMALL;              // extension
};

// auto_aim_interfaces::msg::Armors: std_msgs/Header + Armor[]
struct ArmorsMsg
{
  struct
  {
    int64_t stamp_ns = 0;                          // image.time_stamp.time_since_epoch() (:194)
    std::string frame_id = "camera_optical_frame"; // :197
  } header;
  std::vector<ArmorMsg> armors;
};

// Camera::StampedImage without the cv::Mat (the pixels already sit in engine slot `id`,
// reference include/irmv_detection/camera.hpp:27-32, src/camera.cpp:24-29)
struct StampedFrame
{
  std::chrono::time_point<std::chrono::system_clock> time_stamp{};
  int id = 0;
};

class IrmDetectorCore
{
public:
  // The node's parameters that reach the hot path (src/irm_detector.cpp:122-174)
  struct Params
  {
    cv::Size image_input_size = cv::Size(1280, 1024);   // camera frame size (:140-144)
    bool profiling = false;
    int binary_threshold = 150;
    double light_min_ratio = 0.1, light_max_ratio = 0.4, light_max_angle = 40.0;
    double armor_min_small_center_distance = 0.8, armor_max_small_center_distance = 3.2;
    double armor_min_large_center_distance = 3.2, armor_max_large_center_distance = 5.5;
    int device = -1;                                     // HIP device; -1: IRMV_DEVICE or 0
    cv::Size net_input_size{0, 0};                       // network input width x height; 0: the engine's default (square);
                                                         // height 0: square of the width (1280 x 1024 camera: 640 x 512)
    cv::Size window_size{0, 0};                          // tracking window of the three engines (YoloEngine's `window`); 0: none.  No policy here:
                                                         // the caller moves each engine's window (engine(id).set_window_center(...))
    cv::Size tile_overlap{-1, -1};                       // tiled search of the three engines (YoloEngine's `tile_overlap`; needs window_size): the least overlap
                                                         // of neighbouring tiles; negative: off.  engine(id).detect_tiles() then searches the frame in its buffer
    int enemy_color = -1;                                // the node's enemy_color (:154-160, "0 for blue, 1 for red"): 0 keeps B1..BS, 1 keeps R1..RS,
                                                         // on the GPU where candidates are emitted; -1: no filter (what the reference's unused parameter amounts to)
    std::vector<int> large_plate_classes;                // ArmorClass values whose detections PnP solves with the 225 mm plate; the rest: 135 mm
    int point_source = IRMV_POINTS_AUTO;                 // IRMV_POINTS_*; IRMV_POINTS_REFINED: a pose model's points snapped to the light bars, inside the step
    double refine_snap = 0.5, refine_roi_margin = 4.0;   // its two live parameters (irmv_engine_set_refine; set_parameter "refine.snap" / "refine.roi_margin")
    // Pose ambiguity (include/irmv_hip.h): struct_size != 0 enables it on the three engines at creation -- FrameResult::alts is
    // then filled, and mode IRMV_POSE_PRIOR lets the tilt prior choose.  Live: set_parameter "pose_prior" (the mode; enables),
    // "pose_prior.ratio", "pose_prior.normal_up" (every class), and "up.x" / "up.y" / "up.z" or set_up() for the gimbal's up vector.
    irmv_pose_prior pose_prior{};
    std::array<double, 3> up{0.0, -1.0, 0.0};
    // Constrained pose (include/irmv_hip.h): struct_size != 0 enables it on the three engines at creation (YoloEngine::yaw_opts())
    // -- FrameResult::yaw is then filled.  yaw_publish: the message carries the constrained pose in place of IPPE's wherever
    // its state is 1.  Live: set_parameter "yaw_solve" (0 | 1; the first 1 enables), "yaw_publish" (0 | 1).
    // Models with a keypoint head only (a refined engine is one), like FrameResult::alts: a bbox-only detector takes its armors
    // from extract_armors() -- explicit boxes, which have no side records --, so FrameResult::yaw stays empty there and
    // yaw_publish changes nothing.
    irmv_yaw_opts yaw_solve{};
    bool yaw_publish = false;
    // Pose uncertainty (include/irmv_hip.h): pose_cov enables it on the three engines at creation with corner noise sigma_px
    // (pixels, in (0, 64]) -- FrameResult::covs is then filled.  Live: set_parameter "pose_cov" (0 | 1; the first 1 enables),
    // "sigma_px".  Models with a keypoint head only, like FrameResult::yaw.
    bool pose_cov = false;
    double sigma_px = 1.0;
    // Armor tracks (include/irmv_hip.h): struct_size != 0 (ArmorTracker::default_opts()) gives the detector ONE tracker, fed with
    // every frame's poses in frame order -- the three engines each see every third frame, so none of them could keep the
    // table -- and with their covariances where `pose_cov` is on; FrameResult::det_tracks / tracks are then filled, stamped
    // from the frame's time stamp.  The camera pose in the world comes from set_camera_pose() (default identity).  The
    // tracker's measurement is always the IPPE translation of FrameResult::poses, also where `yaw_publish` puts the constrained
    // pose into the message: the covariance it takes from `pose_cov` is that pose's.  Live:
    // set_parameter "tracking" (0 | 1: 0 drops the tracker and its table, 1 starts an empty one).
    irmv_track_opts tracking{};
    // Plate patches (include/irmv_hip.h): struct_size != 0 enables them on the three engines at creation
    // (YoloEngine::patch_opts()) -- FrameResult::patches is then filled.  Live: set_parameter "patches" (0 | 1; the first 1
    // enables).  Models with a keypoint head only, like FrameResult::yaw.
    irmv_patch_opts patches{};
    // Plate numbers (include/irmv_hip.h): the path of an .irmn model file, empty = off.  The three engines load it at creation
    // and read every plate patch with it (the patches are turned on with their defaults where `patches` did not) --
    // FrameResult::numbers is then filled.  Live: set_parameter("number_model", path); an empty path switches the records off.
    std::string number_model;
    bool debug = false;                                  // the node's debug (:90-95, :259-280): every frame also yields FrameResult::visualized_image / binary_image,
                                                         // rendered on the GPU (YoloEngine::render); live through set_bool_parameter("debug", v) like the reference (:380-381)
    int debug_scale = 1;                                 // 1, 2 or 4: the debug images at full, half or quarter size (set_parameter "debug_scale")
    int src_format = IRMV_SRC_HWC8;                      // IRMV_SRC_*: a Bayer format makes image_buffers() raw CFA frames, demosaiced on the GPU
    // Frame metering (include/irmv_hip.h): struct_size != 0 enables it on the three engines at creation (YoloEngine::meter_opts
    // fills one) -- FrameResult::stats is then each frame's record.
    irmv_meter_opts metering{};
    // Automatic white balance: every awb_period-th frame the gains irmv_stats_gray_world(lo = 8, hi = 247) reads from that
    // frame's record go to all three engines (set_bayer_isp, the tone LUT kept); a record the helper refuses leaves the gains
    // alone.  0: off.  Needs Bayer engines and IRMV_METER_RAW metering -- white balance must look in front of its own gains --,
    // else the constructor throws and set_parameter("awb_period", v) refuses.  Live: set_parameter "awb_period".
    int awb_period = 0;
  };

  // What one frame produced, beyond the message: kept for debug publishers and tests.
  struct FrameResult
  {
    ArmorsMsg armors_msg;
    std::vector<YoloEngine::bbox> bboxes;
    std::vector<Armor> armors;          // one per message entry, same order
    std::vector<irmv_det> poses;        // rvec / tvec / quaternion of each, as computed on the GPU
    // Pose ambiguity enabled and a pose-style model: per entry of `poses` the IPPE solution it does NOT report, with
    // err / err_alt, the rms normalised residuals of the reported pose and of this one (else empty).  A tracker keeps both
    // while err_alt / err is small and lets its motion model decide; a large ratio means the reported pose stands alone.
    std::vector<irmv_pose_alt> alts;
    // Params::yaw_solve only (else empty): parallel to `poses`, the plate's pose with its yaw solved at the class's known tilt
    // and the up vector (state 1; -1: refused, 0: nothing)
    std::vector<irmv_yaw_pose> yaw;
    // Params::pose_cov only (else empty): parallel to `poses`, the first-order covariance of each armor's pose -- and, where
    // `yaw` is filled, of its constrained pose -- under Params::sigma_px of corner noise (state 1; -1: refused, 0: nothing)
    std::vector<irmv_pose_cov> covs;
    // Params::patches only (else empty): parallel to `poses`, each armor's rectified 20 x 28 gray number image, its Otsu
    // threshold and the colour vote of its two light bars (state 1; 0: no patch)
    std::vector<irmv_plate_patch> patches;
    // Params::number_model only (else empty): parallel to `poses`, the MLP's reading of each armor's patch -- label, runner-up,
    // margin, logits (state 1; 0: no answer, exactly where the patch has none)
    std::vector<irmv_plate_number> numbers;
    // Params::tracking only (else empty / state 0): parallel to `poses`, what the tracker made of each armor -- id, hits, filtered
    // position and velocity in the world frame --, the frame's header and the whole table (IRMV_TRACK_CAP entries, coasting
    // tracks included; irmv_track_predict extrapolates one)
    std::vector<irmv_det_track> det_tracks;
    irmv_track_frame track_frame{};
    std::vector<irmv_track> tracks;
    double inference_latency_ms = 0;    // YoloEngine::get_profiling_time() (:251)
    // Params::debug only (else empty): the frame with this frame's armors, boxes and labels drawn on it (:261-263; the latency
    // text lines are not drawn), and gray -> threshold(binary_threshold) -> three channels with the boxes and labels (:273-277)
    cv::Mat visualized_image, binary_image;
    // Params::metering only (else stats_valid = false): this frame's metering record; awb_applied: this frame's record set new
    // white-balance gains, awb_gains, which hold from the next frame on
    irmv_frame_stats stats{};
    bool stats_valid = false, awb_applied = false;
    std::array<uint16_t, 3> awb_gains{256, 256, 256};
  };

  // Three engines, one per TripleBuffer slot, like the node (:33-38); K, D from camera_info (:52).
  IrmDetectorCore(const std::string & model_path, const std::array<double, 9> & k, const std::vector<double> & d, const Params & p)
  : params_(p)
  {
    if (p.awb_period < 0 || (p.awb_period > 0 && !awb_possible(p)))
      throw std::invalid_argument("IrmDetectorCore: awb_period needs a Bayer src_format and IRMV_METER_RAW metering");
    for (auto & e : yolo_engines_) {
      e = std::make_unique<YoloEngine>(model_path, p.image_input_size, p.profiling, p.device, false, p.net_input_size.width > 0 ? p.net_input_size.width : -1,
                                       p.src_format, std::array<uint16_t, 3>{256, 256, 256}, p.net_input_size.height > 0 ? p.net_input_size.height : -1,
                                       IRMV_DEMOSAIC_BILINEAR, p.window_size, p.tile_overlap, p.point_source);
      if (p.metering.struct_size != 0) e->set_metering(&p.metering);
      push_params(*e);
      if (p.refine_snap != 0.5 || p.refine_roi_margin != 4.0) e->set_refine(float(p.refine_snap), float(p.refine_roi_margin));
      if (p.enemy_color != -1 || !p.large_plate_classes.empty()) push_class_policy(*e);
      if (p.pose_prior.struct_size != 0) { e->set_pose_prior(&p.pose_prior); e->set_up(p.up); }
      if (p.yaw_solve.struct_size != 0) { e->set_yaw_solve(p.yaw_solve); e->set_up(p.up); }
      if (p.pose_cov) e->set_pose_cov(YoloEngine::pose_cov_opts(true, p.sigma_px));
      if (p.patches.struct_size != 0) e->set_patches(p.patches);
      if (!p.number_model.empty()) { e->set_number_model(p.number_model); e->set_numbers(true); }
    }
    yolo_engines_[0]->warm_up();   // the tile choices are shared by the three engines: one warm-up tunes for all
    for (size_t i = 1; i < yolo_engines_.size(); i++) yolo_engines_[i]->warm_up();
    pnp_solver_ = std::make_unique<PnPSolver>(k, d, p.device);
    if (p.tracking.struct_size != 0 && p.tracking.enable) tracker_ = std::make_unique<ArmorTracker>(p.tracking, p.device);
  }

  // Camera::Config::image_buffers (:68-72): where the producer deposits frames
  std::array<uint8_t *, 3> image_buffers() const
  {
    return {yolo_engines_[0]->get_src_image_buffer(), yolo_engines_[1]->get_src_image_buffer(), yolo_engines_[2]->get_src_image_buffer()};
  }

  YoloEngine & engine(int id) { return *yolo_engines_[size_t(id)]; }
  const PnPSolver & pnp_solver() const { return *pnp_solver_; }

  // IrmDetector::message_callback without the publishers (:176-245)
  FrameResult message_callback(const StampedFrame & image)
  {
    FrameResult out;
    YoloEngine & eng = *yolo_engines_[size_t(image.id)];
    out.bboxes = eng.detect();
    out.armors_msg.header.stamp_ns = std::chrono::duration_cast<std::chrono::nanoseconds>(image.time_stamp.time_since_epoch()).count();

    std::vector<Armor> armors;
    std::vector<irmv_det> poses;
    std::vector<irmv_pose_alt> alts;
    std::vector<irmv_yaw_pose> yaws;
    std::vector<irmv_pose_cov> covs;
    std::vector<irmv_plate_patch> plates;
    std::vector<irmv_plate_number> numbers;
    if (eng.has_keypoint_head()) {
      // pose-style model: each detection carries its four points and, already, its pose
      int n = 0;
      const irmv_det * dets = eng.last_detections(&n);
      const std::vector<irmv_pose_alt> all = eng.pose_alts();   // parallel to dets (empty: not enabled)
      const std::vector<irmv_yaw_pose> all_yaw = eng.yaw_poses();
      const std::vector<irmv_pose_cov> all_covs = eng.pose_covs();
      const std::vector<irmv_plate_patch> all_plates = eng.plate_patches();
      const std::vector<irmv_plate_number> all_numbers = eng.plate_numbers();
      for (int i = 0; i < n; i++) {
        const irmv_det & d = dets[i];
        if (d.armor_valid != 1) continue;
        if (size_t(i) < all.size()) alts.push_back(all[size_t(i)]);
        if (size_t(i) < all_yaw.size()) yaws.push_back(all_yaw[size_t(i)]);
        if (size_t(i) < all_covs.size()) covs.push_back(all_covs[size_t(i)]);
        if (size_t(i) < all_plates.size()) plates.push_back(all_plates[size_t(i)]);
        if (size_t(i) < all_numbers.size()) numbers.push_back(all_numbers[size_t(i)]);
        Armor a(Light(cv::Point2f(d.kpts[2], d.kpts[3]), cv::Point2f(d.kpts[0], d.kpts[1])),
                Light(cv::Point2f(d.kpts[4], d.kpts[5]), cv::Point2f(d.kpts[6], d.kpts[7])));
        a.armor_class = static_cast<ArmorClass>(d.class_id);
        a.confidence = d.score;
        a.size = d.armor_size == IRMV_ARMOR_LARGE ? ArmorSize::LARGE : ArmorSize::SMALL;
        armors.push_back(a);
        poses.push_back(d);
      }
    } else {
      armors = eng.extract_armors(out.bboxes, &poses);   // :183, on the GPU, poses included
    }

    for (size_t i = 0; i < armors.size(); i++) {
      const irmv_det & d = poses[i];
      if (!d.pnp_ok) continue;                             // `if (!pnp_solver_->solvePnP(...)) continue;` (:207-209)
      ArmorMsg m;
      m.pose.position.x = d.tvec[0];                       // :214-216
      m.pose.position.y = d.tvec[1];
      m.pose.position.z = d.tvec[2];
      m.pose.orientation.x = d.quat[0];                    // Rodrigues -> tf2::Matrix3x3::getRotation (:218-226)
      m.pose.orientation.y = d.quat[1];
      m.pose.orientation.z = d.quat[2];
      m.pose.orientation.w = d.quat[3];
      m.distance_to_image_center = pnp_solver_->calculateDistanceToCenter(armors[i].center);   // :229
      m.armor_class = armors[i].armor_class;
      m.size = armors[i].size;
      out.armors_msg.armors.push_back(m);
      out.armors.push_back(armors[i]);
      out.poses.push_back(d);
      if (alts.size() == armors.size()) out.alts.push_back(alts[i]);
      if (covs.size() == armors.size()) out.covs.push_back(covs[i]);
      if (plates.size() == armors.size()) out.patches.push_back(plates[i]);
      if (numbers.size() == armors.size()) out.numbers.push_back(numbers[i]);
      if (yaws.size() == armors.size()) {
        out.yaw.push_back(yaws[i]);
        if (params_.yaw_publish && yaws[i].state == 1) {     // the constrained pose in place of IPPE's
          ArmorMsg & pm = out.armors_msg.armors.back();
          pm.pose.position.x = yaws[i].tvec[0]; pm.pose.position.y = yaws[i].tvec[1]; pm.pose.position.z = yaws[i].tvec[2];
          pm.pose.orientation.x = yaws[i].quat[0]; pm.pose.orientation.y = yaws[i].quat[1];
          pm.pose.orientation.z = yaws[i].quat[2]; pm.pose.orientation.w = yaws[i].quat[3];
        }
      }
    }
    if (tracker_) {
      // one frame of the tracker: the armors of the message, in its order, at the frame's stamp relative to the first frame's
      // (seconds since the epoch would leave a double 2e-7 s of resolution)
      const int64_t ns = out.armors_msg.header.stamp_ns;
      if (!track_epoch_set_) { track_epoch_ns_ = ns; track_epoch_set_ = true; }
      std::vector<irmv_track_obs> obs;
      for (size_t i = 0; i < out.poses.size(); i++)
        obs.push_back(ArmorTracker::observation(out.poses[i], out.covs.size() == out.poses.size() ? &out.covs[i] : nullptr));
      ArmorTracker::Result r = tracker_->update(double(ns - track_epoch_ns_) * 1e-9, obs, &cam_R_, &cam_t_);
      out.det_tracks = std::move(r.det_tracks);
      out.track_frame = r.frame;
      out.tracks = std::move(r.tracks);
    }
    out.inference_latency_ms = eng.get_profiling_time();
    if (params_.metering.struct_size != 0) {
      out.stats = eng.frame_stats();
      out.stats_valid = true;
      if (params_.awb_period > 0 && ++awb_frames_ % uint64_t(params_.awb_period) == 0) {
        std::vector<uint8_t> lut;
        std::array<uint16_t, 3> g = eng.bayer_gains(&lut);
        if (irmv_stats_gray_world(&out.stats, 8, 247, g.data()) == IRMV_OK) {   // (refused: g is untouched, and nothing is set)
          for (auto & e : yolo_engines_) e->set_bayer_isp(g, lut.data());
          out.awb_applied = true;
          out.awb_gains = g;
        }
      }
    }
    if (params_.debug) {
      // the marks: every bbox (:263, :277) and every extracted armor (:262) -- of a pose model both live in the detection
      // records; of a bbox-only model the armors are records of their own whose box is no number, so it draws none
      std::vector<irmv_det> marks;
      if (eng.has_keypoint_head()) {
        int n = 0;
        const irmv_det * dets = eng.last_detections(&n);
        marks.assign(dets, dets + n);
      } else {
        for (const auto & b : out.bboxes) {
          irmv_det m{};
          std::copy(b.xyxy.begin(), b.xyxy.end(), m.xyxy);
          m.class_id = static_cast<int32_t>(b.class_id);
          marks.push_back(m);
        }
        for (irmv_det m : poses) {
          std::fill(m.xyxy, m.xyxy + 4, std::nanf(""));
          marks.push_back(m);
        }
        if (marks.size() > eng.max_det()) marks.resize(eng.max_det());   // (boxes first: the armors' marks are what is dropped)
      }
      out.visualized_image = eng.render(IRMV_RENDER_COLOR, params_.debug_scale, IRMV_MARK_BOXES | IRMV_MARK_LABELS | IRMV_MARK_ARMORS, &marks);
      out.binary_image = eng.render(IRMV_RENDER_BINARY, params_.debug_scale, IRMV_MARK_BOXES | IRMV_MARK_LABELS, &marks);
    }
    return out;
  }

  // IrmDetector::param_event_callback (:372-403): returns false for a name that is not a hot-path parameter
  bool set_parameter(const std::string & name, double value)
  {
    if (name == "binary_threshold") params_.binary_threshold = int(value);
    else if (name == "light.min_ratio") params_.light_min_ratio = value;
    else if (name == "light.max_ratio") params_.light_max_ratio = value;
    else if (name == "light.max_angle") params_.light_max_angle = value;
    else if (name == "armor.min_small_center_distance") params_.armor_min_small_center_distance = value;
    else if (name == "armor.max_small_center_distance") params_.armor_max_small_center_distance = value;
    else if (name == "armor.min_large_center_distance") params_.armor_min_large_center_distance = value;
    else if (name == "armor.max_large_center_distance") params_.armor_max_large_center_distance = value;
    else if (name == "debug_scale") {                      // live: the next frame's debug images have that size
      const int sc = int(value);
      if (sc != 1 && sc != 2 && sc != 4) return false;
      params_.debug_scale = sc;
      return true;
    }
    else if (name == "awb_period") {                       // live; refused without Bayer engines and IRMV_METER_RAW metering
      const int n = int(value);
      if (n < 0 || double(n) != value || (n > 0 && !awb_possible(params_))) return false;
      params_.awb_period = n;
      return true;
    }
    else if (name == "enemy_color") {                      // :384-385; live, and re-captures nothing
      const int c = int(value);
      if (c < -1 || c > 1) return false;
      params_.enemy_color = c;
      for (auto & e : yolo_engines_) e->set_enemy_color(c);   // (thresholds and plates set on an engine(id) stay)
      return true;
    }
    else if (name == "refine.snap" || name == "refine.roi_margin") {   // live, and re-captures nothing
      const double snap = name == "refine.snap" ? value : params_.refine_snap, margin = name == "refine.roi_margin" ? value : params_.refine_roi_margin;
      if (!(snap > 0.0 && snap <= 4.0) || !(margin >= 0.0 && margin <= 64.0)) return false;
      params_.refine_snap = snap; params_.refine_roi_margin = margin;
      for (auto & e : yolo_engines_) e->set_refine(float(snap), float(margin));
      return true;
    }
    else if (name == "yaw_solve") {
      // live; the first 1 enables the records (one re-capture per engine), later ones re-capture nothing
      if (value != 0.0 && value != 1.0) return false;
      if (value == 0.0 && params_.yaw_solve.struct_size == 0) return true;
      irmv_yaw_opts o = params_.yaw_solve.struct_size ? params_.yaw_solve : YoloEngine::yaw_opts();
      o.enable = int(value);
      params_.yaw_solve = o;
      for (auto & e : yolo_engines_) { e->set_yaw_solve(o); e->set_up(params_.up); }
      return true;
    }
    else if (name == "pose_cov" || name == "sigma_px") {
      // live; the first pose_cov = 1 enables the records (one re-capture per engine), later calls re-capture nothing
      const bool on = name == "pose_cov" ? value == 1.0 : params_.pose_cov;
      const double sigma = name == "sigma_px" ? value : params_.sigma_px;
      if (name == "pose_cov" && value != 0.0 && value != 1.0) return false;
      if (!(sigma > 0.0 && sigma <= 64.0)) return false;
      if (on || params_.pose_cov)
        for (auto & e : yolo_engines_) e->set_pose_cov(YoloEngine::pose_cov_opts(on, sigma));
      params_.pose_cov = on;
      params_.sigma_px = sigma;
      return true;
    }
    else if (name == "patches") {
      // live; the first 1 enables the records (one re-capture per engine), later ones re-capture nothing
      if (value != 0.0 && value != 1.0) return false;
      if (value == 0.0 && params_.patches.struct_size == 0) return true;
      irmv_patch_opts o = params_.patches.struct_size ? params_.patches : YoloEngine::patch_opts();
      o.enable = int(value);
      params_.patches = o;
      for (auto & e : yolo_engines_) e->set_patches(o);
      return true;
    }
    else if (name == "tracking") {
      // live; 1 starts a tracker with an empty table (ids from 1), 0 drops it
      if (value != 0.0 && value != 1.0) return false;
      if (value == 1.0 && !tracker_) {
        irmv_track_opts o = params_.tracking.struct_size ? params_.tracking : ArmorTracker::default_opts();
        o.enable = 1;
        tracker_ = std::make_unique<ArmorTracker>(o, params_.device);
        params_.tracking = o;
      } else if (value == 0.0) {
        tracker_.reset();
        track_epoch_set_ = false;
        if (params_.tracking.struct_size) params_.tracking.enable = 0;
      }
      return true;
    }
    else if (name == "yaw_publish") {
      if (value != 0.0 && value != 1.0) return false;
      params_.yaw_publish = value == 1.0;
      return true;
    }
    else if (name == "pose_prior" || name == "pose_prior.ratio" || name == "pose_prior.normal_up") {
      // live; the first one enables the alt records (one re-capture per engine), later ones re-capture nothing
      irmv_pose_prior p = params_.pose_prior.struct_size ? params_.pose_prior : yolo_engines_[0]->pose_prior();
      if (name == "pose_prior") {
        if (value != double(IRMV_POSE_MIN_ERR) && value != double(IRMV_POSE_PRIOR)) return false;
        p.mode = int(value);
      } else if (name == "pose_prior.ratio") {
        if (!(value >= 1.0)) return false;
        p.ambiguity_ratio = value;
      } else {
        if (!(std::fabs(value) <= 1.0)) return false;
        for (double & s : p.normal_up) s = value;
        p.normal_up_default = value;
      }
      params_.pose_prior = p;
      for (auto & e : yolo_engines_) e->set_pose_prior(&p);
      return true;
    }
    else if (name == "up.x" || name == "up.y" || name == "up.z") {   // one component; set_up() takes the whole vector
      std::array<double, 3> u = params_.up;
      u[size_t(name[3] - 'x')] = value;
      return set_up(u);
    }
    else return false;
    for (auto & e : yolo_engines_) push_params(*e);
    return true;
  }

  // The node's string parameters: "number_model" is live -- a path loads that .irmn file into the three engines and switches
  // the number records on (the first time: one re-capture per engine), an empty path switches them off.  false, and nothing
  // changed on the engines that refused, for a file that cannot be read or a model that is refused.
  bool set_parameter(const std::string & name, const std::string & value)
  {
    if (name != "number_model") return false;
    try {
      for (auto & e : yolo_engines_) {
        if (!value.empty()) e->set_number_model(value);
        if (!value.empty() || !params_.number_model.empty()) e->set_numbers(!value.empty());
      }
    } catch (const std::exception &) {
      return false;
    }
    params_.number_model = value;
    return true;
  }

  // The gimbal's up vector in the camera frame (any length), for the frames to come: false for a zero or non-finite vector
  bool set_up(const std::array<double, 3> & up)
  {
    const double n2 = (up[0] * up[0] + up[1] * up[1]) + up[2] * up[2];
    if (!(n2 > 0.0 && std::isfinite(n2))) return false;
    params_.up = up;
    for (auto & e : yolo_engines_) e->set_up(up);
    return true;
  }

  // The camera's pose in the world (R_wc row-major, t_wc) for the frames to come: what the tracker turns each armor's tvec
  // into a world position with.  false for a value that is not finite.
  bool set_camera_pose(const std::array<double, 9> & R_wc, const std::array<double, 3> & t_wc)
  {
    for (double v : R_wc) if (!std::isfinite(v)) return false;
    for (double v : t_wc) if (!std::isfinite(v)) return false;
    cam_R_ = R_wc;
    cam_t_ = t_wc;
    return true;
  }

  // The node's bool parameters (parameter.as_bool(), :380-381): "debug" is live -- the next frame carries, or drops, the two
  // debug images.  (A NUMBER sent to "debug" through set_parameter stays refused, as it is not a number.)
  bool set_bool_parameter(const std::string & name, bool value)
  {
    if (name != "debug") return false;
    params_.debug = value;
    return true;
  }

  const Params & params() const { return params_; }

private:
  static bool awb_possible(const Params & p)
  {
    return p.src_format != IRMV_SRC_HWC8 && p.metering.struct_size != 0 && p.metering.domain == IRMV_METER_RAW;
  }

  void push_params(YoloEngine & e) const
  {
    e.set_extract_params(params_.binary_threshold, float(params_.light_min_ratio), float(params_.light_max_ratio), float(params_.light_max_angle),
                         params_.armor_min_small_center_distance, params_.armor_max_small_center_distance,
                         params_.armor_min_large_center_distance, params_.armor_max_large_center_distance);
  }

  // enemy_color and large_plate_classes -> the engine's class policy, built once and uploaded once.  Nothing is sent while
  // both are at their defaults.
  void push_class_policy(YoloEngine & e) const
  {
    irmv_class_policy p = e.user_class_policy();
    for (int c : params_.large_plate_classes)
      if (c >= 0 && c < 16) p.plate[c] = IRMV_ARMOR_LARGE;
    e.set_class_policy(p, params_.enemy_color);
  }

  Params params_;
  uint64_t awb_frames_ = 0;   // frames since creation, counted while awb_period is on
  std::array<std::unique_ptr<YoloEngine>, 3> yolo_engines_;
  std::unique_ptr<PnPSolver> pnp_solver_;
  std::unique_ptr<ArmorTracker> tracker_;      // Params::tracking: the one tracker behind the three engines
  std::array<double, 9> cam_R_{1, 0, 0, 0, 1, 0, 0, 0, 1};
  std::array<double, 3> cam_t_{0, 0, 0};
  int64_t track_epoch_ns_ = 0;                 // the first tracked frame's stamp: the tracker's time zero
  bool track_epoch_set_ = false;
};
}  // namespace irmv_detection
