// ROS2 component shell around IrmDetectorCore: the node surface of the reference (reference src/irm_detector.cpp:25-78
// constructor, :122-174 parameters, :176-245 callback -> /detector/armors, :372-403 live parameter updates), with the
// TensorRT engines replaced by the HIP engine.  NOT compiled in the build image (no ROS2 there): see CMakeLists.txt.
// Frames arrive through `image_buffers()` + `on_frame(slot, stamp)` from whatever camera driver the deployment uses
// (the reference's VirtualCamera / MVCamera, src/camera.cpp, src/mv_camera.cpp, are out of scope: SURVEY section 2).
#include <auto_aim_interfaces/msg/armors.hpp>
#include <rclcpp/rclcpp.hpp>
#include <rclcpp_components/register_node_macro.hpp>
#include <sensor_msgs/msg/image.hpp>

#include "irmv_detection/irm_detector_core.hpp"

namespace irmv_detection
{
class IrmDetector
{
public:
  explicit IrmDetector(const rclcpp::NodeOptions & options)
  {
    node_ = std::make_shared<rclcpp::Node>("irmv_detector", options);
    IrmDetectorCore::Params p;
    p.profiling = node_->declare_parameter("profiling", false);
    const auto sz = node_->declare_parameter("image_input_size", std::vector<int64_t>{1280, 1024});
    p.image_input_size = cv::Size(int(sz[0]), int(sz[1]));
    p.binary_threshold = int(node_->declare_parameter("binary_threshold", 150));
    p.light_min_ratio = node_->declare_parameter("light.min_ratio", 0.1);
    p.light_max_ratio = node_->declare_parameter("light.max_ratio", 0.4);
    p.light_max_angle = node_->declare_parameter("light.max_angle", 40.0);
    p.armor_min_small_center_distance = node_->declare_parameter("armor.min_small_center_distance", 0.8);
    p.armor_max_small_center_distance = node_->declare_parameter("armor.max_small_center_distance", 3.2);
    p.armor_min_large_center_distance = node_->declare_parameter("armor.min_large_center_distance", 3.2);
    p.armor_max_large_center_distance = node_->declare_parameter("armor.max_large_center_distance", 5.5);
    p.device = int(node_->declare_parameter("device", 0));
    p.enemy_color = int(node_->declare_parameter("enemy_color", -1));   // 0 for blue, 1 for red (reference :154-160), -1: no filter; live through the callback below
    for (int64_t c : node_->declare_parameter("large_plate_classes", std::vector<int64_t>{})) p.large_plate_classes.push_back(int(c));
    p.point_source = int(node_->declare_parameter("point_source", 0));   // IRMV_POINTS_*: 0 auto, 3 refined (a pose model's points snapped to the light bars)
    p.refine_snap = node_->declare_parameter("refine.snap", 0.5);         // live through the callback below, like refine.roi_margin
    p.refine_roi_margin = node_->declare_parameter("refine.roi_margin", 4.0);
    p.debug = node_->declare_parameter("debug", false);                   // reference :90-95; live through the callback below (:380-381)
    p.debug_scale = int(node_->declare_parameter("debug_scale", 1));      // 1, 2 or 4: the debug images at full, half or quarter size
    // frame metering (IrmDetectorCore::Params::metering): "" off, "view" or "raw" on the rectangle {x0, y0, w, h} ({0, 0, 0, 0}: the
    // whole view) every metering_step pixels; awb_period (live through the callback below): gray-world white balance every n-th
    // frame, for a Bayer src_format with "raw" metering
    p.src_format = int(node_->declare_parameter("src_format", 0));        // IRMV_SRC_*: 0 HWC, 1..4 the Bayer patterns
    const std::string metering = node_->declare_parameter("metering", std::string(""));
    const auto mr = node_->declare_parameter("metering_rect", std::vector<int64_t>{0, 0, 0, 0});
    const int metering_step = int(node_->declare_parameter("metering_step", 1));
    if (!metering.empty() && mr.size() == 4)
      p.metering = YoloEngine::meter_opts(metering == "raw" ? IRMV_METER_RAW : IRMV_METER_VIEW, cv::Point(int(mr[0]), int(mr[1])), cv::Size(int(mr[2]), int(mr[3])), metering_step);
    p.awb_period = int(node_->declare_parameter("awb_period", 0));
    // constrained pose (IrmDetectorCore::Params::yaw_solve): the plate's yaw solved at its known tilt beside every pose;
    // yaw_publish: the message carries that pose where it was solved
    if (node_->declare_parameter("yaw_solve", false)) p.yaw_solve = YoloEngine::yaw_opts();
    p.yaw_publish = node_->declare_parameter("yaw_publish", false);
    // pose uncertainty (IrmDetectorCore::Params::pose_cov): the first-order covariance of every pose under sigma_px of corner
    // noise (FrameResult::covs; not published: auto_aim_interfaces has no field for it, INTEGRATION.md shows the layout of a
    // geometry_msgs/PoseWithCovariance)
    p.pose_cov = node_->declare_parameter("pose_cov", false);
    p.sigma_px = node_->declare_parameter("sigma_px", 1.0);
    // armor tracks (IrmDetectorCore::Params::tracking): frame-to-frame ids and a velocity filter over the published armors
    // (FrameResult::det_tracks / tracks; not published: auto_aim_interfaces has no field for them)
    if (node_->declare_parameter("tracking", false)) p.tracking = ArmorTracker::default_opts();
    // plate patches (IrmDetectorCore::Params::patches): each armor's rectified number image beside its pose (FrameResult::patches;
    // not published)
    if (node_->declare_parameter("patches", false)) p.patches = YoloEngine::patch_opts();
    // plate numbers (IrmDetectorCore::Params::number_model): the path of an .irmn model, "" = off; each armor's patch read by that
    // MLP beside its pose (FrameResult::numbers; not published).  Live through the callback below.
    p.number_model = node_->declare_parameter("number_model", std::string(""));
    const auto ns = node_->declare_parameter("net_input_size", std::vector<int64_t>{0, 0});   // {width, height}; {0, 0}: square default
    if (ns.size() == 2) p.net_input_size = cv::Size(int(ns[0]), int(ns[1]));
    const std::string model = node_->declare_parameter("model_path", std::string("models/yolov7.onnx"));
    const auto k = node_->declare_parameter("camera_matrix", std::vector<double>{957.669211, 0, 345.943891, 0, 969.127115, 284.057302, 0, 0, 1});
    const auto d = node_->declare_parameter("distortion", std::vector<double>{-0.405274, 0.126058, -0.026939, -0.006503, 0.0});
    std::array<double, 9> K{};
    for (size_t i = 0; i < 9 && i < k.size(); i++) K[i] = k[i];
    core_ = std::make_unique<IrmDetectorCore>(model, K, d, p);
    armors_pub_ = node_->create_publisher<auto_aim_interfaces::msg::Armors>("/detector/armors", rclcpp::SensorDataQoS());
    // the reference's two debug topics (:90-95), as plain rgb8 sensor_msgs/Image: the pictures come finished from the GPU
    // (IrmDetectorCore::FrameResult), so neither cv_bridge nor image_transport is needed.  Created always: `debug` is live.
    visualized_img_pub_ = node_->create_publisher<sensor_msgs::msg::Image>("/image/visualized_image", rclcpp::SensorDataQoS());
    binary_img_pub_ = node_->create_publisher<sensor_msgs::msg::Image>("/image/binary_image", rclcpp::SensorDataQoS());
    param_handle_ = node_->add_on_set_parameters_callback([this](const std::vector<rclcpp::Parameter> & ps) {
      rcl_interfaces::msg::SetParametersResult r;
      r.successful = true;
      r.reason = "success";
      for (const auto & q : ps)
        if (q.get_type() == rclcpp::ParameterType::PARAMETER_BOOL) core_->set_bool_parameter(q.get_name(), q.as_bool());
        else if (q.get_type() == rclcpp::ParameterType::PARAMETER_INTEGER) core_->set_parameter(q.get_name(), double(q.as_int()));
        else if (q.get_type() == rclcpp::ParameterType::PARAMETER_DOUBLE) core_->set_parameter(q.get_name(), q.as_double());
        else if (q.get_type() == rclcpp::ParameterType::PARAMETER_STRING) core_->set_parameter(q.get_name(), q.as_string());
      return r;
    });
  }

  rclcpp::node_interfaces::NodeBaseInterface::SharedPtr get_node_base_interface() const { return node_->get_node_base_interface(); }
  std::array<uint8_t *, 3> image_buffers() const { return core_->image_buffers(); }

  // Camera::CameraCallback body (src/irm_detector.cpp:176-245)
  void on_frame(int slot, std::chrono::time_point<std::chrono::system_clock> stamp)
  {
    const auto r = core_->message_callback(StampedFrame{stamp, slot});
    auto_aim_interfaces::msg::Armors msg;
    msg.header.stamp = rclcpp::Time(r.armors_msg.header.stamp_ns, RCL_ROS_TIME);
    msg.header.frame_id = r.armors_msg.header.frame_id;
    for (const auto & a : r.armors_msg.armors) {
      auto_aim_interfaces::msg::Armor m;
      m.pose.position.x = a.pose.position.x; m.pose.position.y = a.pose.position.y; m.pose.position.z = a.pose.position.z;
      m.pose.orientation.x = a.pose.orientation.x; m.pose.orientation.y = a.pose.orientation.y;
      m.pose.orientation.z = a.pose.orientation.z; m.pose.orientation.w = a.pose.orientation.w;
      m.distance_to_image_center = a.distance_to_image_center;
      msg.armors.emplace_back(m);
    }
    armors_pub_->publish(msg);
    if (!r.visualized_image.empty()) {   // debug is on (:259-280)
      visualized_img_pub_->publish(image_msg(r.visualized_image, msg.header));
      binary_img_pub_->publish(image_msg(r.binary_image, msg.header));
    }
  }

private:
  static sensor_msgs::msg::Image image_msg(const cv::Mat & m, const std_msgs::msg::Header & header)
  {
    sensor_msgs::msg::Image img;
    img.header = header;
    img.height = uint32_t(m.rows);
    img.width = uint32_t(m.cols);
    img.encoding = "rgb8";   // as the reference publishes them (:271, :279)
    img.is_bigendian = 0;
    img.step = uint32_t(m.cols) * 3;
    img.data.assign(m.data, m.data + size_t(m.rows) * m.cols * 3);
    return img;
  }

  rclcpp::Publisher<sensor_msgs::msg::Image>::SharedPtr visualized_img_pub_, binary_img_pub_;
  rclcpp::Node::SharedPtr node_;
  std::unique_ptr<IrmDetectorCore> core_;
  rclcpp::Publisher<auto_aim_interfaces::msg::Armors>::SharedPtr armors_pub_;
  rclcpp::node_interfaces::OnSetParametersCallbackHandle::SharedPtr param_handle_;
};
}  // namespace irmv_detection

RCLCPP_COMPONENTS_REGISTER_NODE(irmv_detection::IrmDetector)
