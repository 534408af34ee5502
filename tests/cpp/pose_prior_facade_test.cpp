// Pose ambiguity through the C++ facade (include/irmv_detection/pnp_solver.hpp, yolo_engine.hpp, irm_detector_core.hpp):
// PnPSolver::solvePnPGeneric, YoloEngine::set_pose_prior / set_up / pose_alts, and the core's parameters and FrameResult::alts.
// A plain main().  Without arguments: the parameters only, no engine (exit code 2).  argv = <model.onnx path>: one engine on a
// black 256 x 128 frame and a solver on a fixed quad; prints both solutions as bit patterns.
#include <cstdio>
#include <cstring>
#include <vector>

#include "irmv_detection/irm_detector_core.hpp"
#include "irmv_detection/pnp_solver.hpp"
#include "irmv_detection/yolo_engine.hpp"

int main(int argc, char ** argv)
{
  irmv_detection::IrmDetectorCore::Params params;
  params.pose_prior.struct_size = sizeof(irmv_pose_prior);
  params.pose_prior.mode = IRMV_POSE_PRIOR;
  params.pose_prior.ambiguity_ratio = 8.0;
  for (double & s : params.pose_prior.normal_up) s = -0.25881904510252074;
  params.pose_prior.normal_up_default = -0.25881904510252074;
  params.up = {0.0, -0.9, 0.1};
  irmv_detection::IrmDetectorCore::FrameResult result;
  static_assert(sizeof(irmv_pose_alt) == 104 && sizeof(irmv_pose_prior) == 152, "ABI structs");
  if (argc < 2) return result.alts.empty() && params.pose_prior.mode == 1 ? 2 : 4;

  const cv::Size size(256, 128);
  irmv_detection::YoloEngine engine(argv[1], size, false, -1, false, 128, IRMV_SRC_HWC8, {256, 256, 256}, 64);
  std::memset(engine.get_src_image_buffer(), 0, size_t(size.width) * size.height * 3);
  std::printf("before %d\n", int(engine.delivers_pose_alts()));
  engine.set_pose_prior(&params.pose_prior);
  engine.set_up(params.up);
  const auto u = engine.up();
  std::printf("after %d mode %d up %.17g %.17g %.17g\n", int(engine.delivers_pose_alts()), engine.pose_prior().mode, u[0], u[1], u[2]);
  engine.detect();
  int n = 0;
  engine.last_detections(&n);
  std::printf("records %d alts %zu\n", n, engine.pose_alts().size());

  const std::array<double, 9> K = {957.669211, 0, 345.943891, 0, 969.127115, 284.057302, 0, 0, 1.0};
  irmv_detection::PnPSolver solver(K, {-0.405274, 0.126058, -0.026939, -0.006503, 0.0});
  irmv_detection::Armor armor(irmv_detection::Light(cv::Point2f(300.f, 240.f), cv::Point2f(301.f, 262.f)),
                              irmv_detection::Light(cv::Point2f(352.f, 243.f), cv::Point2f(351.f, 266.f)));
  std::vector<cv::Mat> rvecs, tvecs;
  std::vector<double> errs;
  const int ns = solver.solvePnPGeneric(armor, rvecs, tvecs, errs);
  cv::Mat r1, t1;
  const bool ok = solver.solvePnP(armor, r1, t1);
  std::printf("solutions %d ok %d\n", ns, int(ok));
  for (int s = 0; s < ns; s++) {
    uint64_t b[7];
    for (int i = 0; i < 3; i++) {
      std::memcpy(&b[i], &rvecs[size_t(s)].at<double>(i), 8);
      std::memcpy(&b[3 + i], &tvecs[size_t(s)].at<double>(i), 8);
    }
    std::memcpy(&b[6], &errs[size_t(s)], 8);
    std::printf("sol %d %016llx %016llx %016llx %016llx %016llx %016llx err %016llx\n", s, (unsigned long long)b[0], (unsigned long long)b[1],
                (unsigned long long)b[2], (unsigned long long)b[3], (unsigned long long)b[4], (unsigned long long)b[5], (unsigned long long)b[6]);
  }
  if (ok && ns >= 1)
    for (int i = 0; i < 3; i++)
      if (std::memcmp(&r1.at<double>(i), &rvecs[0].at<double>(i), 8) != 0 || std::memcmp(&t1.at<double>(i), &tvecs[0].at<double>(i), 8) != 0) return 5;
  return 0;
}
