// Pose uncertainty through the C++ surface: YoloEngine::set_pose_cov / pose_cov / pose_covs
// (include/irmv_detection/yolo_engine.hpp), PnPSolver::pose_cov (include/irmv_detection/pnp_solver.hpp) and IrmDetectorCore's
// Params::pose_cov / Params::sigma_px / FrameResult::covs (include/irmv_detection/irm_detector_core.hpp), on a 128 x 96 frame
// with a 64 x 64 net.
//   * the facade: pose_covs() is empty before the first set_pose_cov; afterwards it is parallel to the detections and written
//     to <out file> beside them, where the Python test compares both with the C ABI's records and with the host reference;
//     sigma_px is live, off zeroes the records
//   * the core: FrameResult::covs parallel to armors and poses, the bytes of the engine's records; "pose_cov" and "sigma_px"
//     are live
// argv: <model.onnx path (sibling .irmw exists)> <128 x 96 x 3 frame file> <out file>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <vector>

#include "irmv_detection/irm_detector_core.hpp"
#include "irmv_detection/pnp_solver.hpp"

using namespace irmv_detection;

static int fails = 0;
#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__);     \
      std::printf(__VA_ARGS__);                            \
      std::printf("\n");                                   \
      fails++;                                             \
    }                                                      \
  } while (0)

template <class F> static bool throws(F && f)
{
  try { f(); } catch (const std::exception &) { return true; }
  return false;
}

static bool same(const std::vector<irmv_pose_cov> & a, const std::vector<irmv_pose_cov> & b)
{
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(irmv_pose_cov)) == 0);
}

static bool all_zero(const std::vector<irmv_pose_cov> & a)
{
  const irmv_pose_cov z{};
  for (const auto & r : a)
    if (std::memcmp(&r, &z, sizeof z) != 0) return false;
  return true;
}

static int computed(const std::vector<irmv_pose_cov> & a)
{
  int n = 0;
  for (const auto & r : a) n += r.state == 1;
  return n;
}

int main(int argc, char ** argv)
{
  if (argc < 4) return 2;
  const cv::Size size(128, 96);
  std::vector<uint8_t> frame(size_t(size.width) * size.height * 3);
  {
    std::ifstream f(argv[2], std::ios::binary);
    f.read(reinterpret_cast<char *>(frame.data()), std::streamsize(frame.size()));
    if (!f) return 3;
  }
  const std::array<double, 9> K = {957.669211, 0, 345.943891, 0, 969.127115, 284.057302, 0, 0, 1};
  const std::vector<double> D = {-0.405274, 0.126058, -0.026939, -0.006503, 0.0};

  {
    YoloEngine eng(argv[1], size, false, -1, false, 64);
    std::memcpy(eng.get_src_image_buffer(), frame.data(), frame.size());
    const auto before = eng.detect();
    CHECK(!before.empty(), "detections");
    CHECK(eng.pose_covs().empty() && eng.pose_cov().enable == 0 && eng.pose_cov().sigma_px == 1.0, "nothing before the first set");
    CHECK(throws([&] { eng.set_pose_cov(YoloEngine::pose_cov_opts(true, 0.0)); }) && eng.pose_covs().empty(), "sigma_px = 0 throws");
    CHECK(throws([&] { eng.set_pose_cov(YoloEngine::pose_cov_opts(true, 64.5)); }) && eng.pose_cov().enable == 0, "sigma_px > 64 throws");
    eng.set_yaw_solve();
    eng.set_pose_cov(YoloEngine::pose_cov_opts(true, 0.5));
    CHECK(eng.pose_cov().enable == 1 && eng.pose_cov().sigma_px == 0.5, "on");
    CHECK(eng.detect() == before, "the detections do not change");
    int n = 0;
    const irmv_det * dets = eng.last_detections(&n);
    const auto covs = eng.pose_covs();
    const auto yaws = eng.yaw_poses();
    CHECK(int(covs.size()) == n && yaws.size() == covs.size() && n > 0, "parallel to the detections: %zu %zu %d", covs.size(), yaws.size(), n);
    CHECK(computed(covs) >= 1, "a computed record");
    // the stand-alone call on the same points and pose
    PnPSolver pnp(K, D);
    int compared = 0;
    for (int i = 0; i < n; i++) {
      const irmv_det & d = dets[i];
      CHECK((covs[size_t(i)].state != 0) == (d.pnp_ok == 1 && d.armor_valid == 1), "record %d: a state wherever there is a pose", i);
      if (covs[size_t(i)].state != 1) continue;
      const Armor a(Light(cv::Point2f(d.kpts[2], d.kpts[3]), cv::Point2f(d.kpts[0], d.kpts[1])),
                    Light(cv::Point2f(d.kpts[4], d.kpts[5]), cv::Point2f(d.kpts[6], d.kpts[7])));
      cv::Mat rv(3, 1, CV_64F), tv(3, 1, CV_64F);
      for (int k = 0; k < 3; k++) { rv.at<double>(k) = d.rvec[k]; tv.at<double>(k) = d.tvec[k]; }
      const irmv_pose_cov one = pnp.pose_cov(a, rv, tv, 0.5, nullptr, d.armor_size);
      CHECK(one.state == 1 && one.yaw_state == 0 && std::memcmp(one.cov, covs[size_t(i)].cov, 23 * sizeof(double)) == 0,
            "record %d: PnPSolver::pose_cov gives the step's 6 x 6 block", i);
      compared++;
    }
    CHECK(compared >= 1, "a record compared with PnPSolver::pose_cov");
    {
      std::ofstream o(argv[3], std::ios::binary);
      const int32_t count = int32_t(n);
      o.write(reinterpret_cast<const char *>(&count), 4);
      o.write(reinterpret_cast<const char *>(dets), std::streamsize(size_t(n) * sizeof(irmv_det)));
      o.write(reinterpret_cast<const char *>(yaws.data()), std::streamsize(yaws.size() * sizeof(irmv_yaw_pose)));
      o.write(reinterpret_cast<const char *>(covs.data()), std::streamsize(covs.size() * sizeof(irmv_pose_cov)));
      CHECK(bool(o), "the out file");
    }
    eng.set_pose_cov(YoloEngine::pose_cov_opts(false, 0.5));
    CHECK(eng.pose_covs().size() == covs.size() && all_zero(eng.pose_covs()), "off: the records are zero");
    CHECK(eng.detect() == before && all_zero(eng.pose_covs()), "... and stay zero");
    eng.set_pose_cov(YoloEngine::pose_cov_opts(true, 0.5));
    eng.detect();
    CHECK(same(eng.pose_covs(), covs), "on again: the same records");
  }

  IrmDetectorCore::Params prm;
  prm.image_input_size = size;
  prm.net_input_size = cv::Size(64, 64);
  StampedFrame img;
  std::vector<irmv_pose_cov> at_one;
  {
    IrmDetectorCore plain(argv[1], K, D, prm);
    for (uint8_t * b : plain.image_buffers()) std::memcpy(b, frame.data(), frame.size());
    img.id = 0;
    auto r = plain.message_callback(img);
    CHECK(!r.armors.empty() && r.covs.empty(), "no records without Params::pose_cov");
    CHECK(plain.set_parameter("pose_cov", 0.0) && !plain.params().pose_cov, "off while off");
    CHECK(!plain.set_parameter("pose_cov", 2.0) && !plain.set_parameter("sigma_px", 0.0) && !plain.set_parameter("sigma_px", 65.0), "bad values are refused");
    CHECK(plain.set_parameter("pose_cov", 1.0) && plain.params().pose_cov, "pose_cov is live");
    r = plain.message_callback(img);
    CHECK(r.covs.size() == r.armors.size() && computed(r.covs) >= 1, "... and the next frame carries the records");
    at_one = r.covs;
    CHECK(plain.set_parameter("sigma_px", 2.0) && plain.params().sigma_px == 2.0, "sigma_px is live");
    r = plain.message_callback(img);
    bool scaled = r.covs.size() == at_one.size();
    for (size_t i = 0; scaled && i < r.covs.size(); i++)
      if (at_one[i].state == 1) scaled = std::fabs(r.covs[i].cov[0] - 4.0 * at_one[i].cov[0]) <= 1e-12 * r.covs[i].cov[0];
    CHECK(scaled, "twice the noise, four times the variance");
  }
  prm.pose_cov = true;
  prm.sigma_px = 1.0;
  IrmDetectorCore core(argv[1], K, D, prm);
  for (uint8_t * b : core.image_buffers()) std::memcpy(b, frame.data(), frame.size());
  for (int id = 0; id < 3; id++) {
    img.id = id;
    const auto r = core.message_callback(img);
    CHECK(!r.armors.empty() && r.covs.size() == r.armors.size() && r.poses.size() == r.armors.size(), "engine %d: covs parallel to armors: %zu %zu",
          id, r.covs.size(), r.armors.size());
    CHECK(computed(r.covs) >= 1 && same(r.covs, at_one), "engine %d: the records of the engine that was switched on live", id);
    const auto all = core.engine(id).pose_covs();
    CHECK(all.size() >= r.covs.size(), "engine %d: the engine's records", id);
  }
  CHECK(core.set_parameter("pose_cov", 0.0) && !core.params().pose_cov, "off");
  img.id = 2;
  const auto r = core.message_callback(img);
  CHECK(r.covs.size() == r.armors.size() && all_zero(r.covs), "off: zero records");
  std::printf("pose_cov_facade_test fails %d\n", fails);
  return fails ? 1 : 0;
}
