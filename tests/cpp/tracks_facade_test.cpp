// Armor tracks through the C++ surface: YoloEngine::set_tracking / tracking / set_stamp / set_camera_pose / det_tracks / tracks /
// reset_tracks (include/irmv_detection/yolo_engine.hpp), ArmorTracker (include/irmv_detection/tracker.hpp) and IrmDetectorCore's
// Params::tracking / FrameResult::det_tracks / tracks (include/irmv_detection/irm_detector_core.hpp), on a 128 x 96 frame with a
// 64 x 64 net.
//   * the facade: nothing before the first set_tracking; one frame stepped four times with rising stamps -- started, then
//     matched with d2 == 0, confirmed at the third step; the records of every step go to <out file>, where the Python test
//     feeds the host reference with the detections and compares; a stale stamp is refused; off zeroes
//   * ArmorTracker fed the facade's detections gives the engine's records, byte for byte
//   * the core: ONE tracker behind the three engines -- the ids persist from engine to engine, stamped from the frames' time stamps
// argv: <model.onnx path (sibling .irmw exists)> <128 x 96 x 3 frame file> <out file>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <vector>

#include "irmv_detection/irm_detector_core.hpp"
#include "irmv_detection/tracker.hpp"

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

template <class R> static bool same(const std::vector<R> & a, const std::vector<R> & b)
{
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(R)) == 0);
}

template <class R> static bool all_zero(const std::vector<R> & a)
{
  for (const auto & r : a) {
    const unsigned char * p = reinterpret_cast<const unsigned char *>(&r);
    for (size_t i = 0; i < sizeof(R); i++)
      if (p[i]) return false;
  }
  return true;
}

static int with_state(const std::vector<irmv_det_track> & a, int state)
{
  int n = 0;
  for (const auto & r : a) n += r.state == state;
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
  const std::array<double, 9> R = {1, 0, 0, 0, 1, 0, 0, 0, 1};

  {
    YoloEngine eng(argv[1], size, false, -1, false, 64);
    std::memcpy(eng.get_src_image_buffer(), frame.data(), frame.size());
    const auto before = eng.detect();
    CHECK(!before.empty(), "detections");
    CHECK(eng.det_tracks().empty() && eng.tracks().empty() && eng.tracking().enable == 0 && eng.tracking().gate == 16.27, "nothing before the first set");
    irmv_track_opts bad = YoloEngine::track_opts();
    bad.gate = 0.0;
    CHECK(throws([&] { eng.set_tracking(bad); }) && eng.det_tracks().empty(), "gate = 0 throws");
    eng.set_tracking();
    CHECK(eng.tracking().enable == 1 && eng.tracking().confirm_hits == 3, "on");
    ArmorTracker alone;
    std::ofstream o(argv[3], std::ios::binary);
    int n = 0;
    const int32_t steps = 4;
    o.write(reinterpret_cast<const char *>(&steps), 4);
    for (int k = 0; k < steps; k++) {
      const double t = 0.5 + 0.02 * k;
      const std::array<double, 3> tw = {0.01 * k, 0.0, 0.0};
      eng.set_stamp(t);
      eng.set_camera_pose(R, tw);
      CHECK(eng.detect() == before, "the detections do not change");
      const irmv_det * dets = eng.last_detections(&n);
      irmv_track_frame fr{};
      const auto dt = eng.det_tracks();
      const auto tr = eng.tracks(&fr);
      CHECK(int(dt.size()) == n && tr.size() == size_t(IRMV_TRACK_CAP) && fr.state == 1 && fr.stamp == t, "step %d: parallel to the detections, 32 tracks", k);
      CHECK(k == 0 ? (with_state(dt, 2) >= 1 && with_state(dt, 1) == 0) : with_state(dt, 1) >= 1, "step %d: started, then matched", k);
      CHECK(fr.n_confirmed == (k >= 2 ? fr.n_live : 0) && fr.n_live >= 1, "step %d: confirmed at the third step", k);
      std::vector<irmv_track_obs> obs;
      for (int i = 0; i < n; i++) obs.push_back(ArmorTracker::observation(dets[i]));
      const ArmorTracker::Result r = alone.update(t, obs, &R, &tw);
      CHECK(same(r.det_tracks, dt) && same(r.tracks, tr) && std::memcmp(&r.frame, &fr, sizeof fr) == 0, "step %d: ArmorTracker on the same records", k);
      const int32_t count = n;
      o.write(reinterpret_cast<const char *>(&count), 4);
      o.write(reinterpret_cast<const char *>(&t), 8);
      o.write(reinterpret_cast<const char *>(tw.data()), 24);
      o.write(reinterpret_cast<const char *>(dets), std::streamsize(size_t(n) * sizeof(irmv_det)));
      o.write(reinterpret_cast<const char *>(dt.data()), std::streamsize(dt.size() * sizeof(irmv_det_track)));
      o.write(reinterpret_cast<const char *>(&fr), sizeof fr);
      o.write(reinterpret_cast<const char *>(tr.data()), std::streamsize(tr.size() * sizeof(irmv_track)));
    }
    CHECK(bool(o), "the out file");
    // irmv_track_predict on a live track: its own position at its own stamp
    {
      const auto tr = eng.tracks();
      double pos[3], cov[9];
      CHECK(irmv_track_predict(&tr[0], tr[0].stamp, 8.0, pos, cov) == IRMV_OK && pos[0] == tr[0].x[0] && cov[0] == tr[0].P[0], "predict at dt = 0");
      CHECK(irmv_track_predict(&tr[0], tr[0].stamp + 0.1, 8.0, pos, cov) == IRMV_OK && cov[0] > tr[0].P[0], "predict ahead: the covariance grows");
    }
    eng.set_stamp(0.1);
    eng.detect();
    irmv_track_frame fr{};
    eng.tracks(&fr);
    CHECK(fr.state == -2 && all_zero(eng.det_tracks()) && int(eng.det_tracks().size()) == n, "a stale stamp is refused");
    eng.reset_tracks();
    eng.detect();
    eng.tracks(&fr);
    CHECK(fr.state == 1 && fr.n_started >= 1 && fr.n_confirmed == 0, "reset: an empty table and no stamp");
    eng.set_tracking(YoloEngine::track_opts(false));
    CHECK(all_zero(eng.det_tracks()) && all_zero(eng.tracks()), "off: the records are zero");
    CHECK(eng.detect() == before && all_zero(eng.det_tracks()), "... and stay zero");
  }

  IrmDetectorCore::Params prm;
  prm.image_input_size = size;
  prm.net_input_size = cv::Size(64, 64);
  StampedFrame img;
  {
    IrmDetectorCore plain(argv[1], K, D, prm);
    for (uint8_t * b : plain.image_buffers()) std::memcpy(b, frame.data(), frame.size());
    auto r = plain.message_callback(img);
    CHECK(!r.armors.empty() && r.det_tracks.empty() && r.tracks.empty() && r.track_frame.state == 0, "no records without Params::tracking");
    CHECK(!plain.set_parameter("tracking", 2.0) && plain.set_parameter("tracking", 0.0), "bad values are refused, off while off");
    CHECK(plain.set_parameter("tracking", 1.0) && plain.params().tracking.enable == 1, "tracking is live");
    img.time_stamp += std::chrono::milliseconds(10);
    r = plain.message_callback(img);
    CHECK(r.det_tracks.size() == r.armors.size() && with_state(r.det_tracks, 2) >= 1 && r.track_frame.stamp == 0.0, "... and the next frame starts tracks at time zero");
  }
  prm.tracking = ArmorTracker::default_opts();
  prm.pose_cov = true;
  IrmDetectorCore core(argv[1], K, D, prm);
  for (uint8_t * b : core.image_buffers()) std::memcpy(b, frame.data(), frame.size());
  std::vector<irmv_det_track> first;
  for (int k = 0; k < 6; k++) {
    img.id = k % 3;
    img.time_stamp += std::chrono::milliseconds(10);
    const auto r = core.message_callback(img);
    CHECK(!r.armors.empty() && r.det_tracks.size() == r.armors.size() && r.tracks.size() == size_t(IRMV_TRACK_CAP) && r.covs.size() == r.armors.size(),
          "frame %d: det_tracks parallel to armors: %zu %zu", k, r.det_tracks.size(), r.armors.size());
    CHECK(r.track_frame.state == 1 && (k == 0 || r.track_frame.stamp > 0.0), "frame %d: stamped from the frame's time", k);
    if (k == 0) first = r.det_tracks;
    else {
      bool kept = r.det_tracks.size() == first.size();
      for (size_t i = 0; kept && i < first.size(); i++)
        if (first[i].state == 2) kept = r.det_tracks[i].state == 1 && r.det_tracks[i].id == first[i].id && r.det_tracks[i].hits == k + 1;
      CHECK(kept, "frame %d (engine %d): one table behind the three engines, the ids persist", k, img.id);
    }
    CHECK(k < 2 || r.track_frame.n_confirmed >= 1, "frame %d: confirmed", k);
  }
  CHECK(core.set_camera_pose(R, {0.5, 0.0, 0.0}) && !core.set_camera_pose(R, {NAN, 0.0, 0.0}), "the camera pose: finite values only");
  CHECK(core.set_parameter("tracking", 0.0), "off");
  const auto r = core.message_callback(img);
  CHECK(r.det_tracks.empty() && r.tracks.empty(), "off: no records");
  std::printf("tracks_facade_test fails %d\n", fails);
  return fails ? 1 : 0;
}
