// Frame metering through the C++ surface: YoloEngine::set_metering / frame_stats / meter (include/irmv_detection/yolo_engine.hpp)
// and the automatic white balance of IrmDetectorCore (include/irmv_detection/irm_detector_core.hpp), on a 100 x 68 RGGB frame
// with a 64 x 64 net.
//   * the facade: frame_stats() throws before set_metering; afterwards the record of detect() == meter() == the record the
//     Python test wrote beside the frame (irmv_detection_amd/metering.py); nullptr switches it off
//   * the core with awb_period = 2 and RAW metering: FrameResult::stats is that record on every frame; the second frame sets
//     gains, which are irmv_stats_gray_world's on that record, reach all three engines and keep the tone LUT
//   * awb_period without a Bayer format or without RAW metering: the constructor throws, set_parameter refuses
// argv: <model.onnx path (sibling .irmw exists)> <raw 100 x 68 frame file> <irmv_frame_stats file> <gain R> <gain B>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <vector>

#include "irmv_detection/irm_detector_core.hpp"

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

static bool same(const irmv_frame_stats & a, const irmv_frame_stats & b) { return std::memcmp(&a, &b, sizeof a) == 0; }

template <class F> static bool throws(F && f)
{
  try { f(); } catch (const std::exception &) { return true; }
  return false;
}

int main(int argc, char ** argv)
{
  if (argc < 6) return 2;
  const cv::Size size(100, 68);
  std::vector<uint8_t> frame(size_t(size.width) * size.height);
  irmv_frame_stats want;
  {
    std::ifstream f(argv[2], std::ios::binary), s(argv[3], std::ios::binary);
    f.read(reinterpret_cast<char *>(frame.data()), std::streamsize(frame.size()));
    s.read(reinterpret_cast<char *>(&want), sizeof want);
    if (!f || !s) return 3;
  }
  const std::array<uint16_t, 3> want_gains = {uint16_t(std::atoi(argv[4])), 256, uint16_t(std::atoi(argv[5]))};

  {
    YoloEngine eng(argv[1], size, false, -1, false, 64, IRMV_SRC_BAYER_RGGB8);
    std::memcpy(eng.get_src_image_buffer(), frame.data(), frame.size());
    CHECK(eng.is_bayer() && !eng.metering(), "a Bayer engine, metering off");
    CHECK(throws([&] { eng.frame_stats(); }), "frame_stats before set_metering throws");
    CHECK(same(eng.meter(IRMV_METER_RAW), want), "meter() on an engine that never enabled it");
    CHECK(throws([&] { eng.set_metering(IRMV_METER_RAW, {}, {}, 3); }), "step 3 is refused");
    eng.set_metering(IRMV_METER_RAW);
    irmv_meter_opts o{};
    CHECK(eng.metering(&o) && o.domain == IRMV_METER_RAW && o.step == 1, "the options in force");
    const auto bboxes = eng.detect();
    CHECK(!bboxes.empty(), "detections");
    CHECK(same(eng.frame_stats(), want), "frame_stats() of detect()");
    CHECK(same(eng.meter(IRMV_METER_RAW), want), "meter() == frame_stats()");
    const irmv_frame_stats part = eng.meter(IRMV_METER_VIEW, cv::Point(13, 7), cv::Size(51, 33), 2);
    CHECK(part.rect[0] == 13 && part.rect[1] == 7 && part.rect[2] == 51 && part.rect[3] == 33 && part.n[0] == 26 * 17 && part.domain == IRMV_METER_VIEW, "a rectangle on demand");
    CHECK(same(eng.frame_stats(), want), "meter() leaves the step's record alone");
    eng.set_metering(nullptr);
    CHECK(!eng.metering() && eng.detect() == bboxes, "off; the detections do not change");
    const irmv_frame_stats off = eng.frame_stats();
    CHECK(off.n[3] == 0 && off.domain == 0 && off.step == 0, "the record of a step that ran with metering off is zero");
  }

  const std::array<double, 9> K = {957.669211, 0, 345.943891, 0, 969.127115, 284.057302, 0, 0, 1};
  const std::vector<double> D = {-0.405274, 0.126058, -0.026939, -0.006503, 0.0};
  IrmDetectorCore::Params prm;
  prm.image_input_size = size;
  prm.net_input_size = cv::Size(64, 64);
  prm.awb_period = 2;
  CHECK(throws([&] { IrmDetectorCore bad(argv[1], K, D, prm); }), "awb_period on HWC engines without metering throws");
  prm.src_format = IRMV_SRC_BAYER_RGGB8;
  prm.metering = YoloEngine::meter_opts(IRMV_METER_VIEW);
  CHECK(throws([&] { IrmDetectorCore bad(argv[1], K, D, prm); }), "awb_period with VIEW metering throws");
  {
    IrmDetectorCore::Params hp;
    hp.image_input_size = size;
    hp.net_input_size = cv::Size(64, 64);
    IrmDetectorCore hwc(argv[1], K, D, hp);
    CHECK(!hwc.set_parameter("awb_period", 2) && hwc.params().awb_period == 0 && hwc.set_parameter("awb_period", 0), "awb_period is refused on an HWC core");
    StampedFrame img;
    CHECK(!hwc.message_callback(img).stats_valid, "no record without Params::metering");
  }
  prm.metering = YoloEngine::meter_opts(IRMV_METER_RAW);
  IrmDetectorCore core(argv[1], K, D, prm);
  for (uint8_t * b : core.image_buffers()) std::memcpy(b, frame.data(), frame.size());
  std::vector<uint8_t> lut(3 * 256);
  for (int c = 0; c < 3; c++)
    for (int v = 0; v < 256; v++) lut[size_t(c * 256 + v)] = uint8_t(255 - v / (c + 1));
  for (int id = 0; id < 3; id++) core.engine(id).set_bayer_isp({256, 256, 256}, lut.data());
  StampedFrame img;
  img.id = 1;
  auto r = core.message_callback(img);
  CHECK(r.stats_valid && same(r.stats, want) && !r.awb_applied, "frame 1: the record, no new gains");
  CHECK(core.engine(0).bayer_gains() == (std::array<uint16_t, 3>{256, 256, 256}), "the gains are still the identity");
  img.id = 2;
  r = core.message_callback(img);
  CHECK(r.stats_valid && same(r.stats, want), "frame 2: the RAW record does not depend on the gains");
  std::array<uint16_t, 3> helper{0, 0, 0};
  CHECK(irmv_stats_gray_world(&r.stats, 8, 247, helper.data()) == IRMV_OK && helper == want_gains, "the helper's gains are the reference's: %d %d %d", helper[0], helper[1], helper[2]);
  CHECK(r.awb_applied && r.awb_gains == helper, "frame 2 set the helper's gains");
  for (int id = 0; id < 3; id++) {
    std::vector<uint8_t> got;
    CHECK(core.engine(id).bayer_gains(&got) == helper && got == lut, "engine %d: the gains, and the tone LUT kept", id);
  }
  CHECK(core.set_parameter("awb_period", 0) && !core.set_parameter("awb_period", -1) && !core.set_parameter("awb_period", 1.5), "awb_period is live");
  for (int id = 0; id < 3; id++) core.engine(id).set_bayer_isp({256, 256, 256}, lut.data());
  img.id = 0;
  r = core.message_callback(img);
  r = core.message_callback(img);
  CHECK(r.stats_valid && !r.awb_applied && core.engine(0).bayer_gains() == (std::array<uint16_t, 3>{256, 256, 256}), "awb off: the gains stay");
  // an all-dark frame: the helper refuses, the gains stay
  CHECK(core.set_parameter("awb_period", 1), "awb_period 1");
  std::memset(core.image_buffers()[0], 0, frame.size());
  r = core.message_callback(img);
  CHECK(r.stats_valid && r.stats.hist[3][0] == r.stats.n[3] && !r.awb_applied, "a frame without mass in [8, 247] leaves the gains alone");
  CHECK(core.engine(1).bayer_gains() == (std::array<uint16_t, 3>{256, 256, 256}), "... on every engine");
  std::printf("metering_test fails %d\n", fails);
  return fails ? 1 : 0;
}
