// The debug images through the C++ surface: YoloEngine::render (include/irmv_detection/yolo_engine.hpp) and the debug mode of
// IrmDetectorCore (include/irmv_detection/irm_detector_core.hpp), on a 100 x 68 frame with a 64 x 64 net.
//   * colour, scale 1, no marks == get_rotated_image()
//   * colour, scale 1, boxes + labels on explicit records == get_rotated_image() + visualize_bboxes()
//   * nullptr records == the last detect()'s own records, handed over explicitly
//   * scale 2 and 4 halve and quarter the size; a bad scale throws and the engine goes on
//   * the core: no images until debug is switched on live; then visualized_image == render(colour, all marks) and
//     binary_image == render(binary, boxes + labels) of that frame's records, at the live debug_scale and binary_threshold
// The pictures themselves are compared with the host reference in tests/test_gpu_render.py.
// argv: <model.onnx path (sibling .irmw exists)> <raw 100 x 68 x 3 frame file>
#include <cstdio>
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

static bool same(const cv::Mat & a, const cv::Mat & b)
{
  return a.rows == b.rows && a.cols == b.cols && a.rows > 0 && std::memcmp(a.data, b.data, size_t(a.rows) * a.cols * 3) == 0;
}

int main(int argc, char ** argv)
{
  if (argc < 3) return 2;
  const cv::Size size(100, 68);
  std::vector<uint8_t> frame(size_t(size.width) * size.height * 3);
  std::ifstream f(argv[2], std::ios::binary);
  f.read(reinterpret_cast<char *>(frame.data()), std::streamsize(frame.size()));
  if (!f) return 3;
  constexpr uint32_t kAll = IRMV_MARK_BOXES | IRMV_MARK_LABELS | IRMV_MARK_ARMORS, kBoxes = IRMV_MARK_BOXES | IRMV_MARK_LABELS;

  {
    YoloEngine eng(argv[1], size, false, -1, false, 64);
    std::memcpy(eng.get_src_image_buffer(), frame.data(), frame.size());
    const auto bboxes = eng.detect();
    CHECK(!bboxes.empty(), "detections");
    const cv::Mat rotated = eng.get_rotated_image().clone();
    const std::vector<irmv_det> none;
    CHECK(same(eng.render(IRMV_RENDER_COLOR, 1, kAll, &none), rotated), "no marks: the rotated image");

    // boxes that meet the frame (where visualize_bboxes without OpenCV and the kernel clamp alike), both colours, UNKNOWN
    const std::vector<YoloEngine::bbox> boxes = {{{10.5f, 30.2f, 60.9f, 50.f}, 0.5f, ArmorClass::B3}, {{-4.f, 25.f, 30.f, 80.f}, 0.5f, ArmorClass::RS},
                                                 {{70.f, -3.f, 120.f, 40.f}, 0.5f, ArmorClass::UNKNOWN}, {{40.f, 35.f, 55.f, 45.f}, 0.5f, ArmorClass::R1}};
    std::vector<irmv_det> recs;
    for (const auto & b : boxes) {
      irmv_det d{};
      std::copy(b.xyxy.begin(), b.xyxy.end(), d.xyxy);
      d.class_id = int32_t(b.class_id);
      recs.push_back(d);
    }
    cv::Mat drawn = rotated.clone();
    eng.visualize_bboxes(drawn, boxes);
    CHECK(!same(drawn, rotated), "visualize_bboxes drew");
#if !IRMV_HAVE_OPENCV
    CHECK(same(eng.render(IRMV_RENDER_COLOR, 1, kBoxes, &recs), drawn), "scale 1: boxes + labels == visualize_bboxes");
#endif

    int n = 0;
    const irmv_det * last = eng.last_detections(&n);
    const std::vector<irmv_det> own(last, last + n);
    for (int kind : {IRMV_RENDER_COLOR, IRMV_RENDER_BINARY})
      for (int s : {1, 2, 4}) {
        const cv::Mat a = eng.render(kind, s), b = eng.render(kind, s, kAll, &own);
        CHECK(a.cols == size.width / s && a.rows == size.height / s, "size at scale %d", s);
        CHECK(same(a, b), "last results == explicit records (kind %d scale %d)", kind, s);
      }
    CHECK(!same(eng.render(), rotated), "the last results are drawn");
    bool threw = false;
    try { eng.render(IRMV_RENDER_COLOR, 3); } catch (const std::runtime_error &) { threw = true; }
    CHECK(threw, "scale 3 is refused");
    CHECK(same(eng.render(IRMV_RENDER_COLOR, 1, 0), rotated), "and the engine goes on");
    CHECK(eng.detect() == bboxes, "detect() after render");
  }

  const std::array<double, 9> K = {957.669211, 0, 345.943891, 0, 969.127115, 284.057302, 0, 0, 1};
  const std::vector<double> D = {-0.405274, 0.126058, -0.026939, -0.006503, 0.0};
  IrmDetectorCore::Params prm;
  prm.image_input_size = size;
  prm.net_input_size = cv::Size(64, 64);
  IrmDetectorCore core(argv[1], K, D, prm);
  for (uint8_t * b : core.image_buffers()) std::memcpy(b, frame.data(), frame.size());
  StampedFrame img;
  img.id = 1;
  auto r = core.message_callback(img);
  CHECK(r.visualized_image.empty() && r.binary_image.empty(), "no images without debug");
  CHECK(!core.set_bool_parameter("profiling", true) && core.set_bool_parameter("debug", true) && core.params().debug, "debug is live");
  CHECK(!core.set_parameter("debug_scale", 3) && core.params().debug_scale == 1, "debug_scale 3 is refused");
  for (int s : {1, 2, 4}) {
    CHECK(core.set_parameter("debug_scale", s), "debug_scale %d", s);
    CHECK(core.set_parameter("binary_threshold", 100 + 20 * s), "binary_threshold");
    r = core.message_callback(img);
    CHECK(!r.bboxes.empty(), "core detections");
    YoloEngine & eng = core.engine(img.id);
    int n = 0;
    const irmv_det * last = eng.last_detections(&n);
    const std::vector<irmv_det> own(last, last + n);
    CHECK(r.visualized_image.cols == size.width / s && r.visualized_image.rows == size.height / s, "visualized size at scale %d", s);
    CHECK(same(r.visualized_image, eng.render(IRMV_RENDER_COLOR, s, kAll, &own)), "visualized image at scale %d", s);
    CHECK(same(r.binary_image, eng.render(IRMV_RENDER_BINARY, s, kBoxes, &own, 100 + 20 * s)), "binary image at scale %d", s);
    CHECK(!same(r.binary_image, eng.render(IRMV_RENDER_BINARY, s, kBoxes, &own, 250)), "the threshold matters");
  }
  CHECK(core.set_bool_parameter("debug", false), "debug off");
  r = core.message_callback(img);
  CHECK(r.visualized_image.empty() && r.binary_image.empty() && !r.bboxes.empty(), "no images after debug is off");
  std::printf("render_test fails %d\n", fails);
  return fails ? 1 : 0;
}
