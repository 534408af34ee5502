// Plate numbers through the C++ surface: YoloEngine::set_number_model / set_numbers / plate_numbers / numbers_at
// (include/irmv_detection/yolo_engine.hpp) and IrmDetectorCore's Params::number_model / FrameResult::numbers
// (include/irmv_detection/irm_detector_core.hpp), on a 128 x 96 frame with a 64 x 64 net.
//   * the facade: plate_numbers() is empty before the first set_numbers(true), which needs a model; afterwards it is parallel
//     to the detections and the patches, equal to numbers_at() of those patches, and written to <out file> beside the patches,
//     where the Python test compares both with the C ABI's records and with the host reference
//   * the core: FrameResult::numbers parallel to armors and patches, equal to numbers_at(patches); "number_model" is live
// argv: <model.onnx path (sibling .irmw exists)> <128 x 96 x 3 frame file> <.irmn model file> <out file>
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

template <class F> static bool throws(F && f)
{
  try { f(); } catch (const std::exception &) { return true; }
  return false;
}

static bool same(const std::vector<irmv_plate_number> & a, const std::vector<irmv_plate_number> & b)
{
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(irmv_plate_number)) == 0);
}

static bool all_zero(const std::vector<irmv_plate_number> & a)
{
  const irmv_plate_number z{};
  for (const auto & r : a)
    if (std::memcmp(&r, &z, sizeof z) != 0) return false;
  return true;
}

static int classified(const std::vector<irmv_plate_number> & a)
{
  int n = 0;
  for (const auto & r : a) n += r.state == 1;
  return n;
}

int main(int argc, char ** argv)
{
  if (argc < 5) return 2;
  const cv::Size size(128, 96);
  std::vector<uint8_t> frame(size_t(size.width) * size.height * 3);
  {
    std::ifstream f(argv[2], std::ios::binary);
    f.read(reinterpret_cast<char *>(frame.data()), std::streamsize(frame.size()));
    if (!f) return 3;
  }
  const std::string model = argv[3];
  int n_classes = 0;
  {
    std::vector<float> buf(90384);
    irmv_number_model m;
    CHECK(irmv_number_model_read(model.c_str(), &m, buf.data(), int64_t(buf.size()), nullptr) == IRMV_OK, "the model file reads: %s", irmv_last_error());
    n_classes = m.dims[m.n_layers];
  }

  {
    YoloEngine eng(argv[1], size, false, -1, false, 64);
    std::memcpy(eng.get_src_image_buffer(), frame.data(), frame.size());
    const auto before = eng.detect();
    CHECK(!before.empty(), "detections");
    CHECK(eng.plate_numbers().empty() && eng.plate_patches().empty() && !eng.numbers(), "nothing before the first set");
    CHECK(throws([&] { eng.set_numbers(); }) && !eng.numbers() && eng.plate_numbers().empty(), "set_numbers without a model throws");
    eng.set_numbers(false);
    CHECK(eng.plate_numbers().empty() && eng.plate_patches().empty(), "a first set_numbers(false) changes nothing");
    CHECK(throws([&] { eng.set_number_model(model + ".missing"); }), "a missing model file throws");
    CHECK(throws([&] { eng.numbers_at(std::vector<irmv_plate_patch>(1)); }), "numbers_at without a model throws");
    eng.set_number_model(model);
    eng.set_numbers();
    CHECK(eng.numbers() && eng.patches().enable == 1, "on, and the patches with them");
    CHECK(eng.detect() == before, "the detections do not change");
    int n = 0;
    eng.last_detections(&n);
    const auto patches = eng.plate_patches();
    const auto numbers = eng.plate_numbers();
    CHECK(int(numbers.size()) == n && patches.size() == numbers.size() && n > 0, "parallel to the detections: %zu %zu %d", numbers.size(), patches.size(), n);
    CHECK(classified(numbers) >= 1, "a classified record");
    CHECK(same(eng.numbers_at(patches), numbers), "numbers_at(plate_patches()) == plate_numbers()");
    for (size_t i = 0; i < numbers.size(); i++) {
      const irmv_plate_number & r = numbers[i];
      CHECK(r.state == patches[i].state, "record %zu: the patch's state", i);
      const auto p = YoloEngine::number_softmax(r, n_classes);
      float sum = 0.f;
      int best = 0;
      for (int c = 0; c < 16; c++) { sum += p[size_t(c)]; if (p[size_t(c)] > p[size_t(best)]) best = c; }
      if (r.state == 1) CHECK(std::fabs(sum - 1.f) < 1e-5f && p[size_t(r.label)] == p[size_t(best)], "record %zu: softmax sums to 1 and peaks at the label", i);
      else CHECK(sum == 0.f, "record %zu: no answer, no confidence", i);
    }
    {
      std::ofstream o(argv[4], std::ios::binary);
      const int32_t count = int32_t(numbers.size());
      o.write(reinterpret_cast<const char *>(&count), 4);
      o.write(reinterpret_cast<const char *>(patches.data()), std::streamsize(patches.size() * sizeof(irmv_plate_patch)));
      o.write(reinterpret_cast<const char *>(numbers.data()), std::streamsize(numbers.size() * sizeof(irmv_plate_number)));
      CHECK(bool(o), "the out file");
    }
    eng.set_numbers(false);
    CHECK(!eng.numbers() && eng.plate_numbers().size() == numbers.size() && all_zero(eng.plate_numbers()), "off: the records are zero");
    CHECK(eng.detect() == before && all_zero(eng.plate_numbers()), "... and stay zero");
    CHECK(same(eng.numbers_at(patches), numbers), "numbers_at does not ask whether the op is on");
    eng.set_numbers();
    eng.detect();
    CHECK(same(eng.plate_numbers(), numbers), "on again: the same records");
  }

  const std::array<double, 9> K = {957.669211, 0, 345.943891, 0, 969.127115, 284.057302, 0, 0, 1};
  const std::vector<double> D = {-0.405274, 0.126058, -0.026939, -0.006503, 0.0};
  IrmDetectorCore::Params prm;
  prm.image_input_size = size;
  prm.net_input_size = cv::Size(64, 64);
  StampedFrame img;
  {
    IrmDetectorCore plain(argv[1], K, D, prm);
    for (uint8_t * b : plain.image_buffers()) std::memcpy(b, frame.data(), frame.size());
    img.id = 0;
    auto r = plain.message_callback(img);
    CHECK(!r.armors.empty() && r.numbers.empty() && r.patches.empty(), "no records without Params::number_model");
    CHECK(!plain.set_parameter("number_model", model + ".missing") && plain.params().number_model.empty(), "a missing file is refused");
    CHECK(plain.set_parameter("number_model", std::string("")), "off while off");
    CHECK(plain.set_parameter("number_model", model) && plain.params().number_model == model, "number_model is live");
    r = plain.message_callback(img);
    CHECK(r.numbers.size() == r.armors.size() && classified(r.numbers) >= 1, "... and the next frame carries the records");
  }
  prm.number_model = model;
  IrmDetectorCore core(argv[1], K, D, prm);
  for (uint8_t * b : core.image_buffers()) std::memcpy(b, frame.data(), frame.size());
  for (int id = 0; id < 3; id++) {
    img.id = id;
    const auto r = core.message_callback(img);
    CHECK(!r.armors.empty() && r.numbers.size() == r.armors.size() && r.patches.size() == r.armors.size() && r.poses.size() == r.armors.size(),
          "engine %d: numbers parallel to armors: %zu %zu %zu", id, r.numbers.size(), r.patches.size(), r.armors.size());
    CHECK(classified(r.numbers) >= 1 && same(core.engine(id).numbers_at(r.patches), r.numbers), "engine %d: the records are the patches' numbers", id);
  }
  CHECK(core.set_parameter("number_model", std::string("")) && core.params().number_model.empty(), "off");
  img.id = 2;
  auto r = core.message_callback(img);
  CHECK(r.numbers.size() == r.armors.size() && all_zero(r.numbers) && r.patches.size() == r.armors.size(), "off: no answers, the patches stay");
  CHECK(!core.set_parameter("number_model", 1.0) && !core.set_parameter("patches_model", model), "other names and types are refused");
  std::printf("number_facade_test fails %d\n", fails);
  return fails ? 1 : 0;
}
