// The tiled search through the C++ facade: the lost-target loop of INTEGRATION.md section 9 / 11 written against
// include/irmv_detection/yolo_engine.hpp.  A plain main(): argv = <model.onnx path> <raw 322x201x3 frame>.
// Prints the grid, then every merged detection with its floats as bit patterns, for a byte comparison with the Python mirror.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>

#include "irmv_detection/irm_detector_core.hpp"
#include "irmv_detection/yolo_engine.hpp"

int main(int argc, char ** argv)
{
  if (argc < 3) return 2;
  const cv::Size size(322, 201), window(256, 128), overlap(190, 55);   // 2 x 2 tiles at (0, 0) (66, 0) (0, 73) (66, 73)
  std::vector<uint8_t> frame(size_t(size.width) * size.height * 3);
  std::ifstream f(argv[2], std::ios::binary);
  f.read(reinterpret_cast<char *>(frame.data()), std::streamsize(frame.size()));
  if (!f) return 3;

  irmv_detection::YoloEngine engine(argv[1], size, false, -1, false, 128, IRMV_SRC_HWC8, {256, 256, 256}, 64, IRMV_DEMOSAIC_BILINEAR, window, overlap);
  std::printf("tiles %d grid %d %d\n", engine.num_tiles(), engine.tile_grid().width, engine.tile_grid().height);
  std::memcpy(engine.get_src_image_buffer(), frame.data(), frame.size());

  // the tracker's loop: follow the target in the window; once it is lost, search the SAME frame at the sensor's resolution
  engine.set_window_center(cv::Point2f(161.f, 100.f));
  std::vector<irmv_detection::YoloEngine::bbox> tracked = engine.detect();
  std::vector<irmv_detection::YoloEngine::bbox> found = engine.detect_tiles();
  int n = 0;
  const irmv_tile_det * recs = engine.last_tile_detections(&n);
  std::printf("tracked %zu found %zu records %d\n", tracked.size(), found.size(), n);
  for (int i = 0; i < n; i++) {
    uint32_t u[5];
    std::memcpy(u, found[size_t(i)].xyxy.data(), 16);
    std::memcpy(u + 4, &found[size_t(i)].score, 4);
    std::printf("det %d %08x %08x %08x %08x %08x %d tile %d index %d cut %d\n", i, u[0], u[1], u[2], u[3], u[4], int(found[size_t(i)].class_id),
                recs[i].tile, recs[i].index, recs[i].cut);
  }
  if (!found.empty()) engine.set_window_center(cv::Point2f((found[0].xyxy[0] + found[0].xyxy[2]) / 2, (found[0].xyxy[1] + found[0].xyxy[3]) / 2));
  engine.set_tile_merge(0.4f, 3.0f);
  std::printf("again %zu\n", engine.detect_tiles().size());

  // the parameter passes through the node's core unchanged
  irmv_detection::IrmDetectorCore::Params params;
  params.tile_overlap = overlap;
  return params.tile_overlap.width == 190 ? 0 : 4;
}
