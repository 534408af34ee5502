// The refined point source through the C++ facade (include/irmv_detection/yolo_engine.hpp, irm_detector_core.hpp): the trailing
// constructor argument, set_refine(), refines_points() and has_keypoint_head() of a refined engine, and the core's parameters.
// A plain main(): argv = <model.onnx path> <raw 256x128x3 frame>.  Prints every detection's refine flag and its keypoints as
// bit patterns, for a byte comparison with the Python mirror.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>

#include "irmv_detection/irm_detector_core.hpp"
#include "irmv_detection/yolo_engine.hpp"

int main(int argc, char ** argv)
{
  // the parameters pass through the node's core unchanged (no engine needed for that)
  irmv_detection::IrmDetectorCore::Params params;
  params.point_source = IRMV_POINTS_REFINED;
  params.refine_snap = 0.75;
  params.refine_roi_margin = 6.0;
  if (argc < 3) return params.point_source == 3 && params.refine_snap == 0.75 ? 2 : 4;

  const cv::Size size(256, 128);
  std::vector<uint8_t> frame(size_t(size.width) * size.height * 3);
  std::ifstream f(argv[2], std::ios::binary);
  f.read(reinterpret_cast<char *>(frame.data()), std::streamsize(frame.size()));
  if (!f) return 3;

  irmv_detection::YoloEngine engine(argv[1], size, false, -1, false, 128, IRMV_SRC_HWC8, {256, 256, 256}, 64, IRMV_DEMOSAIC_BILINEAR, {}, cv::Size(-1, -1),
                                    IRMV_POINTS_REFINED);
  std::printf("refines %d keypoint_head %d\n", int(engine.refines_points()), int(engine.has_keypoint_head()));
  std::memcpy(engine.get_src_image_buffer(), frame.data(), frame.size());
  for (int pass = 0; pass < 2; pass++) {
    if (pass == 1) engine.set_refine(float(params.refine_snap), float(params.refine_roi_margin));
    engine.detect();
    int n = 0;
    const irmv_det * dets = engine.last_detections(&n);
    std::printf("pass %d records %d\n", pass, n);
    for (int i = 0; i < n; i++) {
      uint32_t u[8];
      std::memcpy(u, dets[i].kpts, 32);
      std::printf("det %d flag %d lights %d %08x %08x %08x %08x %08x %08x %08x %08x\n", i, dets[i].reserved, dets[i].n_lights, u[0], u[1], u[2], u[3], u[4], u[5],
                  u[6], u[7]);
    }
  }
  return 0;
}
