// irmv_detection::ArmorTracker -- the armor tracker stand-alone on explicit observations (include/irmv_hip.h, "armor tracks";
// irmv_tracker_*): persistent ids, a constant-velocity Kalman filter per armor in a world frame, gated greedy association and a
// track life cycle, one kernel launch per frame.  IrmDetectorCore feeds one with every frame's poses, in frame order, because
// its three engines each see every third frame; a caller with one engine asks the engine itself (YoloEngine::set_tracking).
#pragma once

#include <array>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#include "irmv_hip.h"

namespace irmv_detection
{
class ArmorTracker
{
public:
  struct Result
  {
    std::vector<irmv_det_track> det_tracks;   // parallel to the observations
    irmv_track_frame frame{};
    std::vector<irmv_track> tracks;           // IRMV_TRACK_CAP entries, free ones included
  };

  // The library's defaults, enabled
  static irmv_track_opts default_opts()
  {
    irmv_track_opts o{};
    irmv_track_default_opts(&o);
    o.enable = 1;
    return o;
  }

  // `device`: HIP ordinal, -1 = IRMV_DEVICE or 0 (as PnPSolver's)
  explicit ArmorTracker(const irmv_track_opts & o = default_opts(), int device = -1)
  {
    if (device < 0) {
      const char * v = std::getenv("IRMV_DEVICE");
      device = v ? std::atoi(v) : 0;
    }
    if (irmv_tracker_create(device, &o, &tracker_) != IRMV_OK)
      throw std::runtime_error(std::string("ArmorTracker: ") + irmv_last_error());
  }
  ~ArmorTracker() { irmv_tracker_destroy(tracker_); }
  ArmorTracker(const ArmorTracker &) = delete;
  ArmorTracker & operator=(const ArmorTracker &) = delete;

  // One frame at stamp t (seconds) under the camera pose in the world (nullptr: identity, zero).  A stamp that does not rise is
  // a result (frame.state == -2), not an error.
  Result update(double t, const std::vector<irmv_track_obs> & obs, const std::array<double, 9> * R_wc = nullptr,
                const std::array<double, 3> * t_wc = nullptr)
  {
    Result r;
    r.det_tracks.resize(obs.size());
    r.tracks.resize(IRMV_TRACK_CAP);
    if (irmv_tracker_update(tracker_, t, R_wc ? R_wc->data() : nullptr, t_wc ? t_wc->data() : nullptr, obs.data(), static_cast<int>(obs.size()),
                            r.det_tracks.data(), &r.frame, r.tracks.data()) != IRMV_OK)
      throw std::runtime_error(std::string("ArmorTracker::update: ") + irmv_last_error());
    return r;
  }

  void reset()
  {
    if (irmv_tracker_reset(tracker_) != IRMV_OK) throw std::runtime_error(std::string("ArmorTracker::reset: ") + irmv_last_error());
  }

  // What the tracker reads of a detection record, and of its pose covariance where there is one
  static irmv_track_obs observation(const irmv_det & d, const irmv_pose_cov * c = nullptr)
  {
    irmv_track_obs o{};
    o.class_id = d.class_id;
    o.valid = (d.pnp_ok == 1 && d.armor_valid == 1) ? 1 : 0;
    for (int i = 0; i < 3; i++) o.tvec[i] = d.tvec[i];
    if (c && c->state == 1) {
      // rows and columns 3 .. 5 of the 6 x 6 whose upper triangle cov[21] holds row-major
      static const int at[3][3] = {{15, 16, 17}, {16, 18, 19}, {17, 19, 20}};
      o.has_cov = 1;
      for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) o.cov[3 * i + j] = c->cov[at[i][j]];
    }
    return o;
  }

private:
  irmv_tracker * tracker_ = nullptr;
};
}  // namespace irmv_detection
