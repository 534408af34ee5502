"""bench.py --dump-outputs: the arrays it writes (no GPU: detections built by hand)."""
import os

import numpy as np

import bench
from irmv_detection_amd.engine import Armor, ArmorClass, ArmorSize, Light


def _armor(k):
    return Armor(left_light=Light(top=(k + 1.0, 2.0), bottom=(k + 3.0, 4.0)), right_light=Light(top=(k + 5.0, 6.0), bottom=(k + 7.0, 8.0)),
                 size=ArmorSize.LARGE, armor_class=ArmorClass.R3, confidence=0.5 + k / 100, bbox_xyxy=(k, 1.0, k + 2.0, 3.0),
                 pnp_ok=True, n_lights=2, rvec=np.array([0.1, 0.2, k]), tvec=np.array([1.0, 2.0, k]), quat_xyzw=np.array([0.0, 0.0, 0.0, 1.0]))


def test_dump_layout(tmp_path):
    slots = [[_armor(0)], [], [_armor(1), _armor(2)]]
    bench.dump_outputs(str(tmp_path), slots, [4, 5, 6], 100)
    got = {n[:-4]: np.load(tmp_path / n) for n in os.listdir(tmp_path)}
    assert set(got) == {"slot", "frame_index", "num_dets", "boxes_xyxy", "scores", "class_id", "image_points", "armor_size",
                        "valid", "n_lights", "pnp_ok", "rvec", "tvec", "quat_xyzw"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert got["num_dets"].tolist() == [1, 0, 2] and got["frame_index"].tolist() == [4, 5, 6] and got["slot"].tolist() == [0, 1, 2]
    assert got["boxes_xyxy"].shape == (3, 100, 4) and got["image_points"].shape == (3, 100, 4, 2)
    assert np.array_equal(got["image_points"][2, 1], _armor(2).image_points())
    assert got["class_id"][2, 0] == int(ArmorClass.R3) and got["armor_size"][0, 0] == int(ArmorSize.LARGE)
    assert got["rvec"].dtype == np.float64 and got["rvec"][2, 1, 2] == 2.0
    assert not got["scores"][1].any() and not got["scores"][0, 1:].any()      # zero past num_dets


def test_dump_is_bounded_and_samples_the_same_slots(tmp_path):
    slots = [[_armor(0)]] * 20000
    bench.dump_outputs(str(tmp_path / "a"), slots, list(range(20000)), 100)
    bench.dump_outputs(str(tmp_path / "b"), slots, list(range(20000)), 100)
    total = sum(os.path.getsize(tmp_path / "a" / n) for n in os.listdir(tmp_path / "a"))
    assert total <= 64 * 1000 * 1000
    s = np.load(tmp_path / "a" / "slot.npy")
    assert 0 < len(s) < 20000 and np.all(np.diff(s) > 0)
    assert np.array_equal(s, np.load(tmp_path / "b" / "slot.npy"))
    assert np.array_equal(np.load(tmp_path / "a" / "frame_index.npy"), s)
