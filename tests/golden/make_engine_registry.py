"""Writes tests/golden/engine_registry.json: what an engine that enables no optional feature consists of -- the op list (kind,
kernel name), the classified device ranges (name, class, bytes), the graphs it holds after one detect() and the rows of its
profile -- for the engine of tests/test_gpu_pose_cov.py test_a_never_enabled_engine_is_the_recorded_one: a 128 x 64 net on
a 256 x 128 source, the window tests' crafted blob, untimed choices (IRMV_AUTOTUNE=0, IRMV_GROUP_HEAD=0).

    IRMV_LIB_PATH=<build of libirmv_hip.so> python3 tests/golden/make_engine_registry.py [out.json]      (needs the GPU)

The committed file was written by the library of the commit in front of the pose uncertainty, so the
test holds "an engine that never enables it is the engine it was" to a record and not to a second engine of the same build.
A change that alters every engine's ops or ranges on purpose writes the file anew with its own library and says so.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def registry():
    os.environ["IRMV_AUTOTUNE"] = "0"
    os.environ["IRMV_GROUP_HEAD"] = "0"
    import detect_craft as dc
    import mem_residue as MR
    from conftest import K_REF
    from irmv_detection_amd import frames, weights
    from irmv_detection_amd.engine import YoloEngine
    blob = dc.craft(weights.synthetic_blob(0), cls=("shift", 3.0), kpt=("bias", dc.quad_kpt_bias(8)))
    with YoloEngine(None, (256, 128), weights_blob=blob, net_size=128, net_height=64, camera_matrix=tuple(float(v) for v in K_REF)) as e:
        e.get_src_image_buffer(0)[:] = frames.synthetic_frame(12, 256, 128)
        e.detect()
        return dict(ops=[[o.kind.decode(), o.kname.decode()] for o in MR.graph_ops(e)],
                    allocs=[[a["name"], a["cls"], a["bytes"]] for a in e.debug_allocs()],
                    graph_count=e.debug_graph_count(), sync_launch=e.sync_launch, profile=[k["name"] for k in e.profile(0, 1)])


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "engine_registry.json")
    open(out, "w").write(json.dumps(registry(), indent=0) + "\n")
    print("wrote", out)
