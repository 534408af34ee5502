"""The step programs and their model on the CPU (tests/step_programs.py): the generator is deterministic and obeys the
producer rule, the set of programs the GPU test runs covers the alphabet, and the model attributes hand-written programs as
written out here by hand."""
import itertools

import pytest

import step_programs as sp

# the programs tests/test_gpu_step_programs.py runs: step_programs.GPU_CASES at step_programs.LENGTH, and P's two
LENGTH = sp.LENGTH
GPU_SET = {fam: [sp.generate(fam, seed, LENGTH) for seed in sorted({s for f, _, s in sp.GPU_CASES if f == fam})] for fam in "WBC"}
GPU_SET["P"] = [sp.generate_p(0, False), sp.generate_p(0, True)]


def test_generate_is_deterministic():
    for fam in "WBC":
        for seed in (0, 3, 5):
            assert sp.generate(fam, seed, LENGTH) == sp.generate(fam, seed, LENGTH) == GPU_SET[fam][seed]
        assert sp.generate(fam, 0, LENGTH) != sp.generate(fam, 1, LENGTH)
    assert sp.generate("P", 0, LENGTH) == sp.generate_p(0, True) and sp.generate_p(0, False) == GPU_SET["P"][0]


def test_every_program_obeys_the_producer_rule():
    for fam, programs in GPU_SET.items():
        for p in programs:
            assert sp.check_producer_rule(fam, p) == []
            sp.Model(fam).run(p)                    # (raises Illegal on anything the contract leaves undefined)
    # the checker is no tautology: a write moved in front of its wait_upload is found, whoever generated the program
    p = [("write", 0, 1), ("submit", 0, 1, True, True), ("write", 0, 2), ("wait_upload", 0, 1), ("wait_slots", 0, 1)]
    assert sp.check_producer_rule("W", p) == [2]
    p = [("write", 1, 1), ("submit_tiles", 1, 2, 2, True, True), ("wait_slots", 2, 2), ("write", 1, 2)]
    assert sp.check_producer_rule("W", p) == [3]       # (the frame slot lies outside the range that was waited for)
    assert sp.check_producer_rule("W", p[:2] + [("wait_upload", 1, 1), ("write", 1, 2)]) == []
    assert sp.check_producer_rule("W", [("write", 0, 1), ("detect", 0), ("write", 0, 2)]) == []


def test_the_set_covers_the_alphabet():
    kinds = set()
    for fam in "WBC":
        f = sp.FAMILIES[fam]
        cov = sp.coverage(fam, GPU_SET[fam])
        kinds |= cov["kinds"]
        # every setter with a step of its own slot in flight and with only other slots in flight (a setter of the whole engine:
        # with a step in flight, and with none)
        assert cov["inflight"] >= set(itertools.product(f["setters"], ("same", "other"))), fam
        assert cov["pairs"] >= set(itertools.product(f["setters"], f["forms"])), fam
        assert cov["observed"] >= set(f["forms"]), fam
        assert cov["overwritten"] >= {"single", "batched", "tiled"} & set(f["forms"]), fam
        # every policy and every corner of the palettes stands behind a step that is read
        seen = [o["res"][1] for p in GPU_SET[fam] for _, o in sp.Model(fam).run(p) if o["kind"] == "read" and not o["post"]]
        assert {s[2] for s in seen} == set(range(sp.N_POLICY)) and {s[1] for s in seen if s[0] == "window"} >= set(f["corners"]), fam
    cov = sp.coverage("P", GPU_SET["P"])
    kinds |= cov["kinds"]
    assert cov["overwritten"] == {"single"} and cov["observed"] >= {"single"}
    every = set(sp.SETTER_KINDS) | set(sp.STEP_KINDS) | set(sp.WAIT_KINDS) | set(sp.ENTRY_KINDS) | set(sp.READ_KINDS) | {"write", "refused_views", "refused_window"}
    assert every <= kinds


# ---- the model on hand-written programs --------------------------------------------------------------------------------
C0 = (33, 36)                                           # a W slot's window at creation: centred


def st(view="window", corner=C0, policy=0, colour=-1, prior=None, up=0, refine=0, metering=None, isp=0, extract=0):
    return (view, corner, policy, colour, prior, up, refine, metering, isp, extract)


def reads(fam, program, **flags):
    return [o for _, o in sp.Model(fam, **flags).run(program)]


def test_set_window_between_two_async_submits():
    p = [("write", 0, 1), ("submit", 0, 1, True, True), ("set_window", 0, (5, 37)), ("wait_slots", 0, 1), ("read", 0),
         ("submit", 0, 1, True, True), ("wait_slots", 0, 1), ("read", 0)]
    a, b = reads("W", p)
    assert a["res"] == (1, st()) and a["shift"] == (0, 0) and a["stats"] == (1, st())          # the first step keeps the old window
    assert b["res"] == (1, st(corner=(5, 37)))
    a, b = reads("W", p, late_setters=True)
    assert a["res"] == (1, st(corner=(5, 37)))                                                 # (the control's error)
    a, b = reads("W", p, current_corner=True)
    assert a["res"] == (1, st()) and a["shift"] == (5 - 33, 37 - 36) and b["shift"] == (0, 0)


def test_pinned_overwrite_after_wait_upload():
    p = [("write", 2, 4), ("submit", 2, 1, True, True), ("wait_upload", 2, 1), ("write", 2, 5), ("wait_slots", 2, 1), ("read", 2)]
    assert reads("W", p)[0]["res"] == (4, st())                                                # the frame of the submit
    assert reads("W", p, late_frames=True)[0]["res"] == (5, st())
    with pytest.raises(sp.Illegal):
        sp.Model("W").run(p[:2] + p[3:])                                                       # the write without the wait
    # a tiled step reads its frame slot only, and owns it
    t = [("write", 0, 1), ("write", 1, 2), ("set_tiles", 1, ((0, 0), (66, 73))), ("set_tile_merge", 1), ("submit_tiles", 0, 1, 2, True, True),
         ("wait_upload", 0, 1), ("write", 0, 3), ("set_tile_merge", 0), ("wait_slots", 1, 2), ("read_tiles", 1, 2), ("read", 2)]
    tiles, two = reads("W", t)
    assert tiles["parts"] == [(1, st(corner=(0, 0))), (1, st(corner=(66, 73)))] and tiles["merge"] == 1
    assert two["res"] == (1, st(corner=(66, 73))) and two["stats"] is None                     # (a tiled step does not meter)


def test_regrouping():
    w = [("write", s, s) for s in range(4)]
    p = w + [("submit", 0, 4, True, False), ("set_class_policy", 2), ("submit", 1, 1, True, True), ("set_enemy_color", 0), ("submit", 0, 2, True, True),
             ("set_up", 2, 1), ("submit", 1, 2, True, False), ("wait",)] + [("read", s) for s in range(4)]
    r = reads("W", p)
    assert [o["res"] for o in r] == [(0, st(policy=2, colour=0)), (1, st(policy=2, colour=0)), (2, st(policy=2, colour=0, up=1)), (3, st())]
    r = reads("W", p, sticky_groups=True)
    assert [o["res"] for o in r] == [(s, st()) for s in range(4)]                              # (the control's error)


def test_a_step_without_h2d_after_a_render():
    p = [("write", 1, 2), ("set_view", 1, "frame"), ("render", 1), ("write", 1, 3), ("submit", 1, 1, False, False), ("wait_slots", 1, 1), ("read", 1)]
    ren, got = reads("W", p)
    assert ren["res"] == (2, st(view="frame")) and got["res"] == (2, st(view="frame"))          # the loaded frame, not the pinned one
    # an HWC window engine in the window view loads the window's band: readable while the window keeps its rows
    q = [("write", 1, 2), ("set_window", 1, (0, 40)), ("meter", 1), ("set_window", 1, (66, 40)), ("submit", 1, 1, False, False), ("wait_slots", 1, 1), ("read", 1)]
    assert reads("W", q)[1]["res"] == (2, st(corner=(66, 40)))
    with pytest.raises(sp.Illegal):
        sp.Model("W").run(q[:3] + [("set_window", 1, (0, 41))] + q[4:])
    # ... and a window-view step with H2D leaves the device frame unspecified there; a Bayer engine always uploads whole frames
    d = [("write", 0, 1), ("detect", 0), ("write", 0, 2), ("submit", 0, 1, False, False), ("wait_slots", 0, 1), ("read", 0)]
    with pytest.raises(sp.Illegal):
        sp.Model("W").run(d)
    assert reads("B", d)[0]["res"] == (1, st(corner=(33, 37)))


def test_run_post_and_entries_leave_the_rest_alone():
    p = [("set_pose_prior", 0), ("set_metering", 1), ("write", 0, 1), ("detect", 0), ("set_class_policy", 1), ("set_metering", None), ("run_post", 0),
         ("read", 0), ("write", 0, 2), ("rotated", 0), ("read", 0)]
    a, rot, b = reads("W", p)
    step = (1, st(prior=0, metering=1))
    assert a["res"] == step and a["post"] == (step, st(policy=1, prior=0)) and a["stats"] == step
    assert rot["res"] == (2, st(policy=1, prior=0)) and (b["res"], b["post"], b["stats"]) == (a["res"], a["post"], a["stats"])
    with pytest.raises(sp.Illegal):
        sp.Model("W").run(p + [("run_post", 0)])                                              # the entry has replaced the slot's device frame


def test_shrink_keeps_a_failing_core():
    program = next(p for p in GPU_SET["W"] if any(op[0] == "submit_tiles" for op in p))
    target = next(op for op in program if op[0] == "submit_tiles")
    small = sp.shrink("W", program, lambda q: target in q)
    assert target in small and sp.valid("W", small) and len(small) <= 4
