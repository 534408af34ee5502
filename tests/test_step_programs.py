"""The step programs and their model on the CPU (tests/step_programs.py): the generator is deterministic and obeys the
producer rule, the set of programs the GPU test runs covers the alphabet, and the model attributes hand-written programs as
written out here by hand.  Families T and D (rule 7, the track table, and the newer side records): every program holds the
deliberate phrases (a) .. (h), the seeds walk every (new setter, step form) pair, hand-written programs pin the fed log, and a
host simulation -- a Model for an engine, irmv_detection_amd/tracks.py on synthetic armors -- shows that the control program
tells the three wrong models of rule 7 apart before any GPU is asked."""
import hashlib
import itertools

import pytest

import step_programs as sp

# the programs tests/test_gpu_step_programs.py runs: step_programs.GPU_CASES at step_programs.LENGTH, and P's two
LENGTH = sp.LENGTH
GPU_SET = {fam: [sp.generate(fam, seed, LENGTH) for seed in sorted({s for f, _, s in sp.GPU_CASES if f == fam})] for fam in "WBC"}
GPU_SET["P"] = [sp.generate_p(0, False), sp.generate_p(0, True)]
# the tracked families: step_programs.TRACK_CASES
TRACK_SET = {fam: {seed: sp.generate(fam, seed, LENGTH) for seed in sorted({s for f, _, s in sp.TRACK_CASES if f == fam})} for fam in "TD"}
# sha256(repr(program)) of every program the GPU test ran before families T and D existed: they stay the programs they were
OLD_PROGRAMS = {
    ('B', 0): "8cd273f95a3b4a47effa36e4767dcb54d9272137a23a39131f19a561819d6c7d",
    ('B', 1): "e8c9a768811b20d1387b6bf37639521404bb1c2bff5570f0b0ef0c16c2b9b936",
    ('B', 2): "339691c6f9669f3a184292206ce99e715911c2567450203ce171e4fe900fa332",
    ('B', 3): "27d48cdd0e0ebac0831348ad919f145cd2c200cdd6d79023cc07e6c692f66369",
    ('B', 4): "dacf7fb1cddb7223340dab8322414f62eea456d35c1735276e8ada4b33fea39a",
    ('B', 5): "44f59ab5561591359e01b006cf32874e069575bc927e263a33cf4d1989e38d9b",
    ('B', 6): "40f79d4c4ff50de376a72e0e0773d1040278773288d8ad16adaf091d8ffb4f5c",
    ('B', 7): "3ace689105c808837fe829c9215bdebfefdc95e1cc2e815bb8c83e8e0bbef990",
    ('C', 0): "53aa5724ced0c2487a70d0b97b2862b861a2cf2d8dffcc83f8aee1167bb52429",
    ('C', 1): "155e6564de4e86d0ac8f39b432c8f87ddcc5f13a8e7ae8b2fea321d8f28f6fc7",
    ('C', 2): "e656147a4da810fea09bd38575e20613fe27bdc4becae7c60e9773e72b385264",
    ('C', 3): "929b30e228221edac55f2fa6457c2f9dfe485f63ff3e1931e1ddedd0133f37e9",
    ('C', 4): "33092907df8bb81dc9554a1c1cedee4690cc6987ca27bde5d3b35b34173db887",
    ('C', 5): "840b59315bb69efea5bd9f435d9049b0d249aecef484fba803e0ef5bbbd28eb2",
    ('P', 'plain'): "977c13b0bc9e4af57b2536daff77c84ba5c69ed94e2a4168dd49477fa36b9aa2",
    ('P', 'rotated'): "def559dfd67f12c021f79b320100a90ba8216f805b2a831a3e09b7b93563e94a",
    ('W', 0): "df4a5a3a1ba61b0e65f45fbbde219c5eca308baef1c339b6e41dc572f1cb69f4",
    ('W', 1): "5cc8cda3cd78b04152d701142ee4c4864a6f3b58a163cb7d7340da7cea543c5d",
    ('W', 2): "f0cfb3f428c1f51e3660462713401d36ed06dfccdc3b475dc677e815dd634c97",
    ('W', 3): "99664beebce1bd64ecc4e08c6eca07bc41a848e566c52e93a25d945c92d26885",
    ('W', 4): "64d14a550e62ace46df5c1ebfb9e2d1eaef267237b7493b588fd73d9f58098c3",
    ('W', 5): "a8fc5b30893e9d33c43866a13129f19941092c64960c9400a170709671da0db9",
    ('W', 6): "3b4961c7b31320647816eb971ed545af206399d29bf0b49d4aec0bb270c38f02",
    ('W', 7): "561540d2a8dade487ab28d13af8207866cd3ea3b9dcc0707e4a09ae147485ad8",
}


def test_the_old_programs_are_unchanged():
    assert {(f, s) for f, _, s in sp.GPU_CASES} | {("P", "plain"), ("P", "rotated")} == set(OLD_PROGRAMS)
    for (fam, seed), want in OLD_PROGRAMS.items():
        p = sp.generate_p(0, seed == "rotated") if fam == "P" else sp.generate(fam, seed, LENGTH)
        assert hashlib.sha256(repr(p).encode()).hexdigest() == want, (fam, seed)


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
    for fam in "TD":
        kinds |= sp.coverage(fam, TRACK_SET[fam].values())["kinds"]
    assert every <= kinds


# ---- the model on hand-written programs --------------------------------------------------------------------------------
C0 = (33, 36)                                           # a W slot's window at creation: centred


def st(view="window", corner=C0, policy=0, colour=-1, prior=None, up=0, refine=0, metering=None, isp=0, extract=0, yaw=None, cov=None,
       patches=None, numbers=None, tracking=None):
    return (view, corner, policy, colour, prior, up, refine, metering, isp, extract, yaw, cov, patches, numbers, tracking)


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


# ---- families T and D: rule 7 and the newer side records -------------------------------------------------------------------
def test_tracked_programs_are_deterministic_and_obey_the_producer_rule():
    for fam in "TD":
        for seed, p in TRACK_SET[fam].items():
            assert sp.generate(fam, seed, LENGTH) == p and len(p) >= LENGTH
            assert sp.check_producer_rule(fam, p) == [], (fam, seed)
            sp.Model(fam).run(p)
        assert TRACK_SET[fam][0] != TRACK_SET[fam][1]
    # the waits of the new setters count for the producer rule: the slot's own for set_stamp, everything for set_pose_cov
    p = [("set_tracking", 1), ("write", 0, 1), ("write", 1, 1), ("submit", 0, 2, True, True), ("set_stamp", 0, 1), ("write", 0, 2), ("write", 1, 2)]
    assert sp.check_producer_rule("T", p) == [6]
    assert sp.check_producer_rule("T", p[:4] + [("set_pose_cov", 2)] + p[5:]) == []
    with pytest.raises(sp.Illegal):
        sp.Model("T").run(p)                                     # (the model agrees: slot 1 may still be read)
    # ... but three calls return at once on an engine that never enabled the feature: set_stamp and reset_tracks before the
    # first set_tracking, set_numbers(off) before the first set_numbers(on); rule and model agree
    for quick in (("set_stamp", 0, 1), ("reset_tracks",), ("set_numbers", 0)):
        q = [("write", 0, 1), ("submit", 0, 1, True, True), quick, ("write", 0, 2)]
        assert sp.check_producer_rule("T", q) == [3], quick
        with pytest.raises(sp.Illegal):
            sp.Model("T").run(q)
        assert sp.check_producer_rule("T", [("set_tracking", 1), ("set_numbers", 1)] + q) == [], quick


def test_every_tracked_program_holds_every_phrase():
    """(a) .. (h) in every T program; (a), (b), (e), (g) in every D program."""
    for fam in "TD":
        want = set().union(*(sp.PHRASE_PARTS[c] for c in sp.FAMILIES[fam]["track_phrases"]))
        for seed, p in TRACK_SET[fam].items():
            assert want <= sp.track_phrases(fam, p), (fam, seed, sorted(want - sp.track_phrases(fam, p)))
            kinds = [o["track"][0] for _, o in sp.Model(fam).run(p) if o["kind"] == "read"]
            assert kinds.count("fed") >= 20 and kinds.count("refused") >= 1 and (fam == "D" or kinds.count("zero") >= 1), (fam, seed)


def test_the_phrase_detector_misses_a_phrase_the_generator_leaves_out(monkeypatch):
    """The detector is no tautology: with one letter taken out of the family's list, the programs of all eight seeds no
    longer show it.  (e) is left out of this: the stamps the generator gives every step make it on their own; and the
    systematic set_pose_cov phrases happen to make (g)'s shape in one seed."""
    keep = sp.FAMILIES["T"]["track_phrases"]
    for letter in "abcdfgh":
        monkeypatch.setitem(sp.FAMILIES["T"], "track_phrases", keep.replace(letter, ""))
        still = [seed for seed in TRACK_SET["T"] if sp.PHRASE_PARTS[letter] <= sp.track_phrases("T", sp.generate("T", seed, LENGTH))]
        assert len(still) <= (1 if letter == "g" else 0), (letter, still)


def test_the_phrase_detector_on_hand_written_programs():
    w = [("set_tracking", 1), ("write", 0, 1), ("write", 1, 1), ("write", 3, 1), ("set_stamp", 0, 1), ("set_stamp", 1, 2), ("set_stamp", 3, 3)]
    # (h): the detect directly behind the asynchronous submit, on another stream (T: slot mod 3)
    assert "h" in sp.track_phrases("T", w + [("submit", 0, 1, True, True), ("detect", 1)])
    assert "h" not in sp.track_phrases("T", w + [("submit", 0, 1, True, True), ("detect", 3)])                    # slots 0 and 3 share stream 0
    assert "h" not in sp.track_phrases("T", w + [("submit", 0, 1, True, False), ("detect", 1)])                   # (the phrase's submit uploads asynchronously too)
    assert "h" not in sp.track_phrases("T", w + [("detect", 3), ("submit", 0, 1, True, True), ("run_post", 3), ("read", 3), ("set_stamp", 1, 4), ("detect", 1)])
    assert "h" not in sp.track_phrases("T", w + [("submit", 0, 1, True, True), ("wait_slots", 0, 1), ("detect", 1)])
    # (c): a fed step still in flight in front of the tiled step, a fed step behind it
    c = w + [("submit", 0, 1, True, True), ("submit_tiles", 1, 2, 2, True, True), ("submit", 1, 1, True, True)]
    assert "c" in sp.track_phrases("T", c)
    assert "c" not in sp.track_phrases("T", c[:8] + [("wait",)] + c[8:])                                          # the first step was waited for
    assert "c" not in sp.track_phrases("T", [("set_stamp", 1, 0) if op == ("set_stamp", 1, 2) else op for op in c])   # the step behind is refused
    # (c'): run_post between two fed steps
    r = w + [("detect", 0), ("run_post", 0), ("detect", 1)]
    assert "c'" in sp.track_phrases("T", r) and "c'" not in sp.track_phrases("T", r[:-1] + [("detect", 0)])       # (slot 0's stamp did not rise)
    # (g): off, on, the other sigma_px, a fed step of one slot on one frame behind each
    g = [("set_tracking", 1), ("write", 0, 1)] + [x for v in (0, 1, 2) for x in (("set_pose_cov", v), ("set_stamp", 0, v + 1), ("detect", 0))]
    assert "g" in sp.track_phrases("T", g)
    assert "g" not in sp.track_phrases("T", [op for op in g if op != ("set_stamp", 0, 2)])                        # the middle step is refused
    assert "g" not in sp.track_phrases("T", [("set_pose_cov", 1) if op == ("set_pose_cov", 2) else op for op in g])


def test_the_seeds_walk_every_new_setter_and_form():
    for fam, seeds in (("T", range(6)), ("D", range(6))):            # (T: the default form's seeds alone)
        f = sp.FAMILIES[fam]
        cov = sp.coverage(fam, [TRACK_SET[fam][s] for s in seeds])
        assert cov["pairs"] >= set(itertools.product(f["walk"], f["forms"])), (fam, sorted(set(itertools.product(f["walk"], f["forms"])) - cov["pairs"]))
        assert cov["inflight"] >= set(itertools.product(f["walk"], ("same", "other"))), fam
        assert cov["observed"] >= set(f["forms"]) and cov["kinds"] >= set(f["walk"]), fam
        seen = [o["res"][1] for s in seeds for _, o in sp.Model(fam).run(TRACK_SET[fam][s]) if o["kind"] == "read"]
        assert {x[11] for x in seen} == {0, 1, 2} and {x[10] for x in seen} == {0, 1} and {x[12] for x in seen} == {0, 1} and {x[14] for x in seen} >= {1, 2}, fam
        assert fam == "D" or 0 in {x[14] for x in seen}              # (T steps while tracking is off, in phrase (f))
        assert fam == "D" or {x[13] for x in seen} == {0, 1}


PRE = [("set_tracking", 1)]               # all a hand-written program needs for the log: the other channels stay "never enabled"
S1 = st(view="window", tracking=1)


def tracks_of(program, fam="T", **flags):
    m = sp.Model(fam, **flags)
    return [o["track"] for _, o in m.run(program) if o["kind"] == "read"], m.log()


def test_the_log_is_in_submit_order():
    p = PRE + [("write", 0, 4), ("write", 1, 5), ("set_stamp", 1, 1), ("set_stamp", 0, 2), ("submit", 1, 1, True, True), ("submit", 0, 1, True, True),
               ("wait",), ("read", 0), ("read", 1)]
    tr, log = tracks_of(p)
    assert tr == [("fed", 0, 1), ("fed", 0, 0)] and log == [[(5, S1, 1, 0, False), (4, S1, 2, 0, False)]]
    tr, log = tracks_of(p, tracks_by_slot=True)                                                 # (the control's error: slot 1 last, and refused)
    assert tr == [("fed", 0, 0), ("refused", 0, 1, 1)]


def test_a_stale_stamp_inside_a_batch_is_refused_and_keeps_its_place():
    """Slot order inside a submit, and the middle slot's stamp below (then equal to) the first one's."""
    p = PRE + [("write", s, s) for s in range(3)] + [("set_stamp", 0, 5), ("set_stamp", 1, 4), ("set_stamp", 2, 6), ("submit", 0, 3, True, False),
                                                    ("wait",), ("read", 1)]
    tr, log = tracks_of(p)
    assert tr == [("refused", 0, 1, 4)] and [(e[0], e[2], e[4]) for e in log[0]] == [(0, 5, False), (1, 4, True), (2, 6, False)]
    tr, log = tracks_of(p, refused_feeds=True)                                                  # (the control's error)
    assert tr == [("fed", 0, 1)] and [e[2] for e in log[0]] == [5, 5.5, 6]
    q = [("set_stamp", 1, 5) if op == ("set_stamp", 1, 4) else op for op in p]                 # an equal stamp is refused too
    assert tracks_of(q)[0] == [("refused", 0, 1, 5)]
    assert sp.track_phrases("T", p) & {"d<", "d="} == {"d<"} and sp.track_phrases("T", q) & {"d<", "d="} == {"d="}


def test_reset_tracks_waits_and_cuts():
    """The read behind it needs no wait of its own; the epoch's first stamp may lie below the last one's."""
    p = PRE + [("write", 0, 1), ("set_stamp", 0, 5), ("submit", 0, 1, True, True), ("reset_tracks",), ("read", 0), ("set_stamp", 0, 1), ("detect", 0),
               ("read", 0)]
    tr, log = tracks_of(p)
    assert tr == [("fed", 0, 0), ("fed", 1, 0)] and [len(e) for e in log] == [1, 1]


def test_set_stamp_waits_for_its_own_slot_only():
    p = PRE + [("write", 0, 1), ("write", 1, 2), ("submit", 0, 2, True, True), ("set_stamp", 0, 3), ("read", 0)]
    assert tracks_of(p)[0] == [("fed", 0, 0)]
    with pytest.raises(sp.Illegal):
        sp.Model("T").run(p + [("read", 1)])


def test_set_tracking_off_zeroes_and_cuts_and_other_options_keep_the_table():
    p = PRE + [("write", 0, 1), ("set_stamp", 0, 1), ("detect", 0), ("set_tracking", 2), ("set_stamp", 0, 2), ("detect", 0), ("read", 0),
               ("set_tracking", 0), ("read", 0)]
    tr, log = tracks_of(p)
    assert tr == [("fed", 0, 1), ("zero",)] and [e[1][14] for e in log[0]] == [1, 2]
    p = PRE + [("write", 0, 1), ("detect", 0), ("set_tracking", 0), ("detect", 0), ("read", 0), ("set_tracking", 1), ("read", 0), ("detect", 0), ("read", 0)]
    tr, log = tracks_of(p)
    assert tr == [("zero",), ("zero",), ("fed", 1, 0)] and [len(e) for e in log] == [1, 1]       # (a step while it is off feeds nothing)


def test_a_tiled_step_and_run_post_do_not_feed():
    p = PRE + [("write", 0, 1), ("detect", 0), ("submit_tiles", 0, 1, 2, True, False), ("wait",), ("read", 1), ("run_post", 0), ("read", 0)]
    assert tracks_of(p)[0] == [("zero",), ("zero",)] and len(tracks_of(p)[1][0]) == 1
    tr, log = tracks_of(p, skips_feed=True)                                                     # (the control's error)
    assert tr[0][0] == "refused" and len(log[0]) == 4


def test_a_disabling_setter_zeroes_its_channel_of_every_slot():
    """set_pose_cov(off) and set_numbers(off), at once; the slot's next step writes the channel again."""
    p = [("set_pose_cov", 1), ("set_numbers", 1), ("write", 0, 1), ("detect", 0), ("set_numbers", 0), ("set_pose_cov", 0), ("set_pose_cov", 2), ("read", 0),
         ("detect", 0), ("read", 0)]
    a, b = reads("T", p)
    assert a["wiped"] == {"covs", "numbers"} and a["res"][1][11:14] == (1, None, 1) and b["wiped"] == frozenset() and b["res"][1][11:14] == (2, None, 0)
    # never enabled: no track records at all
    assert tracks_of([("write", 0, 1), ("detect", 0), ("read", 0)], "W") == ([None], [[]])


def test_shrink_keeps_a_planted_track_failure():
    """The failure: 'some read reports a refused step'.  What is left still has it, and is a fraction of the program."""
    p = TRACK_SET["T"][1]
    fails = lambda q: any(o["kind"] == "read" and o["track"] and o["track"][0] == "refused" for _, o in sp.Model("T").run(q))   # noqa: E731
    small = sp.shrink("T", p, fails)
    assert fails(small) and sp.valid("T", small) and len(small) <= 12, small


# ---- the host simulation: the whole comparison with a Model for an engine and tracks.py on synthetic armors ---------------------
def test_the_simulation_runs_every_case_and_is_not_vacuous():
    """The whole comparison -- model, log, replay, expected bytes -- on every T and D program: it is deterministic, and the
    reads of a program show at least six different track records."""
    for fam in "TD":
        for seed, p in TRACK_SET[fam].items():
            a, b = sp.simulate(fam, p), sp.simulate(fam, p)
            assert a == b and len({x[4] for x in a}) >= 6, (fam, seed)


def test_the_control_program_tells_the_wrong_models_apart():
    p = sp.generate("T", sp.CONTROL_SEED, sp.CONTROL_LENGTH)
    right = sp.simulate("T", p)
    for flag in ("tracks_by_slot", "skips_feed", "refused_feeds"):
        wrong = sp.simulate("T", p, **{flag: True})
        assert [x[:4] for x in wrong] == [x[:4] for x in right], flag        # the per-frame attribution is the contract's ...
        assert [x[4] for x in wrong] != [x[4] for x in right], flag          # ... the track records are not
    for flag in ("late_setters", "late_frames", "sticky_groups", "current_corner"):
        assert sp.simulate("T", p, **{flag: True}) != right, flag
