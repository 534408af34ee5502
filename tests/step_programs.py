"""Seeded step programs and the host model of the engine's ordering contract (numpy only; DESIGN.md, "ordering contract").

A PROGRAM is a list of operations on one engine, each a tuple (kind, args...).  generate(family, seed, length) is
deterministic.  A Model replays a program on the host and says, for every OBSERVATION (an operation that reads something
back), which inputs the observed step saw: it computes no detection, only the attribution

    (frame seed, (view, corner, policy, colour, prior, up, refine, metering, isp, extract, yaw, cov, patches, numbers, tracking))

and, for the armor tracks, which cannot be attributed to one frame, the FED LOG (rule 7 below).

The rules (the engine's promises):
  1. a step sees the live state as of its submit; a setter issued while it is in flight reaches the slot's NEXT step;
  2. a step with H2D sees the pinned slot as of its submit, as long as the producer writes the slot again only after
     wait_upload / wait_slots / wait on it has returned (check_producer_rule verifies every program; the generator writes
     right after wait_upload, in front of wait_slots);
  3. a step without H2D sees the device frame: what the last whole upload put there -- a step with H2D in the frame view, of
     a Bayer or a plain engine, a tiled step's frame slot -- or what an on-demand entry loaded (the band of the window it had
     then, on an HWC window engine in the window view).  A window-view step with H2D of an HWC window engine leaves the
     device frame UNSPECIFIED (it may upload a band, or nothing), so no program reads it afterwards without a load;
  4. results, pose_alts and frame_stats of a slot are those of its last step whatever the grouping that step came in; the
     merged tile list that of the last tiled step with that first slot; frame_stats that of the last ORDINARY step (a tiled
     step and run_post do not meter); window-view results carry the corner they were submitted with;
  5. an on-demand entry (render, meter, rotated image, extract_armors, refine_points) sees the pinned slot, the view and the
     window as they are at the call, after the slot's step in flight has finished, and leaves the slot's results alone;
  7. the track table advances in SUBMIT order, and in slot order inside a multi-slot submit.  The model keeps the fed log: per
     EPOCH the list of (frame, state, stamp, pose) of the ordinary steps submitted while tracking was on, in that order.
     reset_tracks and set_tracking(off) cut it (a new epoch with an empty table; the id counter carries over); set_tracking
     with other options while tracking is on keeps the table (include/irmv_hip.h: only enable = 0 clears it), so the log goes
     on and every entry carries, in its state, the options it was fed under.  A step whose stamp does not rise above the
     table's is REFUSED: it keeps its place in the log and the steps around it are as if it had not been.  A tiled step and
     run_post do not feed and zero their slots' two track records; set_tracking(off) zeroes those of every slot (as
     set_pose_cov(off) and set_numbers(off) zero their channel of every slot: a read's `wiped`, until the slot's next step).  A read
     carries track = ("fed", epoch, k) | ("refused", epoch, k, stamp) | ("zero",) | None (tracking never enabled), and
     Model.log() gives, per epoch, the resolved entries (frame, state, stamp, pose, refused).
     Waits: set_stamp and set_camera_pose wait for their slot (once set_tracking was called); set_tracking, reset_tracks, set_yaw_solve, set_pose_cov,
     set_patches and set_numbers for the whole engine -- afterwards nothing (of the slot) is in flight.

Operations:
  ("write", slot, seed)                                   a palette frame into the pinned slot
  ("set_window" | "set_window_center", slot, (x, y))      ("set_view", slot, "frame" | "window")
  ("set_class_policy", i)  ("set_enemy_color", c)         ("set_pose_prior", i)  ("set_up", slot, i)
  ("set_refine", i)  ("set_metering", i)  ("set_bayer_isp", i)  ("set_extract_params", i)
  ("set_tiles", first, (corner, ...))  ("set_tile_merge", i)
  ("set_pose_cov", i)  0: off, 1 | 2: two sigma_px      ("set_yaw_solve", i)  ("set_patches", i)  two parameter sets each
  ("set_numbers", i)  0: off, 1: on                     ("set_tracking", i)  0: off, 1 | 2: two option sets
  ("reset_tracks",)   ("set_stamp", slot, k)  k: a tick of the program-wide clock   ("set_camera_pose", slot, i)
  ("detect", slot)  ("submit", first, count, h2d, async)  ("submit_tiles", frame_slot, first, count, h2d, async)
  ("run_post", slot)
  ("wait",)  ("wait_slots", first, count)  ("wait_upload", first, count)
  ("render" | "meter" | "rotated" | "extract" | "refine_points" | "read_head", slot)
  ("refused_views", first, count)  ("refused_window", slot, (x, y))
  ("read", slot)  ("read_tiles", first, count)
"""
import random

NEW_SETTERS = ("set_pose_cov", "set_yaw_solve", "set_patches", "set_numbers", "set_tracking", "reset_tracks", "set_stamp", "set_camera_pose")
FAMILIES = {
    # HWC window engine, keypoint source; pose prior and metering switched on by the program's first operations
    "W": dict(slots=4, streams=2, full=(322, 201), win=(256, 128), window=True, bayer=False, band=True,
              corners=((0, 0), (66, 73), (31, 40), (5, 37)),
              setters=("set_window", "set_window_center", "set_view", "set_class_policy", "set_enemy_color", "set_pose_prior", "set_up",
                       "set_metering", "set_tiles", "set_tile_merge"),
              forms=("detect", "single", "batched", "tiled"),
              entries=("render", "meter", "rotated", "extract", "refine_points"),
              preamble=(("set_pose_prior", 0), ("set_metering", 0))),
    # Bayer (mhc) window engine, refined point source
    "B": dict(slots=3, streams=0, full=(322, 202), win=(256, 128), window=True, bayer=True, band=False,
              corners=((0, 0), (66, 74), (31, 41), (5, 37)),
              setters=("set_window", "set_window_center", "set_view", "set_class_policy", "set_enemy_color", "set_refine", "set_bayer_isp",
                       "set_tiles", "set_tile_merge"),
              forms=("detect", "single", "batched", "tiled"),
              entries=("render", "meter", "rotated", "extract", "refine_points"), preamble=()),
    # plain engine, bbox-only blob, classical point source: observed through extract_armors and the rotated image too
    "C": dict(slots=5, streams=2, full=(322, 201), win=None, window=False, bayer=False, band=False, corners=(),
              setters=("set_class_policy", "set_enemy_color", "set_extract_params"), forms=("detect", "single", "batched"),
              entries=("extract", "rotated"), preamble=()),
    # plain engine at the real size: the producer contract only (generate_p)
    "P": dict(slots=3, streams=0, full=(1280, 1024), win=None, window=False, bayer=False, band=False, corners=(),
              setters=(), forms=("single",), entries=("rotated",), preamble=()),
    # W's engine on three streams with every side record and the tracker on: the systematic phrases walk the NEW setters
    "T": dict(slots=4, streams=3, full=(322, 201), win=(256, 128), window=True, bayer=False, band=True,
              corners=((0, 0), (66, 73), (31, 40), (5, 37)),
              setters=("set_window", "set_window_center", "set_view", "set_class_policy", "set_enemy_color", "set_pose_prior", "set_up",
                       "set_metering", "set_tiles", "set_tile_merge") + NEW_SETTERS,
              walk=NEW_SETTERS, forms=("detect", "single", "batched", "tiled"),
              entries=("render", "meter", "rotated", "extract", "refine_points"),
              preamble=(("set_pose_prior", 0), ("set_metering", 0), ("set_yaw_solve", 0), ("set_pose_cov", 1), ("set_patches", 0),
                        ("set_numbers", 1), ("set_tracking", 1)),
              track_phrases="abcdefgh"),
    # C's engine (device records copied out) with yaw solve, covariance, patches and the tracker on
    "D": dict(slots=5, streams=2, full=(322, 201), win=None, window=False, bayer=False, band=False, corners=(),
              setters=("set_class_policy", "set_enemy_color", "set_extract_params") + tuple(k for k in NEW_SETTERS if k != "set_numbers"),
              walk=tuple(k for k in NEW_SETTERS if k != "set_numbers"), forms=("detect", "single", "batched"),
              entries=("extract", "rotated"),
              preamble=(("set_yaw_solve", 0), ("set_pose_cov", 1), ("set_patches", 0), ("set_tracking", 1)),
              track_phrases="abeg"),
}
SEEDS = tuple(range(6))                 # frame palette: indices into the GPU module's list of synthetic frames
N_POLICY, N_PRIOR, N_UP, N_REFINE, N_METERING, N_ISP, N_EXTRACT, N_MERGE = 4, 3, 3, 2, 3, 2, 2, 2
N_COV, N_YAW, N_PATCHES, N_NUMBERS, N_TRACKING, N_POSE = 3, 2, 2, 2, 3, 3        # (index 0 of cov, numbers, tracking: off)
COLOURS = (-1, 0)
LENGTH = 60                             # operations per program of the GPU test, at least
LAUNCH_FORMS = ("default", "eager", "graph", "no_graph_upload", "no_window_upload", "inline_copies", "no_zero_copy")
# the GPU test's cases: six seeds per family under the default launch form, two more of W and B under each other one
GPU_CASES = [(f, "default", s) for f in "WBC" for s in range(6)] + [(f, form, s) for f in "WB" for form in LAUNCH_FORMS[1:] for s in (6, 7)]
# the tracked families: T under the default form on six seeds and two more under each other form; D on four seeds, two more
# with device records for the results too
TRACK_CASES = ([("T", "default", s) for s in range(6)] + [("T", form, s) for form in LAUNCH_FORMS[1:] for s in (6, 7)]
               + [("D", "default", s) for s in range(4)] + [("D", "no_zero_copy", s) for s in (4, 5)])
PHRASES = 6                             # systematic phrases per program, at least
CONTROL_SEED, CONTROL_LENGTH = 0, 60    # the W program the GPU test's controls run on
PER_SLOT = ("set_window", "set_window_center", "set_view", "set_up", "set_tiles", "set_stamp", "set_camera_pose")
WAIT_SLOT_SETTERS = ("set_stamp", "set_camera_pose")                                   # wait for their slot
WAIT_ALL_SETTERS = ("set_tracking", "reset_tracks", "set_yaw_solve", "set_pose_cov", "set_patches", "set_numbers")   # for the whole engine
NEW_GLOBAL = {"set_pose_cov": "cov", "set_yaw_solve": "yaw", "set_patches": "patches", "set_numbers": "numbers", "set_tracking": "tracking"}
STEP_KINDS = ("detect", "submit", "submit_tiles", "run_post")
WAIT_KINDS = ("wait", "wait_slots", "wait_upload")
ENTRY_KINDS = ("render", "meter", "rotated", "extract", "refine_points", "read_head")
READ_KINDS = ("read", "read_tiles")
SETTER_KINDS = ("set_window", "set_window_center", "set_view", "set_class_policy", "set_enemy_color", "set_pose_prior", "set_up", "set_refine",
                "set_metering", "set_bayer_isp", "set_extract_params", "set_tiles", "set_tile_merge") + NEW_SETTERS


class Illegal(Exception):
    """The program asks for something the contract does not define (a generator or shrinker error, never an engine's)."""


def form_of(op):
    """The step form of a step operation: detect, single (asynchronous), batched, tiled; None for the other steps."""
    if op[0] == "detect":
        return "detect"
    if op[0] == "submit_tiles":
        return "tiled"
    if op[0] == "submit":
        return "batched" if op[2] > 1 else ("single" if op[4] else None)
    return None


def step_slots(op):
    """(result slots, pinned slots read) of a step operation."""
    if op[0] == "detect":
        return [op[1]], [op[1]]
    if op[0] == "submit":
        r = list(range(op[1], op[1] + op[2]))
        return r, (r if op[3] else [])
    if op[0] == "submit_tiles":
        return list(range(op[2], op[2] + op[3])), ([op[1]] if op[4] else [])
    if op[0] == "run_post":
        return [op[1]], []
    return [], []


def setter_slots(op, n):
    """The slots whose next step a setter reaches."""
    if op[0] == "set_tiles":
        return list(range(op[1], op[1] + len(op[2])))
    return [op[1]] if op[0] in PER_SLOT else list(range(n))


class Model:
    """The contract.  The keyword flags each break one rule (the GPU test's controls); all False: the contract.  The three
    of rule 7: tracks_by_slot -- within a run of submits with no wait between them the log is ordered by slot index, not by
    submit; skips_feed -- tiled steps and run_post append to the log; refused_feeds -- a refused step still advances the table
    (at a stamp half a tick above the table's)."""

    def __init__(self, family, late_setters=False, late_frames=False, sticky_groups=False, current_corner=False, tracks_by_slot=False,
                 skips_feed=False, refused_feeds=False):
        f = self.fam = FAMILIES[family]
        n = self.n = f["slots"]
        self.flags = dict(late_setters=late_setters, late_frames=late_frames, sticky_groups=sticky_groups, current_corner=current_corner,
                          tracks_by_slot=tracks_by_slot, skips_feed=skips_feed, refused_feeds=refused_feeds)
        self.stamp = [None] * n          # the slot's stamp: a clock tick; None: never set (0.0 on the engine)
        self.pose = [0] * n              # the slot's camera pose: a palette index
        self.wiped = [frozenset()] * n   # the side records ("covs", "numbers") a disabling setter zeroed since the slot's last step
        self.trk = [None] * n            # the slot's track records: None (never enabled) | "zero" | (epoch, entry)
        self.epochs = [[]]               # the fed log: per epoch its entries dict(slot, frame, state, k, pose, group), in table order
        self.run_start = 0               # where, in the present epoch, the present run of unwaited submits begins
        self.pinned = [None] * n
        centre = ((f["full"][0] - f["win"][0]) // 2, (f["full"][1] - f["win"][1]) // 2) if f["window"] else (0, 0)
        self.corner = [centre] * n
        self.view = ["window" if f["window"] else "frame"] * n
        self.up = [0] * n
        self.glob = dict(policy=0, colour=-1, prior=None, refine=0, metering=None, isp=0, extract=0, merge=0,
                         yaw=None, cov=None, patches=None, numbers=None, tracking=None)      # (None: never enabled)
        self.dev = [None] * n            # None | ("whole", seed) | ("band", seed, y0)
        self.last = [None] * n           # the slot's last step: dict(kind, frame, state, h2d, src, group)
        self.stats = [None] * n          # (frame, state) of its last ordinary step
        self.tiles = {}                  # first -> dict(parts=[(frame, state)...], merge, src, h2d)
        self.inflight = set()            # slots with a step no wait has covered
        self.busy = set()                # pinned slots an upload may still read
        self.clean = [False] * n         # head and device frame still those of the last ordinary step, in its view and window
        self.first_group = [None] * n

    # ---- state ------------------------------------------------------------------------------------------------------------
    def state(self, s):
        g = self.glob
        return (self.view[s], self.corner[s], g["policy"], g["colour"], g["prior"], self.up[s], g["refine"], g["metering"], g["isp"], g["extract"],
                g["yaw"], g["cov"], g["patches"], g["numbers"], g["tracking"])

    # ---- tracks (rule 7) --------------------------------------------------------------------------------------------------
    def tracking_on(self):
        return self.glob["tracking"] not in (None, 0)

    def _feed(self, slots, frame_of, group):
        """An ordinary step of `slots` (a tiled step or run_post under skips_feed) joins the log, in slot order."""
        e = self.epochs[-1]
        for s in slots:
            ent = dict(slot=s, frame=frame_of(s), state=self.state(s), k=self.stamp[s], pose=self.pose[s], group=group)
            e.append(ent)
            self.trk[s] = (len(self.epochs) - 1, ent)
        if self.flags["tracks_by_slot"]:
            e[self.run_start:] = sorted(e[self.run_start:], key=lambda x: x["slot"])      # (stable: a slot's own steps keep their order)

    def _no_feed(self, slots, frame_of, group):
        if not self.tracking_on():
            return
        if self.flags["skips_feed"]:
            self._feed(slots, frame_of, group)
        else:
            for s in slots:
                self.trk[s] = "zero"

    def _cut(self):
        if self.epochs[-1]:
            self.epochs.append([])
        self.run_start = 0

    def _run_ends(self):
        self.run_start = len(self.epochs[-1])

    def resolve(self, e):
        """Epoch e in table order -> [(frame, state, stamp, pose, refused)]; a stamp never set counts as tick -1."""
        t, out = None, []
        for ent in self.epochs[e]:
            k = -1 if ent["k"] is None else ent["k"]
            refused = t is not None and k <= t
            if refused and self.flags["refused_feeds"]:
                k, refused = t + 0.5, False
            out.append((ent["frame"], ent["state"], k, ent["pose"], refused))
            if not refused:
                t = k
        return out

    def log(self):
        return [self.resolve(e) for e in range(len(self.epochs))]

    def _track_obs(self, t):
        """The observation of a slot's track records t (self.trk[s] as it was at the read), on the log as it is now."""
        if t is None or t == "zero":
            return t if t is None else ("zero",)
        e, ent = t
        k = next(i for i, x in enumerate(self.epochs[e]) if x is ent)
        r = self.resolve(e)[k]
        return ("refused", e, k, r[2]) if r[4] else ("fed", e, k)

    def _whole(self, s, tiled):
        """Does a step with H2D of slot s leave a whole frame in the device slot, whatever the upload form?"""
        return tiled or not self.fam["band"] or self.view[s] == "frame"

    def _dev_frame(self, s, tiled=False):
        d = self.dev[s]
        if d is None:
            raise Illegal(f"slot {s}: the device frame is unspecified")
        if d[0] == "band" and (tiled or self.view[s] != "window" or self.corner[s][1] != d[2]):
            raise Illegal(f"slot {s}: the device frame holds another window's band")
        return d[1]

    def _step(self, kind, slots, frame_of, h2d, group, src):
        for s in slots:
            self.clean[s] = kind == "step"
            self.wiped[s] = frozenset()
            if self.flags["sticky_groups"]:
                self.first_group[s] = self.first_group[s] or group
                if self.first_group[s] != group:
                    continue
            self.last[s] = dict(kind=kind, frame=frame_of(s), state=self.state(s), h2d=h2d, src=src(s), group=group)
            if kind == "step":
                self.stats[s] = (self.last[s]["frame"], self.last[s]["state"])

    def _setter_done(self, slots):
        if self.flags["late_setters"]:
            for s in slots:
                if s in self.inflight and self.last[s] and "post" not in self.last[s]:
                    self.last[s]["state"] = self.state(s)
                    if self.last[s]["kind"] == "step":
                        self.stats[s] = (self.last[s]["frame"], self.last[s]["state"])
                    if isinstance(self.trk[s], tuple):
                        self.trk[s][1].update(state=self.state(s), k=self.stamp[s], pose=self.pose[s])

    def _waited(self, slots):
        for s in slots:
            l = self.last[s]
            if self.flags["late_frames"] and s in self.inflight and l and l["h2d"] and self.pinned[l["src"]] is not None:
                l["frame"] = self.pinned[l["src"]]
                if l["kind"] == "step":
                    self.stats[s] = (l["frame"], l["state"])
                if isinstance(self.trk[s], tuple):
                    self.trk[s][1]["frame"] = l["frame"]
            self.inflight.discard(s)
            self.busy.discard(s)

    # ---- one operation ----------------------------------------------------------------------------------------------------
    def apply(self, op):
        """-> the observation of a reading operation (a dict), else None."""
        k, n, f = op[0], self.n, self.fam
        if k == "write":
            if op[1] in self.busy:
                raise Illegal(f"slot {op[1]} written while an upload may read it")
            self.pinned[op[1]] = op[2]
        elif k in ("set_window", "set_window_center"):
            self.corner[op[1]] = tuple(op[2])
            self.clean[op[1]] = False
            self._setter_done([op[1]])
        elif k == "set_view":
            self.view[op[1]] = op[2]
            self.clean[op[1]] = False
            self._setter_done([op[1]])
        elif k == "set_up":
            self.up[op[1]] = op[2]
            self._setter_done([op[1]])
        elif k == "set_tiles":
            for t, c in enumerate(op[2]):
                self.corner[op[1] + t] = tuple(c)
                self.clean[op[1] + t] = False
            self._setter_done(setter_slots(op, n))
        elif k in ("set_class_policy", "set_enemy_color", "set_pose_prior", "set_refine", "set_metering", "set_bayer_isp", "set_extract_params", "set_tile_merge"):
            key = {"set_class_policy": "policy", "set_enemy_color": "colour", "set_pose_prior": "prior", "set_refine": "refine", "set_metering": "metering",
                   "set_bayer_isp": "isp", "set_extract_params": "extract", "set_tile_merge": "merge"}[k]
            self.glob[key] = op[1]
            if k == "set_tile_merge" and self.flags["late_setters"]:
                for t in self.tiles.values():
                    if any(s in self.inflight for s in t["slots"]):
                        t["merge"] = op[1]
            self._setter_done(range(n))
        elif k in WAIT_SLOT_SETTERS:
            if k == "set_stamp":
                self.stamp[op[1]] = op[2]
            else:
                self.pose[op[1]] = op[2]
            self._setter_done([op[1]])
            if self.glob["tracking"] is not None:            # (before the first set_tracking there is no device table: no wait)
                self._waited([op[1]])
                self._run_ends()
        elif k in WAIT_ALL_SETTERS:
            if k == "reset_tracks" and self.glob["tracking"] is None:
                return None                                  # (no table yet: the call returns at once)
            if k == "set_numbers" and self.glob["numbers"] is None and op[1] == 0:
                return None                                  # (never enabled: nothing to switch off, nothing is made)
            if k != "reset_tracks":
                self.glob[NEW_GLOBAL[k]] = op[1]
            self._setter_done(range(n))
            self._waited(range(n))
            self.busy.clear()
            if k == "reset_tracks" or (k == "set_tracking" and op[1] == 0):
                self._cut()
            if k == "set_tracking" and op[1] == 0:
                self.trk = ["zero"] * n
            if k in ("set_pose_cov", "set_numbers") and op[1] == 0:      # (disabling zeroes the channel of every slot, at once)
                self.wiped = [w | {"covs" if k == "set_pose_cov" else "numbers"} for w in self.wiped]
            self._run_ends()
        elif k in ("detect", "submit"):
            first, count = (op[1], 1) if k == "detect" else (op[1], op[2])
            h2d = True if k == "detect" else op[3]
            slots = list(range(first, first + count))
            if len({self.view[s] for s in slots}) != 1:
                raise Illegal("one step runs one view")
            if h2d and any(self.pinned[s] is None for s in slots):
                raise Illegal("a pinned slot was never written")
            frames = {s: self.pinned[s] if h2d else self._dev_frame(s) for s in slots}
            self._step("step", slots, frames.get, h2d, (first, count), lambda s: s)
            if self.tracking_on():
                self._feed(slots, frames.get, (first, count))
            for s in slots:
                if h2d:
                    self.dev[s] = ("whole", frames[s]) if self._whole(s, False) else None
                if k == "submit":
                    self.inflight.add(s)
                    if h2d:
                        self.busy.add(s)
                else:                      # (detect returns with the slot's results: nothing of the slot is in flight)
                    self.inflight.discard(s)
                    self.busy.discard(s)
        elif k == "submit_tiles":
            src, first, count, h2d = op[1], op[2], op[3], op[4]
            slots = list(range(first, first + count))
            if not f["window"] or any(self.view[s] != "window" for s in slots):
                raise Illegal("tiles run in the window view")
            frame = self.pinned[src] if h2d else self._dev_frame(src, True)
            if frame is None:
                raise Illegal("a pinned slot was never written")
            self._step("tile", slots, lambda s: frame, h2d, ("tiles", src, first, count), lambda s: src)
            self.tiles[first] = dict(parts=[(frame, self.state(s)) for s in slots], merge=self.glob["merge"], src=src, h2d=h2d, slots=slots)
            self._no_feed(slots, lambda s: frame, ("tiles", src, first, count))
            if h2d:
                self.dev[src] = ("whole", frame)
                self.busy.add(src)
            self.inflight.update(slots)
        elif k == "run_post":
            s = op[1]
            l = self.last[s]
            if s in self.inflight or not l or not self.clean[s]:
                raise Illegal(f"run_post on slot {s}: no head of an ordinary step in the slot's present view and window")
            base = l["post"][0] if "post" in l else (l["frame"], l["state"])
            self.last[s] = dict(l, post=(base, self.state(s)))
            self.wiped[s] = frozenset()
            self._no_feed([s], lambda s: base[0], ("post", s))
        elif k == "wait":
            self._waited(range(n))
            self.busy.clear()
            self._run_ends()
        elif k == "wait_slots":
            self._waited(range(op[1], op[1] + op[2]))
            self._run_ends()
        elif k == "wait_upload":
            for s in range(op[1], op[1] + op[2]):
                self.busy.discard(s)
        elif k in ENTRY_KINDS:
            s = op[1]
            if k == "read_head":
                if s in self.inflight or not self.clean[s] or "post" in self.last[s]:
                    raise Illegal(f"read_head on slot {s}: not the head of the slot's last ordinary step")
                return dict(kind=k, slot=s, res=(self.last[s]["frame"], self.last[s]["state"]))
            if k not in f["entries"]:
                raise Illegal(f"{k} is no entry of this family")
            if self.pinned[s] is None:
                raise Illegal("a pinned slot was never written")
            if s in self.busy:
                raise Illegal(f"{k} on slot {s} would load a pinned slot an upload may still read")   # (legal, but then equal to the step's frame: no information)
            self.dev[s] = ("band", self.pinned[s], self.corner[s][1]) if (f["band"] and self.view[s] == "window") else ("whole", self.pinned[s])
            self.clean[s] = False
            return dict(kind=k, slot=s, res=(self.pinned[s], self.state(s)))
        elif k == "refused_views":
            if len({self.view[s] for s in range(op[1], op[1] + op[2])}) == 1:
                raise Illegal("these slots share a view: the submit would be accepted")
            return dict(kind=k, slot=op[1], windows=list(self.corner), views=list(self.view))
        elif k == "refused_window":
            x, y = op[2]
            if 0 <= x <= f["full"][0] - f["win"][0] and 0 <= y <= f["full"][1] - f["win"][1]:
                raise Illegal("this window lies inside the frame")
            return dict(kind=k, slot=op[1], windows=list(self.corner), views=list(self.view))
        elif k == "read":
            s = op[1]
            l = self.last[s]
            if s in self.inflight or l is None:
                raise Illegal(f"read of slot {s}: in flight, or never stepped")
            shift = (0, 0)
            if self.flags["current_corner"] and l["state"][0] == "window":
                shift = (self.corner[s][0] - l["state"][1][0], self.corner[s][1] - l["state"][1][1])
            return dict(kind=k, slot=s, res=(l["frame"], l["state"]), post=l.get("post"), stats=self.stats[s], shift=shift, form=l["kind"],
                        track=self._track_obs(self.trk[s]), _trk=self.trk[s], wiped=self.wiped[s])
        elif k == "read_tiles":
            t = self.tiles.get(op[1])
            if t is None or len(t["slots"]) != op[2] or any(s in self.inflight for s in t["slots"]):
                raise Illegal("read_tiles: no finished tiled step of this range")
            return dict(kind=k, slot=op[1], parts=list(t["parts"]), merge=t["merge"])
        else:
            raise Illegal(f"unknown operation {op!r}")
        return None

    def run(self, program):
        """-> [(index, observation)] of the program's reading operations."""
        out = []
        for i, op in enumerate(program):
            o = self.apply(op)
            if o is not None:
                o["op"] = i
                out.append((i, o))
        for _, o in out:                      # (tracks_by_slot moves entries of an open run: the place in the log as it is at the end)
            if "_trk" in o:
                o["track"] = self._track_obs(o.pop("_trk"))
        return out


def valid(family, program):
    try:
        Model(family).run(program)
        return not check_producer_rule(family, program)
    except Illegal:
        return False


def check_producer_rule(family, program):
    """Written apart from the Model and the generator: the indices of writes into a pinned slot that a submitted upload may still
    read -- a step with H2D (a tiled one: of its frame slot) with no wait_upload / wait_slots / wait on that slot since."""
    reading, bad = {}, []
    tracking_made = numbers_made = False        # (three calls return without a wait on an engine that never enabled the feature)
    for i, op in enumerate(program):
        tracking_made = tracking_made or op[0] == "set_tracking"
        numbers_made = numbers_made or (op[0] == "set_numbers" and op[1] != 0)
        if op[0] == "submit" and op[3]:
            for s in range(op[1], op[1] + op[2]):
                reading[s] = i
        elif op[0] == "submit_tiles" and op[4]:
            reading[op[1]] = i
        elif op[0] in ("wait_upload", "wait_slots"):
            for s in range(op[1], op[1] + op[2]):
                reading.pop(s, None)
        elif op[0] in ("set_stamp", "set_camera_pose"):          # (they wait for their slot, as wait_slots(slot, 1) does, once tracking was set)
            if tracking_made:
                reading.pop(op[1], None)
        elif op[0] == "reset_tracks" and not tracking_made or op[0] == "set_numbers" and not numbers_made:
            pass                                                 # (no table, no records yet: the call returns at once)
        elif op[0] in ("wait", "set_tracking", "reset_tracks", "set_yaw_solve", "set_pose_cov", "set_patches", "set_numbers"):
            reading.clear()
        elif op[0] == "write" and op[1] in reading:
            bad.append(i)
    return bad


# ---- the generator ---------------------------------------------------------------------------------------------------------
def _groupings(n):
    return [(f, c) for c in range(2, n + 1) for f in range(0, n - c + 1)]


class _Gen:
    def __init__(self, family, rng):
        self.family, self.f, self.rng = family, FAMILIES[family], rng
        self.m = Model(family)
        self.ops = []
        self.turns = 0
        self.tracked = "track_phrases" in self.f      # a family with the tracker on: every ordinary step gets its stamp
        self.raw = False                               # (inside a deliberate track phrase: the phrase sets its own stamps)
        self.clock = 0                                 # the program-wide clock: the last tick handed out
        self.stamped = set()                           # slots whose stamp a set_stamp phrase set for their next step

    def emit(self, *op):
        if self.tracked and not self.raw and op[0] in ("detect", "submit"):
            # a fresh tick for every slot of the step, in slot order.  set_stamp waits for its slot, so a slot still in flight
            # gets one only half of the time: the other half it keeps its stale stamp and the step is refused, with no wait
            for t in step_slots(op)[0]:
                if t in self.stamped:
                    self.stamped.discard(t)
                elif t not in self.m.inflight or self.rng.random() < 0.5:
                    self.tick(t)
        self.m.apply(op)            # (raises Illegal on a generator error)
        self.ops.append(op)

    def tick(self, t, k=None):
        """set_stamp on slot t: the next tick of the clock (or tick k, for a stamp that must not rise)."""
        if k is None:
            self.clock += 1
            k = self.clock
        self.m.apply(("set_stamp", t, k))
        self.ops.append(("set_stamp", t, k))
        return k

    def other(self, values, cur):
        return self.rng.choice([v for v in values if v != cur])

    def turn(self, values, cur):
        """A palette value other than the present one, taken in turn (the seeds start at different places): a palette of four
        is walked through by the few setter calls of a handful of programs, which a random choice does not promise."""
        values = list(values)
        self.turns += 1
        v = values[self.turns % len(values)]
        return v if v != cur else values[(self.turns + 1) % len(values)]

    def seed_for(self, s):
        return self.other(SEEDS, self.m.pinned[s])

    def write(self, s):
        if s in self.m.busy:
            self.emit("wait_upload", s, 1)
        self.emit("write", s, self.seed_for(s))

    def setter(self, kind, t, tile_range=None):
        m, r = self.m, self.rng
        if kind in ("set_window", "set_window_center"):
            self.emit(kind, t, self.turn(self.f["corners"], m.corner[t]))
        elif kind == "set_view":
            self.emit(kind, t, "frame" if m.view[t] == "window" else "window")
        elif kind == "set_up":
            self.emit(kind, t, self.other(range(N_UP), m.up[t]))
        elif kind == "set_tiles":
            first, count = tile_range or self.tile_range(t, inside=True)
            cs = list(self.f["corners"])
            r.shuffle(cs)
            self.emit(kind, first, tuple(cs[:count]))
        elif kind == "reset_tracks":
            self.emit(kind)
        elif kind == "set_stamp":
            self.tick(t)
            self.stamped.add(t)
        elif kind == "set_camera_pose":
            self.emit(kind, t, self.other(range(N_POSE), m.pose[t]))
        elif kind == "set_tracking":    # off, then on with the other option set: the tracker stays on for the program's other phrases
            on = 2 if m.glob["tracking"] == 1 else 1
            self.emit(kind, 0)
            self.emit(kind, on)
        elif kind in NEW_GLOBAL:
            key, vals = NEW_GLOBAL[kind], {"set_pose_cov": N_COV, "set_yaw_solve": N_YAW, "set_patches": N_PATCHES, "set_numbers": N_NUMBERS}[kind]
            self.emit(kind, self.turn(range(vals), m.glob[key]))
        else:
            key, vals = {"set_class_policy": ("policy", range(N_POLICY)), "set_enemy_color": ("colour", COLOURS), "set_pose_prior": ("prior", range(N_PRIOR)),
                         "set_refine": ("refine", range(N_REFINE)), "set_metering": ("metering", [0, 1, None]), "set_bayer_isp": ("isp", range(N_ISP)),
                         "set_extract_params": ("extract", range(N_EXTRACT)), "set_tile_merge": ("merge", range(N_MERGE))}[kind]
            self.emit(kind, self.turn(vals, m.glob[key]))

    def tile_range(self, t, inside):
        """(first, count) of a tile range that holds slot t (inside) or leaves it out, so that it can be the frame slot."""
        n = self.m.n
        if inside:
            c = self.rng.randint(2, n - 1) if n > 2 else 1
            first = self.rng.randint(max(0, t - c + 1), min(t, n - c))
            return first, c
        return (t + 1, n - t - 1) if t < n - 1 and (t == 0 or self.rng.random() < 0.5) else (0, t)

    def same_view(self, slots, lead):
        """Bring `slots` into the view of slot `lead`; the submit refused in front of it is part of the alphabet."""
        if len({self.m.view[s] for s in slots}) > 1:
            self.emit("refused_views", slots[0], len(slots))
        for s in slots:
            if self.m.view[s] != self.m.view[lead]:
                self.emit("set_view", s, self.m.view[lead])

    def finish(self, slots):
        """The producer pattern, then the observations: wait_upload, overwrite at once, wait_slots, read."""
        for s in slots:
            if s in self.m.busy:
                self.emit("wait_upload", s, 1)
                self.emit("write", s, self.seed_for(s))
                if self.rng.random() < 0.5:     # an entry while the step still runs: it shows the NEW frame, the step keeps the old
                    self.entry(s)
        for s in slots:
            if s in self.m.inflight:
                self.emit("wait_slots", s, 1)
            self.emit("read", s)

    def entry(self, s):
        kinds = list(self.f["entries"])
        if s not in self.m.busy and kinds:
            self.emit(self.rng.choice(kinds), s)

    def step(self, form, t):
        """One step of `form` that slot t takes part in, the producer pattern behind it, and the observations."""
        m, r, n = self.m, self.rng, self.m.n
        if form == "detect":
            self.write(t)
            self.emit("detect", t)
            self.emit("read", t)
        elif form == "single":
            self.write(t)
            self.emit("submit", t, 1, True, True)
            self.finish([t])
        elif form == "batched":
            first, count = r.choice([g for g in _groupings(n) if g[0] <= t < g[0] + g[1]])
            slots = list(range(first, first + count))
            self.same_view(slots, t)
            for s in slots:
                if m.pinned[s] is None or r.random() < 0.5:
                    self.write(s)
            self.emit("submit", first, count, True, r.random() < 0.6)
            if r.random() < 0.5 and first + count < n and (first + count) not in m.inflight and m.pinned[first + count] is not None:
                self.emit("submit", first + count, 1, True, True)      # a neighbour in flight beside the batch
                slots = slots + [first + count]
            self.finish(slots)
        elif form == "tiled":
            as_frame = m.view[t] == "frame" or r.random() < 0.3
            first, count = self.tile_range(t, inside=not as_frame)
            src = t if as_frame else r.randrange(n)
            slots = list(range(first, first + count))
            for s in slots:
                if m.view[s] != "window":
                    self.emit("set_view", s, "window")
            self.write(src)
            self.emit("submit_tiles", src, first, count, True, r.random() < 0.6)
            if src in m.busy:
                self.emit("wait_upload", src, 1)
                self.emit("write", src, self.seed_for(src))
            self.emit("wait_slots", first, count)
            self.emit("read_tiles", first, count)
            for s in slots:
                self.emit("read", s)

    def phrase(self, i):
        """Setter i mod nS with a step in flight -- of its own slot (even rounds) or of another one only (odd rounds; a global
        setter: of none) --, then a step of form (i / nS) mod nF, then the observations of both."""
        m, r, n, f = self.m, self.rng, self.m.n, self.f
        walk = f.get("walk", f["setters"])
        nS = len(walk)
        kind, form, same = walk[i % nS], f["forms"][(i // nS) % len(f["forms"])], (i // nS) % 2 == 0
        t = r.randrange(n)
        glob = kind not in PER_SLOT
        self.emit("wait")
        a, tr = None, None
        if not (glob and not same):
            a = t if (same or n == 1) else self.other(range(n), t)
            if kind == "set_tiles":      # (a setter of several slots: one of them in flight, or none of them)
                tr = self.tile_range(t, inside=True)
                a = t if same else r.choice([s for s in range(n) if not tr[0] <= s < tr[0] + tr[1]])
            self.write(a)
            self.emit("submit", a, 1, True, True)
        self.setter(kind, t, tr)
        if r.random() < 0.4:
            self.entry(r.randrange(n))
        if a is not None and same:      # the step that was in flight under the setter: it must not have seen it
            self.finish([a])
        self.step(form, t)
        if a is not None and a in m.inflight:
            self.finish([a])
        elif a is not None and m.last[a] is not None and a not in m.inflight:
            self.emit("read", a)

    # ---- the deliberate phrases of rule 7 (a tracked family places each letter of its "track_phrases" once per program) ----------
    def put(self, t, seed):
        if t in self.m.busy:
            self.emit("wait_upload", t, 1)
        self.emit("write", t, seed)

    def track_phrase(self, letter):
        self.raw = True
        try:
            getattr(self, "_phrase_" + letter)()
        finally:
            self.raw = False

    def _alike(self, slots):
        """One frame in every slot of `slots`, and (a window engine) one view and window: the steps see the same armors."""
        m = self.m
        seed = self.seed_for(slots[0])
        for t in slots:
            self.put(t, seed)
            if self.f["window"]:
                if m.view[t] != "window":
                    self.emit("set_view", t, "window")
                if m.corner[t] != self.f["corners"][2]:
                    self.emit("set_window", t, self.f["corners"][2])

    def _phrase_a(self):
        """Single-slot submits on different streams in the slot order 2, 0, 1, no wait between, stamps rising in submit order;
        the same frame under three camera poses, so the later steps re-see the first one's armors a little moved."""
        order = [2, 0, 1]
        self.emit("wait")
        self._alike(order)
        for i, t in enumerate(order):
            if self.m.pose[t] != i:
                self.emit("set_camera_pose", t, i)
        for t in order:
            self.tick(t)
        for t in order:
            self.emit("submit", t, 1, True, True)
        self.finish(order)

    def _phrase_b(self):
        """Regrouping with no wait: (0, 4), then (1, 2), then (3, 1) -- the last unaligned to a stream share.  The stamps cannot
        change in between (set_stamp waits), so the later groups are refused: only if the launches queue in submit order."""
        self.emit("wait")
        self.same_view(list(range(4)), 0)
        for t in range(4):
            self.write(t)
            self.tick(t)
        for first, count in ((0, 4), (1, 2), (3, 1)):
            self.emit("submit", first, count, True, True)
        self.finish(list(range(4)))

    def _phrase_c(self):
        """A tiled step between two fed steps, the first still in flight; then run_post between two fed steps."""
        m = self.m
        self.emit("wait")
        for t in (2, 3):
            if m.view[t] != "window":
                self.emit("set_view", t, "window")
        for t in (0, 1):
            self.write(t)
            self.tick(t)
        self.emit("submit", 0, 1, True, True)
        self.emit("submit_tiles", 1, 2, 2, True, True)
        self.emit("submit", 1, 1, True, True)
        self.emit("wait_slots", 2, 2)
        self.emit("read_tiles", 2, 2)
        self.emit("read", 2)
        self.emit("read", 3)
        self.finish([0, 1])
        self.emit("wait")
        self.write(2)
        self.write(3)
        self.tick(2)
        self.tick(3)
        self.emit("detect", 2)
        self.emit("submit", 3, 1, True, True)
        self.emit("run_post", 2)
        self.emit("read", 2)
        self.tick(2)
        self.emit("detect", 2)
        self.emit("read", 2)
        self.finish([3])

    def _phrase_d(self):
        """A stamp that does not rise in the middle slot of a three-slot submit, once lower and once equal."""
        for first, equal in ((0, False), (1, True)):
            slots = [first, first + 1, first + 2]
            self.emit("wait")
            self.same_view(slots, first)
            for t in slots:
                self.write(t)
            self.clock += 1
            low = self.clock
            k = self.tick(slots[0])
            self.tick(slots[1], k if equal else low)
            self.tick(slots[2])
            self.emit("submit", first, 3, True, True)
            self.finish(slots)

    def _phrase_e(self):
        """set_stamp on slot A while slot B's step is in flight, then a submit of A."""
        a, b = self.rng.sample(range(self.m.n), 2)
        self.emit("wait")
        self.write(a)
        self.write(b)
        self.tick(b)
        self.emit("submit", b, 1, True, True)
        self.tick(a)
        self.emit("submit", a, 1, True, True)
        self.finish([b, a])

    def _phrase_f(self):
        """reset_tracks, set_tracking off, on, and other options while on, each with a step in flight; steps while it is off."""
        m = self.m
        self.emit("wait")
        for t in (0, 1, 2):
            self.write(t)
        self.tick(0)
        self.emit("submit", 0, 1, True, True)
        self.emit("reset_tracks")
        self.tick(1)
        self.emit("submit", 1, 1, True, True)
        on = m.glob["tracking"]
        self.emit("set_tracking", 0)
        self.emit("read", 0)
        self.emit("read", 1)
        self.tick(2)
        self.emit("submit", 2, 1, True, True)
        self.finish([2])
        self.emit("set_tracking", 3 - on)
        self.tick(0)
        self.emit("submit", 0, 1, True, True)
        self.emit("set_tracking", on)           # (on -> on: the table stays, the options change)
        self.emit("read", 0)
        self.tick(1)
        self.emit("submit", 1, 1, True, True)
        self.finish([1])

    def _phrase_g(self):
        """set_pose_cov off, on and with the other sigma_px between fed steps of one frame; each setter waits for the step
        in front of it, so the slot is read with no wait of the program's own."""
        m = self.m
        t = self.rng.randrange(m.n)
        self.emit("wait")
        self.write(t)
        cur = m.glob["cov"]
        for i, v in enumerate([x for x in (0, 1, 2) if x != cur] + [cur]):
            self.emit("set_pose_cov", v)
            if i:
                self.emit("read", t)
            self.tick(t)
            self.emit("submit", t, 1, True, True)
        self.finish([t])

    def _phrase_h(self):
        """A synchronous detect directly behind an asynchronous submit on another stream that nobody waited for."""
        self.emit("wait")
        streams = max(1, self.f["streams"])
        a = self.rng.randrange(self.m.n)
        b = self.rng.choice([t for t in range(self.m.n) if t % streams != a % streams])      # (a single-slot step rides stream slot mod streams)
        self.write(a)
        self.write(b)
        self.tick(a)
        self.tick(b)
        self.emit("submit", a, 1, True, True)
        self.emit("detect", b)
        self.emit("read", b)
        self.finish([a])

    def spice(self):
        """The operations no systematic phrase reaches: regrouping without waits, a step on the device frame behind an entry,
        run_post, read_head, the refused window, a stream share alone."""
        m, r, n, f = self.m, self.rng, self.m.n, self.f
        what = r.choice(["regroup", "device", "run_post", "read_head", "refused_window", "entries"])
        if what == "regroup":
            self.emit("wait")
            self.same_view(list(range(n)), 0)
            for s in range(n):
                self.write(s)
            seq = [(0, n), (1, 1), (0, 2), (1, 2)] + ([(2, 2)] if n >= 4 else [])
            for first, count in seq:
                self.emit("submit", first, count, True, r.random() < 0.5)
                if f["setters"] and r.random() < 0.7:
                    self.setter(r.choice([k for k in f["setters"] if k not in ("set_view", "set_tiles")]), r.randrange(n))
            self.finish(list(range(n)))
        elif what == "device":
            s = r.randrange(n)
            if s in m.inflight:
                self.emit("wait_slots", s, 1)
            self.write(s)
            self.emit(r.choice([k for k in f["entries"]]), s)
            self.emit("write", s, self.seed_for(s))          # the pinned slot moves on; the device frame is the loaded one
            self.emit("submit", s, 1, False, False)
            self.emit("wait_slots", s, 1)
            self.emit("read", s)
        elif what in ("run_post", "read_head"):
            s = r.randrange(n)
            self.write(s)
            self.emit("detect", s)
            if what == "run_post":
                glob = [k for k in f["setters"] if k in ("set_class_policy", "set_enemy_color", "set_pose_prior", "set_refine")]
                self.setter(r.choice(glob), s)
                self.emit("run_post", s)
                self.emit("read", s)
            else:
                self.emit("read_head", s)
        elif what == "refused_window" and f["window"]:
            s = r.randrange(n)
            mx, my = f["full"][0] - f["win"][0], f["full"][1] - f["win"][1]
            self.emit("refused_window", s, r.choice([(-1, 0), (0, -1), (mx + 1, 0), (0, my + 1)]))
        else:
            for s in r.sample(range(n), min(2, n)):
                if m.pinned[s] is None:
                    self.write(s)
                self.entry(s)


def generate(family, seed, length=60):
    """The program of (family, seed): at least `length` operations of whole phrases, closed by a synchronous step and a read of
    every slot.  Phrase i of seed s is systematic phrase (s * PHRASES + i): the seeds of a family walk through every (setter,
    step form) pair in turn."""
    if family == "P":
        return generate_p(seed, length >= 60)
    g = _Gen(family, random.Random(f"{family}/{seed}"))
    g.turns = seed
    for op in FAMILIES[family]["preamble"]:
        g.emit(*op)
    for s in range(g.m.n):
        g.write(s)
    if FAMILIES[family]["window"]:          # build the frame view at start-up, as the header advises
        g.emit("set_view", 0, "frame")
        g.emit("set_view", 0, "window")
    letters = FAMILIES[family].get("track_phrases", "")
    if letters:                             # the seeds start the deliberate phrases at different letters
        letters = letters[seed % len(letters):] + letters[:seed % len(letters)]
    i = 0
    while i < max(PHRASES, len(letters)) or len(g.ops) < length:
        g.phrase(seed * PHRASES + i)
        if i < len(letters):
            g.track_phrase(letters[i])
        if g.rng.random() < 0.6:
            g.spice()
        i += 1
    return _close(g)


def _close(g):
    g.emit("wait")
    for s in range(g.m.n):
        g.emit("detect", s)
        g.emit("read", s)
    return g.ops


def generate_p(seed, with_rotated):
    """Family P: 12 frames round robin over 3 slots -- write, submit async, wait_upload, overwrite, [rotated image of the slot],
    submit the next slot, wait_slots, read."""
    g = _Gen("P", random.Random(f"P/{seed}"))
    n = g.m.n
    for k in range(12):
        s = k % n
        if s in g.m.inflight:
            g.emit("wait_slots", s, 1)
            g.emit("read", s)
        g.emit("write", s, (k + seed) % len(SEEDS))
        g.emit("submit", s, 1, True, True)
        g.emit("wait_upload", s, 1)
        g.emit("write", s, (k + seed + 3) % len(SEEDS))
        if with_rotated:
            g.emit("rotated", s)
    for s in range(n):
        if s in g.m.inflight:
            g.emit("wait_slots", s, 1)
        g.emit("read", s)
    return _close(g)


# ---- the shrinker --------------------------------------------------------------------------------------------------------
def shrink(family, program, fails):
    """Drop operations while the program stays valid and fails(program) stays true -> the shrunk program."""
    program = list(program)
    changed = True
    while changed:
        changed = False
        for i in reversed(range(len(program))):
            cand = program[:i] + program[i + 1:]
            if valid(family, cand) and fails(cand):
                program, changed = cand, True
    return program


# ---- coverage (evaluated by the CPU test on the set the GPU test runs) -------------------------------------------------------
def coverage(family, programs):
    """What a set of programs reaches: kinds, (setter, 'same' | 'other') with a step in flight, (setter, next form) pairs,
    forms followed by an observation, forms with the wait_upload-then-overwrite pattern."""
    cov = dict(kinds=set(), inflight=set(), pairs=set(), observed=set(), overwritten=set())
    n = FAMILIES[family]["slots"]
    for p in programs:
        m = Model(family)
        pending = []                       # setters waiting for the next step
        open_steps = {}                    # slot -> (form, pinned slot) of its last step, until it is read
        uploaded = {}                      # pinned slot -> form whose upload wait_upload has covered
        for op in p:
            k = op[0]
            cov["kinds"].add(k)
            if k in SETTER_KINDS:
                mine = set(setter_slots(op, n))
                if k in PER_SLOT:
                    if mine & m.inflight:
                        cov["inflight"].add((k, "same"))
                    elif m.inflight:
                        cov["inflight"].add((k, "other"))
                else:
                    cov["inflight"].add((k, "same" if m.inflight else "other"))
                pending.append(k)
            form = form_of(op) if k in STEP_KINDS else None
            if form:
                cov["pairs"].update((s, form) for s in pending)
                pending = []
                res, pin = step_slots(op)
                for s in res:
                    open_steps[s] = form
                for s in pin:
                    if op[-1]:             # (asynchronous uploads only)
                        uploaded[s] = ("submitted", form)
                    else:
                        uploaded.pop(s, None)
            if k == "wait_upload":
                for s in range(op[1], op[1] + op[2]):
                    if s in uploaded and uploaded[s][0] == "submitted" and s in m.busy:
                        uploaded[s] = ("waited", uploaded[s][1])
            elif k == "write" and uploaded.get(op[1], ("",))[0] == "waited":
                if any(s in m.inflight for s in range(n)):
                    cov["overwritten"].add(uploaded[op[1]][1])
                uploaded.pop(op[1])
            elif k in ("wait", "wait_slots"):
                for s in (range(n) if k == "wait" else range(op[1], op[1] + op[2])):
                    uploaded.pop(s, None)
            if k == "read" and op[1] in open_steps:
                cov["observed"].add(open_steps.pop(op[1]))
            if k == "read_tiles":
                cov["observed"].add("tiled")
            m.apply(op)
    return cov


# ---- the phrases of rule 7 (found again in a finished program, apart from the generator that placed them) ----------------------
WAITING = WAIT_SLOT_SETTERS + WAIT_ALL_SETTERS + ("wait", "wait_slots")


def track_phrases(family, program):
    """The letters (a) .. (h) of the deliberate phrases a program holds; "d<" and "d=" for the two stale stamps of (d),
    "c" for the tiled step and "c'" for run_post, "f0" reset_tracks, "f1" off, "f2" on again, "f3" other options while on.
    Each in the shape the generator places it:
      c   the step operation in front of the tiled step is an ordinary one that fed, with no wait between and a slot of it
          still in flight; the step operation behind the tiled step is an ordinary one that fed, in the same epoch;
      c'  the same around run_post (whose own slot cannot be in flight: waits may lie between);
      g   three set_pose_cov in a row with the values off, on and the other sigma_px in some order, behind each of them and
          in front of the next a fed step of ONE slot on ONE frame, all in one epoch;
      h   the operation directly in front of a detect is an asynchronous submit, a slot of it in flight on another stream."""
    m = Model(family)
    streams = max(1, FAMILIES[family]["streams"])
    found = set()
    run = []                                    # the step operations since the last operation that waits, with the stamps they saw
    stamp_for = None                            # (slot, slots in flight) of a set_stamp not yet followed by a step
    steps = []                                  # every step operation: dict(op, waited: a wait since the step before, entries, epoch, flying)
    waited = False
    gaps = []                                   # per set_pose_cov: [value, [(slot, entry, epoch) of the ordinary steps behind it]]
    for i, op in enumerate(program):
        k = op[0]
        on = m.tracking_on()
        if k in WAITING and k != "set_stamp":
            run = []
        if k == "set_stamp":
            others = m.inflight - {op[1]}
            stamp_for = (op[1], bool(others) and op[1] not in m.inflight)
            run = [r for r in run if op[1] not in step_slots(r[0])[0]] if op[1] not in m.inflight else []
        if k == "reset_tracks" and m.inflight and on:
            found.add("f0")
        if k == "set_tracking":
            if op[1] == 0 and m.inflight and on:
                found.add("f1")
            if op[1] != 0 and m.glob["tracking"] == 0:
                found.add("f2")
            if op[1] != 0 and on and op[1] != m.glob["tracking"] and m.inflight:
                found.add("f3")
        if k in WAITING:
            waited = True
        if k == "set_pose_cov":
            gaps.append([op[1], []])
        if k in STEP_KINDS:
            flying = bool(steps) and any(t in m.inflight for t in step_slots(steps[-1]["op"])[0])     # (of the step in front)
            steps.append(dict(op=op, waited=waited, entries=[], epoch=len(m.epochs), flying=flying, on=on))
            waited = False
        if k in ("detect", "submit") and on:
            slots = step_slots(op)[0]
            if stamp_for and stamp_for[1] and stamp_for[0] in slots and k == "submit":
                found.add("e")
            prev = program[i - 1] if i else ("",)
            if k == "detect" and prev[0] == "submit" and prev[4] and any(t in m.inflight and t % streams != op[1] % streams for t in step_slots(prev)[0]):
                found.add("h")
            run.append((op, [m.stamp[t] for t in slots]))
            singles = [r for r in run if r[0][0] == "submit" and r[0][2] == 1]
            if len(singles) >= 3 and len(singles) == len(run):
                order = [r[0][1] for r in singles[-3:]]
                ticks = [r[1][0] for r in singles[-3:]]
                if order != sorted(order) and len({t % streams for t in order}) > 1 and None not in ticks and ticks == sorted(set(ticks)):
                    found.add("a")
            if [r[0][1:3] for r in run[-3:]] == [(0, 4), (1, 2), (3, 1)]:
                found.add("b")
        if k in STEP_KINDS:
            stamp_for = None
        m.apply(op)
        if k in ("detect", "submit") and on:
            steps[-1]["entries"] = [m.trk[t][1] for t in step_slots(op)[0]]
            steps[-1]["epoch"] = len(m.epochs)
            if gaps:
                gaps[-1][1].extend((t, m.trk[t][1], len(m.epochs)) for t in step_slots(op)[0])
    fed = {id(ent) for e, epoch in enumerate(m.epochs) for ent, r in zip(epoch, m.resolve(e)) if not r[4]}
    feeds = lambda st: st["op"][0] in ("detect", "submit") and any(id(x) in fed for x in st["entries"])      # noqa: E731
    for j in range(1, len(steps) - 1):
        before, skip, after = steps[j - 1], steps[j], steps[j + 1]
        if skip["on"] and skip["op"][0] in ("submit_tiles", "run_post") and feeds(before) and feeds(after) and before["epoch"] == after["epoch"]:
            if skip["op"][0] == "run_post":
                found.add("c'")
            elif skip["flying"] and not skip["waited"]:
                found.add("c")
    for j in range(len(gaps) - 2):
        three = gaps[j:j + 3]
        if sorted(g[0] for g in three) == [0, 1, 2]:
            same = [{(t, ent["frame"], e) for t, ent, e in g[1] if id(ent) in fed} for g in three]
            if same[0] & same[1] & same[2]:
                found.add("g")
    for e, epoch in enumerate(m.epochs):
        res = m.resolve(e)
        t = None
        for i, (ent, r) in enumerate(zip(epoch, res)):
            g = ent["group"]
            if r[4] and len(g) == 2 and g[1] >= 3 and g[0] < ent["slot"] < g[0] + g[1] - 1:
                sides = [x for x, y in zip(epoch, res) if x["group"] == g and not y[4] and abs(x["slot"] - ent["slot"]) == 1]
                if i and i + 1 < len(epoch) and len(sides) >= 2 and epoch[i - 1] in sides and epoch[i + 1] in sides:
                    found.add("d=" if r[2] == t else "d<")
            if not r[4]:
                t = r[2]
    return found


PHRASE_PARTS = {"a": {"a"}, "b": {"b"}, "c": {"c", "c'"}, "d": {"d<", "d="}, "e": {"e"}, "f": {"f0", "f1", "f2", "f3"}, "g": {"g"}, "h": {"h"}}


# ---- the host reference of rule 7: irmv_detection_amd/tracks.py stepped through a model's log ------------------------------------
ZERO_TRACKS = (bytes(40), bytes(32 * 384))          # a slot's frame header and snapshot where no step fed: all zero


class Replay:
    """result(epoch, k) -> (det_tracks, frame, snapshot) as tracks.Tracker returns them for entry k of the epoch, every entry
    before it fed in the log's order, each under the options its state names; a refused entry is fed like the others and the
    reference refuses it itself (asserted).  The id counter carries over from epoch to epoch.  Memoised per (epoch, k); the
    reference is fed incrementally.
      log      Model.log();  obs_of(frame, state) -> [tracks.Obs];  options[i] -> tracks.Options of palette entry i;
      stamp_of(k) -> seconds;  poses[i] -> (R_wc[9], t_wc[3])"""

    def __init__(self, log, obs_of, options, stamp_of, poses):
        self.log, self.obs_of, self.options, self.stamp_of, self.poses = log, obs_of, options, stamp_of, poses
        self.out = [[] for _ in log]
        self.trackers = {}

    def first_id(self, e):
        """The id counter at the start of epoch e: what the epochs before it issued, plus one."""
        if e == 0:
            return 1
        self.result(e - 1, len(self.log[e - 1]) - 1)
        return self.trackers[e - 1].next_id if self.log[e - 1] else self.first_id(e - 1)

    def result(self, e, k):
        from irmv_detection_amd import tracks as T
        if k < 0:
            return None
        if e not in self.trackers:
            self.trackers[e] = T.Tracker(self.options[1])
            self.trackers[e].next_id = self.first_id(e)
        tr = self.trackers[e]
        while len(self.out[e]) <= k:
            frame, state, stamp, pose, refused = self.log[e][len(self.out[e])]
            tr.opt = self.options[state[14]] or self.options[1]      # (an entry fed with tracking off: a wrong model's only)
            res = tr.update(self.stamp_of(stamp), self.obs_of(frame, state), *self.poses[pose])
            if (res[1].state == T.FRAME_STALE) != refused:       # (the model and the reference disagree on a stamp: no engine's error)
                raise RuntimeError(f"epoch {e}, entry {len(self.out[e])}, stamp {stamp}: the reference's refusal is not the model's")
            self.out[e].append(res)
        return self.out[e][k]


def pack_tracks(res):
    from irmv_detection_amd import tracks as T
    dets, frame, snap = res
    return b"".join(T.pack_det_track(d) for d in dets), T.pack_frame(frame), b"".join(T.pack_track(t) for t in snap)


def expected_tracks(replay, track, n_dets):
    """The three byte strings a read with observation `track` must deliver (n_dets: the slot's number of result records)."""
    if track[0] == "zero":
        return (bytes(72 * n_dets),) + ZERO_TRACKS
    return pack_tracks(replay.result(track[1], track[2]))


# ---- a host simulation of the whole comparison: the "engine" is a Model, its detections a fixed synthetic set ------------------
SIM_POINTS = [(-0.6 + 0.3 * (i % 5), -0.2 + 0.2 * (i // 5), 3.0 + 0.25 * (i % 3)) for i in range(10)]
SIM_STAMP = lambda k: 0.0 if k < 0 else 1.0 + 0.01 * k      # noqa: E731
SIM_POSES = [((1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0), t) for t in ((0.0, 0.0, 0.0), (0.002, 0.0, 0.0), (0.0, -0.001, 0.003))]


def sim_options():
    from irmv_detection_amd import tracks as T
    return [None, T.Options(max_misses=1, match_class=1), T.Options(max_misses=2, match_class=0, confirm_hits=2)]


def sim_obs(frame, state):
    """A few armors per palette frame, fixed per (frame, view, corner): five of the ten points, classes by point; with the
    covariance on, a diagonal one that grows with sigma's palette index."""
    from irmv_detection_amd import tracks as T
    r = random.Random(f"sim/{frame}/{state[0]}/{state[1]}")
    cov = None if not state[11] else tuple((1e-5 * state[11] if i == j else 0.0) for i in range(3) for j in range(3))
    return [T.Obs(i % 3, SIM_POINTS[i], 1, cov) for i in sorted(r.sample(range(10), 5))]


def simulate(family, program, **flags):
    """What an engine that followed Model(family, **flags) would deliver at every read of the program: the attribution of the
    per-frame records, and the bytes of the three track records."""
    m = Model(family, **flags)
    obs = m.run(program)
    replay = Replay(m.log(), sim_obs, sim_options(), SIM_STAMP, SIM_POSES)
    out = []
    for _, o in obs:
        if o["kind"] == "read":
            n = len(sim_obs(*o["res"]))
            out.append((o["res"], o["post"], o["stats"], (o["shift"], o["wiped"]), None if o["track"] is None else expected_tracks(replay, o["track"], n)))
    return out
