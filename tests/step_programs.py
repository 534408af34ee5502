"""Seeded step programs and the host model of the engine's ordering contract (numpy only; DESIGN.md, "ordering contract").

A PROGRAM is a list of operations on one engine, each a tuple (kind, args...).  generate(family, seed, length) is
deterministic.  A Model replays a program on the host and says, for every OBSERVATION (an operation that reads something
back), which inputs the observed step saw: it computes no detection, only the attribution

    (frame seed, (view, corner, policy, colour, prior, up, refine, metering, isp, extract))

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
     window as they are at the call, after the slot's step in flight has finished, and leaves the slot's results alone.

Operations:
  ("write", slot, seed)                                   a palette frame into the pinned slot
  ("set_window" | "set_window_center", slot, (x, y))      ("set_view", slot, "frame" | "window")
  ("set_class_policy", i)  ("set_enemy_color", c)         ("set_pose_prior", i)  ("set_up", slot, i)
  ("set_refine", i)  ("set_metering", i)  ("set_bayer_isp", i)  ("set_extract_params", i)
  ("set_tiles", first, (corner, ...))  ("set_tile_merge", i)
  ("detect", slot)  ("submit", first, count, h2d, async)  ("submit_tiles", frame_slot, first, count, h2d, async)
  ("run_post", slot)
  ("wait",)  ("wait_slots", first, count)  ("wait_upload", first, count)
  ("render" | "meter" | "rotated" | "extract" | "refine_points" | "read_head", slot)
  ("refused_views", first, count)  ("refused_window", slot, (x, y))
  ("read", slot)  ("read_tiles", first, count)
"""
import random

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
}
SEEDS = tuple(range(6))                 # frame palette: indices into the GPU module's list of synthetic frames
N_POLICY, N_PRIOR, N_UP, N_REFINE, N_METERING, N_ISP, N_EXTRACT, N_MERGE = 4, 3, 3, 2, 3, 2, 2, 2
COLOURS = (-1, 0)
LENGTH = 60                             # operations per program of the GPU test, at least
LAUNCH_FORMS = ("default", "eager", "graph", "no_graph_upload", "no_window_upload", "inline_copies", "no_zero_copy")
# the GPU test's cases: six seeds per family under the default launch form, two more of W and B under each other one
GPU_CASES = [(f, "default", s) for f in "WBC" for s in range(6)] + [(f, form, s) for f in "WB" for form in LAUNCH_FORMS[1:] for s in (6, 7)]
PHRASES = 6                             # systematic phrases per program, at least
CONTROL_SEED, CONTROL_LENGTH = 0, 60    # the W program the GPU test's controls run on
PER_SLOT = ("set_window", "set_window_center", "set_view", "set_up", "set_tiles")
STEP_KINDS = ("detect", "submit", "submit_tiles", "run_post")
WAIT_KINDS = ("wait", "wait_slots", "wait_upload")
ENTRY_KINDS = ("render", "meter", "rotated", "extract", "refine_points", "read_head")
READ_KINDS = ("read", "read_tiles")
SETTER_KINDS = ("set_window", "set_window_center", "set_view", "set_class_policy", "set_enemy_color", "set_pose_prior", "set_up", "set_refine",
                "set_metering", "set_bayer_isp", "set_extract_params", "set_tiles", "set_tile_merge")


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
    """The contract.  The four keyword flags each break one rule (the GPU test's controls); all False: the contract."""

    def __init__(self, family, late_setters=False, late_frames=False, sticky_groups=False, current_corner=False):
        f = self.fam = FAMILIES[family]
        n = self.n = f["slots"]
        self.flags = dict(late_setters=late_setters, late_frames=late_frames, sticky_groups=sticky_groups, current_corner=current_corner)
        self.pinned = [None] * n
        centre = ((f["full"][0] - f["win"][0]) // 2, (f["full"][1] - f["win"][1]) // 2) if f["window"] else (0, 0)
        self.corner = [centre] * n
        self.view = ["window" if f["window"] else "frame"] * n
        self.up = [0] * n
        self.glob = dict(policy=0, colour=-1, prior=None, refine=0, metering=None, isp=0, extract=0, merge=0)
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
        return (self.view[s], self.corner[s], g["policy"], g["colour"], g["prior"], self.up[s], g["refine"], g["metering"], g["isp"], g["extract"])

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

    def _waited(self, slots):
        for s in slots:
            l = self.last[s]
            if self.flags["late_frames"] and s in self.inflight and l and l["h2d"] and self.pinned[l["src"]] is not None:
                l["frame"] = self.pinned[l["src"]]
                if l["kind"] == "step":
                    self.stats[s] = (l["frame"], l["state"])
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
        elif k == "wait":
            self._waited(range(n))
            self.busy.clear()
        elif k == "wait_slots":
            self._waited(range(op[1], op[1] + op[2]))
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
            return dict(kind=k, slot=s, res=(l["frame"], l["state"]), post=l.get("post"), stats=self.stats[s], shift=shift, form=l["kind"])
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
    for i, op in enumerate(program):
        if op[0] == "submit" and op[3]:
            for s in range(op[1], op[1] + op[2]):
                reading[s] = i
        elif op[0] == "submit_tiles" and op[4]:
            reading[op[1]] = i
        elif op[0] in ("wait_upload", "wait_slots"):
            for s in range(op[1], op[1] + op[2]):
                reading.pop(s, None)
        elif op[0] == "wait":
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

    def emit(self, *op):
        self.m.apply(op)            # (raises Illegal on a generator error)
        self.ops.append(op)

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
        nS = len(f["setters"])
        kind, form, same = f["setters"][i % nS], f["forms"][(i // nS) % len(f["forms"])], (i // nS) % 2 == 0
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
    i = 0
    while i < PHRASES or len(g.ops) < length:
        g.phrase(seed * PHRASES + i)
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
