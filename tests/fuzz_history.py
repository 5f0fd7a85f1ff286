"""Scripts of calls for the call-history tests (tests/test_history_cpu.py, tests/test_gpu_history.py): what ONE long-lived context is asked to
do -- settings, batch calls, sweeps of the callback path, read-outs -- in a random but reproducible order, the clouds and the parameter sets
the steps draw from, and a shadow of urf_policy::plan's history-free part (urban_road_filter_amd/csrc/urf_policy.hpp; tests/test_policy_table.py holds it to the real function) that says where the path
of a call is certain.  Pure numpy; no GPU.

A step is a dict of plain values (names of pool entries, tags of parameter sets), so that the steps so far print readably in an assertion
message and script(seed, family)[:k + 1] replays a failure."""
import numpy as np

import urban_road_filter_amd as u
from fuzz import case as fuzz_case

TILE = 2048
# The smallest shapes at which the paths still differ: three tiles each (16 x 304 and 32 x 136 end in a partial one, 64 x 96 and 128 x 48 are
# three whole tiles).  synth_cloud puts firing c at (c + 0.5) * 360 / cols degrees: with a column count that is a multiple of 8 no firing
# lies on a whole degree, the border of two star sectors.
COLS = {16: 304, 32: 136, 64: 96, 128: 48}
# ... and the shapes where some do (16 x 300: firing 7 at 9 degrees; 32 x 130: firing 6 at 18 degrees).  Rounded to float the points of such a
# firing fall into both sectors, k_front's march needs ONE sector per firing (urf_front.hpp, "the firing's participants share one sector")
# and hands the scan back to the general kernels: kind "astride" (row-major: "astride_rows").  Legal input like any other cloud; with the
# star-shaped search on, never a fused scan.
ASTRIDE_COLS = {16: 300, 32: 130}
LONG_COLS = 4128                                    # 64 x 4128: 129 tiles
FAMILIES = {"small": (128 * 300, 4), "long": (64 * LONG_COLS, 2)}   # u.Context(max_points, max_batch)
SEEDS = {"small": tuple(range(12)), "long": (111, 117, 137)}   # (tests/test_history_cpu.py says what the scripts of these seeds must hold)
STEPS = {"small": 48, "long": 24}
LASERS = {"small": (16, 32, 64, 128), "long": (64, 16)}
MODES = (0, 1, 2, 3)
PRESET_BITS = (2, 4, 16)
ENTRY_POINTS = ("soa", "ragged", "pc2_16", "pc2_23")
PC2_LAYOUT = {"pc2_16": (16, 0, 4, 8), "pc2_23": (23, 3, 11, 17)}   # (the layouts of tests/test_gpu_abi_surface.py)
READOUTS = ("ordered", "marker", "batch", "detect")
CLASSES = ("firing", "rows", "mixed", "callback", "readout", "params", "switch")
VARIANTS = ((1, 1, 0), (1, 0, 1), (1, 1, 2), (0, 1, 0))   # star_shaped_method, blind_spots, xDirection


# ---- the parameter pool ----
def make_params(L, wide, cp, variant):
    p = u.default_params()
    if wide:
        p = p.wide_roi()
    p.channels = L
    if L == 128:
        p.interval = 0.05   # (with the default interval a 128-laser sweep has only 64 rings in oracle B)
    p.curbPoints = cp
    p.star_shaped_method, p.blind_spots, p.xDirection = variant
    return p


def param_tag(L, wide, cp, variant):
    return "L%d/%s/cp%d/star%d/blind%d/xdir%d" % ((L, "wide" if wide else "default", cp) + tuple(variant))


_PARAMS = {}


def param_pool(family):
    """tag -> Params: per laser count the wide and the default region of interest x curbPoints {5, 5, 3, 9}, the three switches varied
    along (family "long": five sets, its oracle runs cost half a second each)."""
    if family not in _PARAMS:
        pool = {}
        for L in LASERS[family]:
            combos = [(w, cp) for w in (True, False) for cp in (5, 5, 3, 9)]
            if family == "long":
                combos = [(True, 5), (False, 5), (True, 3), (True, 9)] if L == 64 else [(True, 5)]
            for k, (wide, cp) in enumerate(combos):
                v = VARIANTS[(k + k // 4) % 4]
                pool[param_tag(L, wide, cp, v)] = make_params(L, wide, cp, v)
        _PARAMS[family] = pool
    return _PARAMS[family]


DEFAULT_TAG = "default"   # a new context's parameters


def params_of(family, tag):
    return u.default_params() if tag == DEFAULT_TAG else param_pool(family)[tag]


def tag_lasers(tag):
    return 64 if tag == DEFAULT_TAG else int(tag.split("/")[0][1:])


def tag_curb_points(tag):
    return 5 if tag == DEFAULT_TAG else int(tag.split("/")[2][2:])


# ---- the cloud pool ----
class Entry:
    def __init__(self, name, kind, lasers, cloud):
        self.name, self.kind, self.lasers = name, kind, lasers   # kind: firing | astride | cut | rows | astride_rows | unorganised
        self.cloud = tuple(np.ascontiguousarray(a, np.float32) for a in cloud)
        for a in self.cloud:
            a.setflags(write=False)

    def __len__(self):
        return len(self.cloud[0])


def ring_major(cloud, L):
    """The same sweep stored row by row (row-major L x W: an organised cloud)."""
    return tuple(np.ascontiguousarray(a.reshape(-1, L).T.reshape(-1)) for a in cloud)


def rolled(cloud, L, cols):
    return tuple(np.ascontiguousarray(np.roll(a.reshape(-1, L), cols, axis=0).reshape(-1)) for a in cloud)


def _fuzz_clouds(count, max_points):
    """tests/fuzz.py cases of at least 3000 points without a point on the sensor's axis (the pool has its own NaN-azimuth entry)"""
    out, seed = [], 2000
    while len(out) < count:
        (x, y, z), _ = fuzz_case(seed)
        if 3000 <= len(x) <= max_points and not ((x == 0) & (y == 0)).any():
            out.append((x, y, z))
        seed += 1
    return out


_POOL = {}


def pool(family):
    """name -> Entry, built once per family."""
    if family in _POOL:
        return _POOL[family]
    max_points = FAMILIES[family][0]
    E = {}

    def add(name, kind, lasers, cloud):
        assert name not in E and len(cloud[0]) <= max_points
        E[name] = Entry(name, kind, lasers, cloud)

    for L in ((16, 32, 64, 128) if family == "small" else (64,)):
        for s in (1, 2, 3, 4):   # (scenes 3 and 4: planar-range ties in every sector)
            c = u.synth_cloud(L, COLS[L], s, 7)
            add("f%ds%d" % (L, s), "firing", L, c)
            add("r%ds%d" % (L, s), "rows", L, ring_major(c, L))
    if family == "small":
        for L, cols in ASTRIDE_COLS.items():
            for s in (1, 2, 3, 4):
                c = u.synth_cloud(L, cols, s, 7)
                add("a%ds%d" % (L, s), "astride", L, c)
                add("ar%ds%d" % (L, s), "astride_rows", L, ring_major(c, L))
    if family == "long":
        for s, seed in ((1, 71), (3, 72)):
            c = u.synth_cloud(64, LONG_COLS, s, seed)
            add("F64s%d" % s, "firing", 64, c)
            add("R64s%d" % s, "rows", 64, ring_major(c, 64))
    base = u.synth_cloud(64, 96, 1, 8)
    add("cut64", "cut", 64, tuple(a[:64 * 60 + 17].copy() for a in base))   # (ends inside a firing)
    for k, c in enumerate(_fuzz_clouds(2, max_points)):
        add("fuzz%d" % k, "unorganised", 0, c)
    pm = np.random.default_rng(1).permutation(64 * 96)
    add("shuffled", "unorganised", 0, tuple(a[pm] for a in base))
    add("rolled", "unorganised", 0, rolled(u.synth_cloud(64, 96, 2, 9), 64, 700 % 96))
    nan = tuple(a.copy() for a in u.synth_cloud(64, 96, 3, 10))
    for a, v in zip(nan, (0.0, 0.0, -1.8)):
        a[2000] = v                                   # x == y == 0 on a ring: a NaN azimuth
    add("nan", "unorganised", 0, nan)
    few = tuple(a.copy() for a in base)
    few[0][29:] = 1.0e6                               # all but 29 points far outside the region of interest: below the 30-point threshold
    add("few", "unorganised", 0, few)
    _POOL[family] = E
    return E


def organised(family):
    return [e for e in pool(family).values() if e.kind != "unorganised"]


# ---- the shadow of the settings ----
def front_curb_points_ok(mode, L, cp):
    return cp == 5 or (mode == 3 and L == 64 and 1 <= cp <= 8)


class Shadow:
    """What the test knows of the context's settings, and from them where urf_policy::plan's decision does not depend on the history.
    `wrs` shadows want_ring_sorted and `last_front` the last call's a.front: True / False where the settings alone decide them, None where
    the history has a say (mode 1's thresholds, the callback path, a refusal that may or may not have come first)."""

    def __init__(self, family):
        self.family = family
        self.rows = min(FAMILIES[family][1], 4)
        self.mode, self.l128, self.long, self.outputs, self.capture = 1, 0, 0, 0, 0
        self.tag = DEFAULT_TAG
        self.wrs = False
        self.last = None            # the last classify step
        self.last_front = False

    @property
    def lasers(self):
        return tag_lasers(self.tag)

    def setting(self, step):
        op, v = step["op"], step.get("value")
        if op == "set_params":
            self.tag = step["params"]
        elif op == "set_front_mode":
            self.mode = v
            if v != 0:
                self.wrs = False
        elif op == "set_front_lasers128":
            self.l128 = v
            if v:
                self.wrs = False
        elif op == "set_front_long_sweeps":
            self.long = v
            if v:
                self.wrs = False
        elif op == "set_front_outputs":
            self.outputs = v
        elif op == "enable_stage_capture":
            self.capture = v
        else:
            assert op == "callback_path_preset", op

    def max_tiles(self):
        return 256 if self.long and self.mode >= 2 else 128

    def excluded(self, tiles):
        """plan() keeps the fused kernels out whatever the history"""
        L = self.lasers
        lasers_ok = L in (16, 32, 64) or (L == 128 and self.l128 and self.mode >= 2)
        return (self.mode == 0 or self.capture != 0 or not lasers_ok or not front_curb_points_ok(self.mode, L, tag_curb_points(self.tag)) or
                tiles > self.max_tiles() or self.wrs is True)

    def tiles(self, step):
        E = pool(self.family)
        return max(1, -(-max(len(E[n]) for n in step["scans"]) // TILE))

    def all_of(self, step, kind):
        E = pool(self.family)
        return all(E[n].kind == kind and E[n].lasers == self.lasers for n in step["scans"])

    def expect(self, step):
        """front_scans() after this classify step: a number where it is certain, None where the history may decide.  Call before call()."""
        n = len(step["scans"]) if step["op"] == "batch" else 1
        if self.excluded(self.tiles(step)):
            return 0
        if step["op"] == "batch" and self.mode >= 2 and self.wrs is False:
            if self.all_of(step, "firing"):
                return n                                            # an anchor step
            if self.all_of(step, "rows") and step.get("repeat"):
                return n                                            # (the call before it has sighted the layout, at the latest)
            E = pool(self.family)
            kinds = [E[m].kind for m in step["scans"]]
            if (set(kinds) <= {"firing", "astride"} and all(E[m].lasers == self.lasers for m in step["scans"]) and
                    params_of(self.family, self.tag).star_shaped_method):
                return kinds.count("firing")                        # (a firing astride a sector border: that scan is handed back, ASTRIDE_COLS)
        return None

    def is_anchor(self, step):
        return step["op"] == "batch" and self.mode >= 2 and self.wrs is False and not self.excluded(self.tiles(step)) and self.all_of(step, "firing")

    def call(self, step, fused_seen=None):
        """fused_seen: front_scans() > 0 where a device has said so"""
        if self.excluded(self.tiles(step)):
            self.last_front = False
        elif step["op"] == "batch" and self.mode >= 2 and self.wrs is False:
            self.last_front = True
        else:
            self.last_front = True if fused_seen else None
        self.last = step

    def busy_possible(self):
        """a read-out may be refused (URF_ERR_BUSY): the last sweep of a group larger than the scratch rows shares its row with an earlier
        one, whose rerun -- if the short sequence voided it -- was the row's later submission"""
        return self.last is not None and self.last["op"] == "callback" and len(self.last["scans"]) > self.rows

    def readout(self, step, busy=None):
        """busy: per read-out of the step whether it was refused (a device has said so); None: busy_possible() decides"""
        for k, (what, _) in enumerate(step["what"]):
            reruns = what == "detect" or not self.outputs
            refused = busy[k] if busy is not None else (None if self.busy_possible() else False)
            if not reruns or refused is True or self.last_front is False:
                continue
            if refused is None or self.last_front is None:
                self.wrs = True if self.wrs is True else None
                self.last_front = None
            else:
                self.wrs, self.last_front = True, False


def step_class(family, step):
    op = step["op"]
    if op == "batch":
        kinds = {pool(family)[n].kind for n in step["scans"]}
        return "firing" if kinds <= {"firing", "cut", "astride"} else ("rows" if kinds <= {"rows", "astride_rows"} else "mixed")
    return {"callback": "callback", "readout": "readout", "set_params": "params"}.get(op, "switch")


# ---- the generator ----
CLASS_WEIGHTS = {"firing": 0.19, "rows": 0.11, "mixed": 0.09, "callback": 0.11, "readout": 0.13, "params": 0.12, "switch": 0.25}
# every setter with every value: a script deals them in turn from one shuffled deck, from a place of its own (with a handful of switch steps
# per script, drawing them at random would leave some value out of all scripts)
SWITCHES = ([("set_front_mode", m) for m in MODES] + [(op, v) for op in ("set_front_lasers128", "set_front_long_sweeps", "set_front_outputs")
                                                       for v in (0, 1)] + [("enable_stage_capture", 0), ("enable_stage_capture", 2)] +
            [("callback_path_preset", b) for b in (2, 4, 16, 22)])


def script(seed, family):
    """The steps of one history: deterministic in (seed, family)."""
    rng = np.random.default_rng([seed, sorted(FAMILIES).index(family)])
    E, P = pool(family), param_pool(family)
    names = {k: [e.name for e in E.values() if e.kind == k] for k in ("firing", "astride", "cut", "rows", "astride_rows", "unorganised")}
    max_batch = FAMILIES[family][1]
    lasers = LASERS[family]
    sh = Shadow(family)
    steps, left = [], [0] * len(lasers)
    deck, dealt = [SWITCHES[i] for i in np.random.default_rng(0).permutation(len(SWITCHES))], seed * 5
    cur = seed % len(lasers)
    classes = list(CLASSES)
    w = np.array([CLASS_WEIGHTS[c] for c in classes])

    def pick(seq):
        return seq[int(rng.integers(len(seq)))]

    def of_lasers(kind, L):
        return [n for n in names[kind] if E[n].lasers == L]

    def scans_of(cls, n):
        L = sh.lasers
        if cls in ("firing", "rows"):
            own = of_lasers(cls, L)
            if own and rng.random() < (0.65 if L in ASTRIDE_COLS and family == "small" else 0.8):
                first = pick(own)
                if family == "long":
                    big = bool(rng.random() < 0.5)   # 129 tiles or 3, as often
                    first = pick([m for m in own if (len(E[m]) > 64 * 96) == big])
                    if rng.random() < 0.6:   # one length: every entry point is open
                        own = [m for m in own if len(E[m]) == len(E[first])]
                return [first] + [pick(own) for _ in range(n - 1)]
            # otherwise any sweep of the layout: another laser count's, the cut one, and -- as often as not, where the laser count has
            # them -- the ones with a firing astride a sector border, alone or next to the others
            astride = of_lasers("astride" if cls == "firing" else "astride_rows", L)
            if astride and rng.random() < 0.75:
                out = [pick(astride)] + ([pick(own)] if n > 1 and own else []) + [pick(astride + own) for _ in range(n - 2)]
                return [out[i] for i in rng.permutation(len(out))]
            return [pick(names[cls] + (names["cut"] + names["astride"] if cls == "firing" else names["astride_rows"])) for _ in range(n)]
        out = [pick(names["unorganised"])] + [pick(list(E)) for _ in range(n - 1)]
        return [out[i] for i in rng.permutation(n)]

    def batch(cls):
        n = int(rng.integers(1, max_batch + 1))
        scans = scans_of(cls, n)
        uniform = len({len(E[m]) for m in scans}) == 1
        entry = pick(ENTRY_POINTS) if uniform else "ragged"
        return {"op": "batch", "entry": entry, "scans": scans, "pad": int(rng.integers(1, 5000)) if entry == "ragged" else 0,
                "info": bool(rng.random() < 0.75)}

    while len(steps) < STEPS[family]:
        p = w.copy()
        if sh.last is None:
            p[classes.index("readout")] = 0.0
        # where the settings alone send a sweep in firing order through the fused kernels, such batches come often (the anchor steps);
        # elsewhere the settings change sooner
        capable = sh.mode >= 2 and sh.wrs is False and not sh.excluded(3)
        if family == "long":   # (24 steps: its scripts have to get to the 129-tile fused path quickly, and stay a while)
            capable = capable and sh.long == 1 and sh.lasers == 64
            p[classes.index("firing")] *= 3.0 if capable else 0.4
            p[classes.index("rows")] *= 2.0 if capable else 0.5
            p[classes.index("switch")] *= 0.8 if capable else 2.5
            p[classes.index("params")] *= 0.7 if capable else (2.0 if sh.lasers != 64 else 1.0)
        else:
            p[classes.index("firing")] *= 3.0 if capable else 0.6
            p[classes.index("switch")] *= 1.0 if capable else 1.8
            p[classes.index("params")] *= 1.0 if capable else 1.3
        cls = classes[int(rng.choice(len(classes), p=p / p.sum()))]
        if cls in ("firing", "rows", "mixed"):
            step = batch(cls)
            steps.append(step)
            sh.call(step)
            if cls == "rows" and len(steps) < STEPS[family] and rng.random() < 0.6:
                step = dict(step, repeat=True)   # the same call once more, no setting in between
                steps.append(step)
                sh.call(step)
        elif cls == "callback":
            n = int(rng.integers(1, 5))
            how = "xyz" if rng.random() < 0.25 else pick(("async16", "async32"))
            kind = "rows" if rng.random() < 0.5 else "mixed"
            step = {"op": "callback", "how": how, "scans": scans_of(kind, 1 if how == "xyz" else n)}
            steps.append(step)
            sh.call(step)
        elif cls == "readout":
            n = len(sh.last["scans"]) if sh.last["op"] == "batch" else 1
            what = [k for k in READOUTS if rng.random() < 0.4] or [pick(READOUTS)]
            step = {"op": "readout", "what": [(k, int(rng.integers(n))) for k in what]}
            steps.append(step)
            sh.readout(step)
        elif cls == "params":
            if family == "long":
                # 64 lasers three times out of four: only they take the 129-tile fused path
                nxt = 0 if rng.random() < 0.75 else 1
            else:
                # the next laser count: from every count to every count in turn
                nxt = (cur + seed // len(lasers) + left[cur]) % len(lasers)   # (seeds 0..3: first to the count they begin with once more)
                left[cur] += 1
            cur = nxt
            tags = [t for t in P if tag_lasers(t) == lasers[cur]]
            # (curbPoints 5 more often than 3 or 9, which only 64 lasers in mode 3 take to the fused kernels)
            tw = np.array([(2.0 if lasers[cur] == 64 else 3.0) if tag_curb_points(t) == 5 else 1.0 for t in tags])
            step = {"op": "set_params", "params": tags[int(rng.choice(len(tags), p=tw / tw.sum()))]}
            steps.append(step)
            sh.setting(step)
        else:
            # a context that has left the fused kernels for good comes back soon: the anchor steps need it there
            back = []
            if sh.mode < 2 or sh.wrs is not False:
                back.append(("set_front_mode", 2 if rng.random() < 0.6 else 3))
            if sh.capture:
                back.append(("enable_stage_capture", 0))
            if sh.lasers == 128 and not sh.l128:
                back.append(("set_front_lasers128", 1))
            if family == "long" and not sh.long:
                back.append(("set_front_long_sweeps", 1))   # (the 129-tile sweeps need it, and mode 2 or 3)
            if sh.mode == 2 and sh.lasers == 64 and 1 <= tag_curb_points(sh.tag) <= 8 and tag_curb_points(sh.tag) != 5:
                back.append(("set_front_mode", 3))
            if back and rng.random() < (0.8 if family == "long" or sh.lasers == 128 else 0.55):
                op, v = pick(back)
            else:
                op, v = deck[dealt % len(deck)]
                dealt += 1
            step = {"op": op, "value": int(v)}
            steps.append(step)
            sh.setting(step)
    return steps


def replay(family, steps):
    """(step, class, expected front_scans or None, anchor?) for every step, from the settings alone"""
    sh = Shadow(family)
    for step in steps:
        cls = step_class(family, step)
        if step["op"] in ("batch", "callback"):
            yield step, cls, sh.expect(step), sh.is_anchor(step)
            sh.call(step)
        elif step["op"] == "readout":
            yield step, cls, None, False
            sh.readout(step)
        else:
            yield step, cls, None, False
            sh.setting(step)
