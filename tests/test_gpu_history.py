"""The result of a call must not depend on what the context did before.  One long-lived u.Context per test, never recreated; every call's
labels, summaries and read-outs against oracle B for the same input and the parameters in force.

(a) random histories (tests/fuzz_history.py: settings, batch calls through every entry point, groups of sweeps on the callback path,
read-outs; tests/test_history_cpu.py pins what the scripts contain), with urf_front_scans asserted wherever urf_policy::plan
(urban_road_filter_amd/csrc/urf_policy.hpp) decides without looking at the history; (b) directed histories: a walk through the laser counts,
a walk through the per-call tile stride, the row-major probation running out, the switches around the read-outs, the callback path through
settings changes, stage capture in mid-life.

A failure names the seed (or the directed test), the step and the steps so far: History.replay(steps) runs them again."""
import numpy as np
import pytest

import fuzz_history as H
import oracles as O
import urban_road_filter_amd as u
from hipmem import DevBuf
from test_gpu_async import records
from test_gpu_front_outputs import batch_readouts, same

pytestmark = pytest.mark.gpu
KEYS = ("status", "n_roi", "n_rings", "n_ring_pts", "n_road", "n_curb", "n_ring10")
BUSY = -7   # URF_ERR_BUSY
_REF = {}


def ref(family, name, tag):
    """Oracle B on one pool entry under one parameter set, computed once (labels, summary, stages, NaN azimuths); never modified."""
    key = (family, name, tag)
    if key not in _REF:
        x, y, z = H.pool(family)[name].cloud
        lb, ib, st = O.run_b(x, y, z, H.params_of(family, tag), debug=True)
        n_nan = int(((x == 0) & (y == 0) & (st["ring"] >= 0)).sum()) if ib["status"] == 0 else 0
        _REF[key] = (lb, ib, st, n_nan)
    return _REF[key]


_FRESH = {}


def fresh_fused(family, name, tag, mode, l128, long):
    """urf_front_scans of a context that has done nothing but classify this sweep under these settings.  A sweep in firing order: its
    first call; a row-major one: the second of two equal calls (the first sights the layout)."""
    key = (family, name, tag, mode, l128, long)
    if key not in _FRESH:
        e = H.pool(family)[name]
        bufs = [DevBuf.from_numpy(a) for a in e.cloud] + [DevBuf(len(e))]
        with u.Context(*H.FAMILIES[family]) as c:
            c.set_front_lasers128(l128)
            c.set_front_long_sweeps(long)
            c.set_front_mode(mode)
            c.set_params(H.params_of(family, tag))
            for _ in range(2 if e.kind.endswith("rows") else 1):
                c.classify_batch_soa(*bufs[:3], len(e), 1, bufs[3], None)
                c.synchronize()
            _FRESH[key] = c.front_scans()
        for b in bufs:
            b.free()
    return _FRESH[key]


class History:
    """Runs steps on one context and compares as it goes; keeps what a later read-out needs of the last call."""

    def __init__(self, family, ctx, name):
        self.family, self.ctx, self.name = family, ctx, name
        self.sh = H.Shadow(family)
        self.E = H.pool(family)
        self.done = []
        self.bufs = []              # the device arrays of the last batch call (a read-out may run it again)
        self.dl = None
        self.last = None            # (step, tag) of the last classify step
        self.row_gen = [0] * 4      # the submissions on each scratch row, as urf_ctx::row_gen counts them
        self.sweep = None           # (row, submission number) of the sweep waited for last
        self.fused = []             # front_scans() after every classify step
        self.wanted = []            # ... and what the settings alone say it is; None: the history may decide
        self.owed = None            # (step, speculations then) of an anchor step with fewer fused scans than the settings say
        self.let_off = 0            # ... and how often that has happened on this context
        self.next_ticket = 0        # the ticket the next sweep on the callback path takes (tickets count up from 0)

    # -- the steps --
    def run(self, step):
        self.done.append(step)
        try:
            op = step["op"]
            if op == "batch":
                self._batch(step)
            elif op == "callback":
                self._callback(step)
            elif op == "readout":
                self._readout(step)
            elif op == "set_stream":
                self.ctx.set_stream(None)
            else:
                if op == "set_params":
                    self.ctx.set_params(H.params_of(self.family, step["params"]))
                else:
                    getattr(self.ctx, op)(step["value"])
                self.sh.setting(step)
        except (AssertionError, u.UrfError) as e:
            raise AssertionError("%s: step %d failed: %s\nsteps so far:\n%s" % (self.name, len(self.done) - 1, e,
                                                                                "\n".join("  %r," % (s,) for s in self.done))) from e
        return self.fused[-1] if self.fused else None

    def replay(self, steps):
        for s in steps:
            self.run(s)

    def setting(self, op, value):
        return self.run({"op": op, "value": value})

    def params(self, tag):
        return self.run({"op": "set_params", "params": tag})

    def batch(self, scans, entry=None, info=True, repeat=False):
        uniform = len({len(self.E[n]) for n in scans}) == 1
        step = {"op": "batch", "entry": entry or ("soa" if uniform else "ragged"), "scans": list(scans), "pad": 333, "info": info}
        if repeat:
            step["repeat"] = True
        return self.run(step)

    def callback(self, scans, how="async16"):
        return self.run({"op": "callback", "how": how, "scans": list(scans)})

    def readout(self, *what):
        return self.run({"op": "readout", "what": list(what)})

    # -- a batch call --
    def _free(self):
        for b in self.bufs:
            b.free()
        self.bufs, self.dl = [], None

    def _batch(self, step):
        ctx, tag = self.ctx, self.sh.tag
        clouds = [self.E[n].cloud for n in step["scans"]]
        lens = [len(c[0]) for c in clouds]
        S, entry = len(clouds), step["entry"]
        ragged = entry == "ragged"
        lead, tail = (step["pad"] % 97, step["pad"]) if ragged else (0, 64)
        offs = lead + np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        total = int(offs[-1]) + tail
        self._free()
        dl = DevBuf(total)
        dl.fill(0xEE)
        di = DevBuf(32 * S) if step["info"] else None
        if di is not None:
            di.fill(0xEE)
        if entry in H.PC2_LAYOUT:
            pstep, ox, oy, oz = H.PC2_LAYOUT[entry]
            raw = DevBuf.from_numpy(np.concatenate([records(*c, step=pstep, ox=ox, oy=oy, oz=oz) for c in clouds]))
            self.bufs = [raw]
            assert len(set(lens)) == 1
            ctx.classify_batch_pc2(raw, lens[0], S, pstep, ox, oy, oz, dl, di)
        else:
            planes = []
            for k in range(3):
                a = np.full(total, 7.5, np.float32)
                for c, o in zip(clouds, offs):
                    a[o:o + len(c[k])] = c[k]
                planes.append(DevBuf.from_numpy(a))
            self.bufs = planes
            if ragged:
                do = DevBuf.from_numpy(offs.astype(np.uint32))
                self.bufs = planes + [do]
                ctx.classify_batch_soa_ragged(*planes, do, max(lens), S, dl, di)
            else:
                ctx.classify_batch_soa(*planes, lens[0], S, dl, di)
        ctx.synchronize()
        self.bufs += [dl] + ([di] if di is not None else [])
        self.dl = dl
        L = dl.to_numpy(np.uint8)
        infos = di.to_numpy(np.uint32).reshape(S, 8) if di is not None else None
        inside = np.zeros(total, bool)
        for k, name in enumerate(step["scans"]):
            lb, ib, _, n_nan = ref(self.family, name, tag)
            got = L[offs[k]:offs[k] + lens[k]]
            inside[offs[k]:offs[k] + lens[k]] = True
            assert np.array_equal(got, lb), "scan %d (%s, %s): %d labels differ" % (k, name, tag, int((got != lb).sum()))
            if infos is not None:
                assert {f: int(v) for f, v in zip(KEYS, infos[k][:7].view(np.int32))} == {f: ib[f] for f in KEYS}, "scan %d (%s, %s)" % (k, name, tag)
                assert infos[k][7] == n_nan, "scan %d (%s): NaN azimuths counted" % (k, name)
        assert (L[~inside] == 0xEE).all(), "label bytes outside the scans were written"
        self.last, self.sweep = (step, tag), None
        self._path(step)

    # -- a group of sweeps on the callback path --
    def _reruns(self):
        return self.ctx.callback_path_state()[0]

    def _submitted(self, ticket):
        row = (ticket % 4) % self.sh.rows
        self.row_gen[row] += 1
        return row, self.row_gen[row]

    def _waited(self, row, gen, reruns):
        if reruns:   # (urf_classify_pc2_wait ran a voided sweep again: the row's latest submissions)
            self.row_gen[row] += reruns
            gen = self.row_gen[row]
        self.sweep = (row, gen)

    def _callback(self, step):
        ctx, tag = self.ctx, self.sh.tag
        names = step["scans"]
        if step["how"] == "xyz":
            assert len(names) == 1
            before = self._reruns()
            lab, info = ctx.classify_xyz(*self.E[names[0]].cloud)
            row, gen = self._submitted(self._tickets())
            self._waited(row, gen, self._reruns() - before)
            self._sweep_equal(lab, info, names[0], tag, 0)
        else:
            pstep = int(step["how"][5:])
            recs = [records(*self.E[n].cloud, step=pstep) for n in names]
            subs = []
            for n, r in zip(names, recs):
                t = ctx.classify_pc2_async(r, len(self.E[n]), pstep, 0, 4, 8)
                self._ticket_seen(t)
                subs.append((t,) + self._submitted(t))
            for k, (t, row, gen) in enumerate(subs):
                lab = np.full(len(self.E[names[k]]), 0xEE, np.uint8)
                before = self._reruns()
                info = ctx.classify_pc2_wait(t, lab)
                self._waited(row, gen, self._reruns() - before)
                self._sweep_equal(lab, info, names[k], tag, k)
        self._free()
        self.last = ({"op": "callback", "how": step["how"], "scans": [names[-1]]}, tag)
        self._path(step)

    def _tickets(self):
        """The ticket urf_classify_xyz took.  The call does not return it: this rests on urf_classify_xyz taking exactly ONE ticket per
        call (a submission and its wait); the next urf_classify_pc2_async, whose ticket is seen, would show a miscount (_ticket_seen)."""
        t = self.next_ticket
        self.next_ticket += 1
        return t

    def _ticket_seen(self, t):
        assert t == self.next_ticket, (t, self.next_ticket)
        self.next_ticket += 1

    def _sweep_equal(self, lab, info, name, tag, k):
        lb, ib, _, n_nan = ref(self.family, name, tag)
        assert np.array_equal(lab, lb), "sweep %d (%s, %s): %d labels differ" % (k, name, tag, int((lab != lb).sum()))
        assert {f: getattr(info, f) for f in KEYS} == {f: ib[f] for f in KEYS}, "sweep %d (%s, %s)" % (k, name, tag)
        assert info.n_nan_azimuth == n_nan, "sweep %d (%s): NaN azimuths counted" % (k, name)

    # -- the path --
    def _speculations(self):
        """urf_callback_path_state: 1 the speculative ring table, 8 the ring count of the row's previous call as its hint"""
        return self.ctx.callback_path_state()[1] & 9

    def _path(self, step):
        """urf_front_scans where the settings alone decide it (fuzz_history.Shadow.expect: an anchor step and a row-major call repeated are
        fully fused).  One thing may keep a scan of such a step from the fused kernels: k_ring_table speculates (it stops at the ring
        count of the row's previous call, and when no new ring has shown up for a while), a scan that proves a rule wrong is repaired and
        handed to the general kernels in the same call, and the context does without that rule from then on (urf_policy::fold, at the
        NEXT call).  There are two such rules (bits 1 and 8 of urf_callback_path_state), each given up once and for good: fewer fused scans
        than the settings say are let off at most twice per context, and only against that receipt -- the next call has folded a
        speculation away."""
        want = self.sh.expect(step)
        nf = self.ctx.front_scans()
        self.fused.append(nf)
        self.wanted.append(want)
        bits = self._speculations()
        if self.owed is not None:
            at, had = self.owed
            assert bits != had and not (bits & ~had), "step %d: fewer fused scans than the settings say, and no speculation was given up (%d -> %d)" % (at, had, bits)
            self.owed = None
        if want is not None and nf != want:
            assert nf < want, "urf_front_scans: %d, the settings alone say %d of these scans" % (nf, want)
            assert bits, "urf_front_scans: %d of %d, and the context does not speculate any more" % (nf, want)
            self.let_off += 1
            assert self.let_off <= 2, "urf_front_scans: %d of %d, for the third time on this context" % (nf, want)
            self.owed = (len(self.done) - 1, bits)
        if want == 0:
            assert nf == want, "urf_front_scans: %d, the settings alone say %d (mode %d, %s, switches %d%d, capture %d, read-back state %r)" % (
                nf, want, self.sh.mode, self.sh.tag, self.sh.l128, self.sh.long, self.sh.capture, self.sh.wrs)
        self.sh.call(step, fused_seen=nf > 0)

    def finish(self):
        """a last call for the receipt that is still owed"""
        if self.owed is not None:
            self.batch(["few"])
        assert self.owed is None

    # -- read-outs of the last call --
    def _readout(self, step):
        ctx = self.ctx
        (last, tag) = self.last
        names = last["scans"]
        refs = [ref(self.family, n, tag) for n in names]
        stride = max(len(self.E[n]) for n in names)
        before = self.dl.to_numpy(np.uint8).copy() if self.dl is not None else None
        busy = self.sweep is not None and self.row_gen[self.sweep[0]] != self.sweep[1]
        refused = []
        for what, k in step["what"]:
            n = len(self.E[names[k]])
            st = refs[k][2]
            try:
                if what == "ordered":
                    got = ctx.ordered_indices(n, scan=k)
                    for g, key in zip(got, ("road_order", "curb_order", "ring10_order")):
                        assert np.array_equal(g, st[key]), (what, k, names[k], key, len(g), len(st[key]))
                elif what == "marker":
                    got = ctx.marker_points(scan=k)
                    assert got.shape == st["marker_pts"].shape and np.array_equal(got.view(np.uint32), st["marker_pts"].view(np.uint32)), (what, k, names[k])
                elif what == "batch":
                    for s, got in enumerate(batch_readouts(ctx, len(names), stride)):
                        same(got, refs[s][2], (what, s, names[s]))
                else:
                    assert what == "detect", what
                    got = ctx.read_stage(u.STAGE_DETECT, n, scan=k)
                    assert np.array_equal(got, st["detect"]), (what, k, names[k], int((got != st["detect"]).sum()))
                refused.append(False)
            except u.UrfError as e:
                # include/urf.h: a sweep whose scratch row a later submission has overtaken is refused, and only that
                assert busy and e.code == BUSY, (what, k, e)
                refused.append(True)
            else:
                assert not busy, "%s: served although a later submission has overtaken the sweep's row" % what
        if before is not None:
            assert np.array_equal(self.dl.to_numpy(np.uint8), before), "a read-out wrote the caller's labels"
        self.sh.readout(step, busy=refused)

    def close(self):
        self._free()


def history(family, name):
    return History(family, u.Context(*H.FAMILIES[family]), name)


def tag_of(family, L, wide=True, cp=5):
    return next(t for t in H.param_pool(family) if t.startswith("L%d/%s/cp%d/" % (L, "wide" if wide else "default", cp)))


# ---- (a) the random histories ----
@pytest.mark.parametrize("family,seed", [(f, s) for f in ("small", "long") for s in H.SEEDS[f]])
def test_random_history(family, seed):
    h = history(family, "script(%d, %r)" % (seed, family))
    try:
        h.replay(H.script(seed, family))
        h.finish()
    finally:
        h.close()
        h.ctx.close()


def test_fresh_contexts_fuse_the_pool():
    """What the path assertions take as certain, on contexts without a history: every sweep of the pool's four shapes is fused, in firing
    order and (from its second call) row-major, under the wide and the default region of interest -- mode 2 with curbPoints 5 at every
    laser count, mode 3 with curbPoints 3 at 64 lasers.  The sweeps with a firing astride a sector border (fuzz_history.ASTRIDE_COLS) are
    handed back where the star-shaped search is on.  One analytic and one sensor-like scene of each."""
    for tag, p in H.param_pool("small").items():
        L, cp = H.tag_lasers(tag), H.tag_curb_points(tag)
        if not H.front_curb_points_ok(3 if L == 64 else 2, L, cp):
            continue
        mode = 2 if cp == 5 else 3
        for e in H.organised("small"):
            if e.lasers != L or e.kind == "cut" or e.name[-2:] not in ("s1", "s4"):
                continue
            if e.kind.startswith("astride") and not p.star_shaped_method:
                continue   # (without the star-shaped search nothing is filed by sector: not what the path assertions rest on)
            n = fresh_fused("small", e.name, tag, mode, 1, 0)
            assert n == (0 if e.kind.startswith("astride") else 1), (e.name, tag, mode)


# ---- (b) directed histories ----
@pytest.fixture
def small():
    h = history("small", "directed")
    yield h
    h.close()
    h.ctx.close()


@pytest.fixture
def long():
    h = history("long", "directed")
    yield h
    h.close()
    h.ctx.close()


def test_laser_count_walk(small):
    """64 -> 128 -> 16 -> 32 -> 64 and back on one context: the lane tables, the row-major copies and the ring hints of one laser count are
    not the next one's."""
    h = small
    h.setting("set_front_lasers128", 1)
    h.setting("set_front_mode", 2)
    for L in (64, 128, 16, 32, 64, 32, 16, 128, 64):
        h.params(tag_of("small", L))
        for scans, repeat in ((["f%ds1" % L, "f%ds3" % L], False), (["r%ds1" % L, "r%ds3" % L], False), (["r%ds1" % L, "r%ds3" % L], True)):
            nf = h.batch(scans, repeat=repeat)
            if scans[0][0] == "f" or repeat:
                assert nf == 2, (L, scans, h.fused)
        if L in H.ASTRIDE_COLS:   # a sweep that k_front16 / k_front32 hand back, between two that they keep
            assert h.batch(["f%ds2" % L, "a%ds1" % L, "f%ds4" % L]) == 2, (L, h.fused)


def test_tile_stride_walk(long):
    """129 tiles, 3 tiles, 129 tiles again: the per-tile tables are laid out with the CALL's tile count.  urf_set_front_long_sweeps off in
    between: the 129-tile call falls to the general kernels and comes back."""
    h = long
    h.setting("set_front_long_sweeps", 1)
    h.setting("set_front_mode", 2)
    h.params(tag_of("long", 64))
    big, bigr, little, littler = ["F64s1", "F64s3"], ["R64s1", "R64s3"], ["f64s1", "f64s3"], ["r64s1", "r64s3"]
    assert h.batch(big) == 2
    h.batch(bigr)
    assert h.batch(bigr, repeat=True) == 2, h.fused
    assert h.batch(little) == 2
    h.batch(littler)
    assert h.batch(littler, repeat=True) == 2, h.fused
    assert h.batch(big) == 2
    h.setting("set_front_long_sweeps", 0)
    assert h.batch(big) == 0
    assert h.batch(little) == 2
    h.setting("set_front_long_sweeps", 1)
    assert h.batch(big) == 2
    h.batch(bigr)
    assert h.batch(["F64s1", "r64s1"]) >= 1, h.fused   # both strides in one ragged call


def test_probation_runs_out(small):
    """Mode 1, 64 lasers: three row-major sweeps are sighted (urf_policy::fold: rows_probation = 16); no scan confirms the sighting, since
    the sixteen batch calls that take the fused kernels on its strength hold sweeps in firing order (probation_batch counts each), and the
    call after them is back on the general kernels.  Two row-major calls afterwards: labels only, their path is recorded in DESIGN.md
    section 7 (a lapsed sighting is not renewed in mode 1: front_sight needs !front_rows)."""
    h = small
    rows, firing = ["r64s1", "r64s2", "r64s3"], ["f64s1", "f64s2", "f64s3"]
    assert h.batch(rows) == 0
    fused = [h.batch(firing) for k in range(18)]
    assert fused == [3] * 16 + [0] * 2, fused                            # calls 2..17 fused, 18 and 19 not
    after = [h.batch(rows), h.batch(rows)]
    assert all(0 <= n <= 3 for n in after), "row-major calls after the lapse: front_scans %r" % (after,)


def test_switches_around_the_read_outs(small):
    """urf_set_front_outputs turned on behind a fused call serves that call; the pre-pass of one call is not the next call's; sub-ranges
    through the single-scan entry points; urf_set_stream in between."""
    h = small
    h.setting("set_front_mode", 2)
    h.params(tag_of("small", 64))
    assert h.batch(["f64s1", "f64s2", "f64s3"]) == 3
    h.setting("set_front_outputs", 1)
    h.readout(("batch", 0), ("ordered", 1), ("marker", 1))
    assert h.ctx.front_scans() == 3                                      # no second run
    assert h.batch(["f64s4", "f64s3", "f64s2"]) == 3                     # other scans, nothing else changed
    h.readout(("batch", 0))
    assert h.batch(["f64s1", "f64s4", "f64s3"]) == 3                     # ... and once more: the SAME range of scans as the read-out before,
    h.readout(("batch", 0))                                              # of another call -- not the pre-pass that is still there
    h.readout(("ordered", 2), ("marker", 2), ("ordered", 0), ("marker", 0))
    assert h.batch(["f64s2", "f64s3", "f64s4"]) == 3
    h.readout(("marker", 0))                                             # (the single-scan range of the read-out before, likewise)
    h.run({"op": "set_stream"})
    h.readout(("batch", 0), ("marker", 1))
    assert h.ctx.front_scans() == 3
    assert h.batch(["f64s2", "f64s1", "f64s4"]) == 3
    h.readout(("marker", 0), ("batch", 0))


def test_callback_path_through_settings_changes(small):
    """Four row-major sweeps in flight until the callback path is fused, then other parameters, mode 0, mode 2 -- every group replays or
    rebuilds its captured sequences; one batch call on the same context in front of every group."""
    h = small
    h.params(tag_of("small", 64))
    group, between = ["r64s1", "r64s2", "r64s3", "r64s4"], ["f64s2", "f64s4"]
    for k in range(4):
        h.batch(between)
        if h.callback(group) == 1:
            break
    assert h.fused[-1] == 1, h.fused
    h.batch(between)
    assert h.callback(group, how="async32") == 1
    h.params(tag_of("small", 64, wide=False, cp=3))
    h.batch(between)
    assert h.callback(group) == 0                                        # (curbPoints 3 below mode 3)
    h.readout(("ordered", 0), ("marker", 0))
    h.setting("set_front_mode", 0)
    h.batch(between)
    assert h.callback(group) == 0
    h.setting("set_front_mode", 2)
    h.batch(between)
    h.callback(group)
    h.params(tag_of("small", 64))
    assert h.batch(between) == 2
    h.callback(group)
    h.callback(group)
    assert all(n in (0, 1) for n in h.fused[-2:]), "callback path, mode 2 after the changes: front_scans %r" % (h.fused[-3:],)


def test_capture_in_mid_life(small):
    """urf_enable_stage_capture(2) on a context that has been fused for a while allocates its scratch group then; the call behind it is a
    general call whose stages read back; capture off and urf_set_front_mode(2): fused again.  The same around a ring-sorted read-back."""
    h = small
    h.setting("set_front_mode", 2)
    h.params(tag_of("small", 64))
    scans = ["f64s1", "f64s3"]
    assert h.batch(scans) == 2
    assert h.batch(scans[::-1]) == 2
    h.setting("enable_stage_capture", 2)
    assert h.batch(scans) == 0
    h.readout(("detect", 0), ("detect", 1))
    for k, name in enumerate(scans):
        st = ref("small", name, h.sh.tag)[2]
        assert np.array_equal(h.ctx.read_stage(u.STAGE_RING, len(h.E[name]), scan=k), st["ring"]), name
        assert np.array_equal(h.ctx.read_stage(u.STAGE_SECTOR, len(h.E[name]), scan=k), st["sector"]), name
    h.setting("enable_stage_capture", 0)
    h.setting("set_front_mode", 2)
    assert h.batch(scans) == 2
    h.readout(("detect", 1))                                             # a ring-sorted read-back: the context keeps to the general kernels ...
    assert h.batch(scans) == 0
    h.setting("set_front_mode", 2)                                       # ... until it is asked again
    assert h.batch(scans) == 2
