"""The particle filter's stages chained on long-lived handles while the cloud resizes (tests/filter_cycle_cases.py; the scenario is
proved non-vacuous by tests/test_filter_cycle_cpu.py): one motion updater, one sensor updater, one estimator and one adaptive resampler
run four cycles on two buffer pairs of 1537 records whose particle count goes 1025 -> some hundreds -> up -> down -> up.

The run is made once and recorded: before every stage the whole of both buffer pairs and of the stages' output buffers is downloaded,
after it again.  Every stage is then judged three ways, always from the stage's own downloaded input, so nothing builds up:

  (a) against the numpy restatement, by the rule the stage's own test uses -- bytes for the surface motion and constraint, the field
      errors and the likelihood chain (tests/test_gpu_band_field.py's _same), refine, the Stein step, the visualisation pack, the
      resampler's sources and n_meas; tests/test_gpu_particle_init.py's _assert_cloud for the init slices and the perturbed copies;
      tests/test_gpu_hypotheses.py's _check_estimate for every estimate; bins and clusters exact unless filter_cycle_cases.undecided
      flags a particle on a bin edge, and n_new == the KLD bound of the device's own k always;
  (b) against the same call on fresh handles and fresh buffers of exactly n records -- the same bytes, no tolerance: what catches stale
      scratch, stale tables and handle state;
  (c) against the buffers themselves: everything outside the records the stage may write holds its bytes.

Then: every handle used at n = 63 after n = 1025, the sharded filter fed the chain's states, and cycle 1 (the one with the asynchronous
update) five times over without a download between its stages.
"""
import ctypes as C
import struct
import time

import numpy as np
import pytest

import adaptive_ref as ar
import filter_cycle_cases as fc
import particle_init_ref as pref
import pf_cycle_cases as pc
import surface_ref as sr

pytestmark = pytest.mark.gpu
F = np.float32
POSE, ATTR = 32, 36
AUX = {"errors": 4 * fc.N_BEAMS, "rows": 16, "labels": 4, "viz": 28}      # bytes per particle of the stages' output buffers
_T0 = [None]
_LINES = {}


# ---- the device side: fields, handles, buffers ------------------------------------------------------------------------------------------
class _Device:
    def __init__(self, ra, orc, ctx):
        self.ra, self.ctx = ra, ctx
        self.w = fc.World(ra, orc)
        self.hm = ra.import_hip_map(ctx, self.w.v, self.w.f)
        self.dense = ra.DistanceFieldHip(self.hm, cell=fc.CELL)
        self.banded = ra.DistanceFieldHip.banded(self.hm, cell=fc.CELL, band=fc.BAND)
        table, coarse, bricks = self.banded.download_banded()
        self.w.set_fields(self.dense.download(), dict(table=table, coarse=coarse, bricks=bricks))

    def field(self, cycle):
        return self.banded if fc.field_kind(cycle) == "banded" else self.dense

    def close(self):
        self.banded.close()
        self.dense.close()


def _kld(ra):
    p = fc.KLD
    return ra.kld_params(bin_xyz=p.bin_xyz, bin_rpy=p.bin_rpy, min_likelihood_rel=p.min_likelihood_rel, epsilon=p.epsilon, z=p.z, n_min=p.n_min,
                         n_max=p.n_max)


def _pf_params():
    from rmcl_amd import types as T
    return T.pf_params(dist_sigma=fc.DIST_SIGMA, max_n_meas=fc.MAX_N_MEAS, correspondence_type=1)


class _Handles:
    """what a node keeps for its lifetime: a motion updater, a sensor updater, an estimator, an adaptive resampler"""

    def __init__(self, dev):
        from rmcl_amd import types as T
        ra = dev.ra
        self.motion = ra.TFMotionUpdaterHip(dev.hm, check_collision=True)
        self.motion.surface = sr.to_capi(ra, fc.SURFACE)
        self.upd = ra.PCDSensorUpdaterHip(dev.hm)
        self.upd.config = _pf_params()
        self.upd.init()
        self.est = ra.PoseEstimatorHip(dev.ctx)
        self.est.kld = _kld(ra)
        self.rs = ra.AdaptiveResamplerHip(dev.ctx, seed=fc.SEED)
        self.rs.kld = _kld(ra)
        self.rs.config = T.gladiator_config(**fc.NOISE)

    def close(self):
        for h in (self.motion, self.upd, self.est, self.rs):
            h.close()


class _Buffers:
    """two pose / attribute pairs with `guard` records of 0xFF on both sides, and the stages' output buffers, all filled with 0xFF"""

    def __init__(self, dev, capacities, guard):
        self.dev, self.cap, self.guard, self.live = dev, tuple(capacities), guard, 0
        ff = lambda nbytes: dev.ra.DeviceArray.from_host(dev.ctx, np.full(max(nbytes, 1), 0xFF, np.uint8))
        self.d = {}
        for k, cap in enumerate(self.cap):
            self.d["p%d" % k], self.d["a%d" % k] = ff((cap + 2 * guard) * POSE), ff((cap + 2 * guard) * ATTR)
        for name, rec in AUX.items():
            self.d[name] = ff(max(self.cap) * rec)

    def P(self, pair=None, first=0):
        return self.d["p%d" % (self.live if pair is None else pair)].ptr + (self.guard + first) * POSE

    def A(self, pair=None, first=0):
        return self.d["a%d" % (self.live if pair is None else pair)].ptr + (self.guard + first) * ATTR

    def aux(self, name):
        return self.d[name].ptr

    def snapshot(self):
        return {k: v.download() for k, v in self.d.items()}

    def upload(self, snap):
        for k, v in self.d.items():
            v.upload(snap[k])

    def put(self, pair, first, poses, attrs):
        """records first .. of a pair, from the host"""
        L, ctx = self.dev.ra._capi.lib(), self.dev.ctx
        for ptr, arr in ((self.P(pair, first), poses), (self.A(pair, first), attrs)):
            arr = np.ascontiguousarray(arr)
            self.dev.ra._capi.check(L.rmclhip_memcpy_h2d(ctx.handle, C.c_void_p(ptr), arr.ctypes.data_as(C.c_void_p), arr.nbytes))

    def free(self):
        for v in self.d.values():
            v.free()


def _records(snap, kind, pair, guard):
    """the records of a snapshot's pose ("p") or attribute ("a") buffer without the guards, as bytes [capacity, record size]"""
    rec = POSE if kind == "p" else ATTR
    raw = snap["%s%d" % (kind, pair)].reshape(-1, rec)
    return raw[guard:len(raw) - guard]


def _cloud(snap, pair, guard, first, count):
    from rmcl_amd import types as T
    p = _records(snap, "p", pair, guard)[first:first + count]
    a = _records(snap, "a", pair, guard)[first:first + count]
    return np.ascontiguousarray(p).reshape(-1).view(T.TRANSFORM).copy(), np.ascontiguousarray(a).reshape(-1).view(T.PARTICLE_ATTRIBUTES).copy()


# ---- the stages: call(h, b, at, count, first, fresh) -> dict(result, poses, attrs, other, aux) ---------------------------------------------
# at: the first record in the live pair, first: the global index of that particle (an init slice's).  poses / attrs: the stage may
# write the records [at, at + count) of the live pair; other: records [0, other) of the other pair;
# aux: {name: bytes written from the start of that output buffer}.  fresh: handles that have not seen the stages before this one.
def _refine_capi(ra):
    p = fc.REFINE
    return ra.refine_params(iterations=p["iterations"], dof_mask=p["dof_mask"], max_dist=float(p["max_dist"]), max_step_trans=float(p["max_step_trans"]),
                            max_step_rot=float(p["max_step_rot"]), lambda0=float(p["lambda0"]))


def _stein_capi(ra, cycle):
    p = fc.stein_params(cycle)
    return ra.stein_params(**{k: (int(v) if k in ("iterations", "dof_mask", "max_per_bin", "seed", "step") else float(v)) for k, v in p.items()})


def _set_sensor(h, dev, cycle):
    h.upd.set_field(dev.field(cycle))
    h.upd.setInput(dev.w.beams[cycle], dev.w.Tsb)


def s_init_uniform(dev, epoch):
    def call(h, b, at, count, first, fresh):
        dev.ra.init_particles_uniform(dev.ctx, b.P(first=at), b.A(first=at), fc.BOX[0], fc.BOX[1], fc.SEED, epoch=epoch,
                                      first=first, count=count)
        return dict(result=None, poses=True, attrs=True)
    return call


def s_init_pose(dev):
    from rmcl_amd import types as T

    def call(h, b, at, count, first, fresh):
        err = dev.ra.init_particles_pose(dev.ctx, b.P(first=at), b.A(first=at), T.transform_from_rpy(*fc.TRUTH0), fc.POSE_COV, fc.SEED,
                                         epoch=fc.EPOCH, first=first, count=count)
        return dict(result=err, poses=True, attrs=True)
    return call


def s_constrain(dev):
    def call(h, b, at, count, first, fresh):
        stats = dev.ra.constrain_to_surface(h.motion, b.P(first=at), b.A(first=at), count, sr.to_capi(dev.ra, fc.SURFACE))
        return dict(result=stats, poses=True, attrs=True)
    return call


def s_motion(dev, cycle):
    def call(h, b, at, count, first, fresh):
        h.motion.update(b.P(), b.A(), count, dev.w.steps[cycle], fc.FORGET_RATE)
        return dict(result=h.motion.surface_stats(), poses=True, attrs=True)
    return call


def s_sensor(dev, cycle, first_of_cycle):
    """the first update of a cycle swaps the field on the long-lived updater and gives it the cycle's beams; the second one finds them
    there.  Cycle ASYNC_CYCLE's updates are update(sync=False) + sync()."""
    def call(h, b, at, count, first, fresh):
        if fresh or first_of_cycle:
            _set_sensor(h, dev, cycle)
        h.upd.set_error_output(b.aux("errors"))
        if cycle == fc.ASYNC_CYCLE:
            h.upd.update(b.P(), b.A(), count, sync=False)
            h.upd.sync()
        else:
            h.upd.update(b.P(), b.A(), count)
        h.upd.set_error_output(None)
        return dict(result=None, attrs=True, aux={"errors": count * AUX["errors"]})
    return call


def s_move(dev, cycle):
    def call(h, b, at, count, first, fresh):
        if fresh:
            _set_sensor(h, dev, cycle)
        if fc.third_stage(cycle) == "refine":
            stats = h.upd.refine(b.P(), count, params=_refine_capi(dev.ra), results_dev=b.aux("rows"))
        else:
            stats = h.upd.stein_step(b.P(), count, params=_stein_capi(dev.ra, cycle), results_dev=b.aux("rows"))
        return dict(result=stats, poses=True, aux={"rows": count * AUX["rows"]})
    return call


def s_hypotheses(dev):
    def call(h, b, at, count, first, fresh):
        got = h.est.hypotheses(b.P(), b.A(), count, fc.MAX_HYPOTHESES, labels=b.aux("labels"))
        return dict(result=got, aux={"labels": count * AUX["labels"]})
    return call


def s_estimate(dev):
    def call(h, b, at, count, first, fresh):
        return dict(result=h.est.estimate(b.P(), b.A(), count))
    return call


def s_viz(dev):
    def call(h, b, at, count, first, fresh):
        host = dev.ra.pack_visualization(dev.ctx, b.P(), b.A(), count, fc.MAX_N_MEAS)
        assert dev.ra.pack_visualization(dev.ctx, b.P(), b.A(), count, fc.MAX_N_MEAS, out_dev=b.aux("viz")) is None
        return dict(result=host, aux={"viz": count * AUX["viz"]})
    return call


def s_resample(dev, cycle):
    def call(h, b, at, count, first, fresh):
        if fresh:
            h.rs.step = cycle
        assert h.rs.step == cycle                       # the long-lived resampler's own counter has got there
        other = 1 - b.live
        res = h.rs.update(b.P(), b.A(), b.P(other), b.A(other), count, capacity_new=b.cap[other])
        return dict(result=res, other=res["n_particles"])
    return call


def _stamp(b, n):
    """stamp = index on the live cloud, from the host (filter_cycle_cases.with_index_stamps)"""
    snap = {k: b.d[k].download() for k in ("p%d" % b.live, "a%d" % b.live)}
    poses, attrs = _cloud(snap, b.live, b.guard, 0, n)
    b.put(b.live, 0, fc.with_index_stamps(poses), attrs)


def _run_stage(log, name, cycle, call, h, b, first, count):
    """one stage on (h, b); log: None, or a list that receives the stage's record with the snapshots around it"""
    before = b.snapshot() if log is not None else None
    out = call(h, b, first, count, first, False)
    if log is not None:
        log.append(dict(name=name, cycle=cycle, call=call, first=first, count=count, live=b.live, guard=b.guard, cap=b.cap, before=before,
                        after=b.snapshot(), out=out))
    return out


def _start(dev, h, b, log, n0=fc.N0, n_uniform=fc.N_UNIFORM, epoch=fc.EPOCH):
    """the two init slices and the standalone constraint; returns n"""
    _run_stage(log, "init_uniform", -1, s_init_uniform(dev, epoch), h, b, 0, n_uniform)
    _run_stage(log, "init_pose", -1, s_init_pose(dev), h, b, n_uniform, n0 - n_uniform)
    _run_stage(log, "constrain", -1, s_constrain(dev), h, b, 0, n0)
    return n0


def _cycle(dev, h, b, log, c, n):
    """stages 1 to 6 of cycle c on n live particles; the pairs swap; returns the new n"""
    _run_stage(log, "motion", c, s_motion(dev, c), h, b, 0, n)
    _run_stage(log, "sensor", c, s_sensor(dev, c, True), h, b, 0, n)
    _run_stage(log, fc.third_stage(c), c, s_move(dev, c), h, b, 0, n)
    _run_stage(log, "sensor2", c, s_sensor(dev, c, False), h, b, 0, n)
    _run_stage(log, "hypotheses", c, s_hypotheses(dev), h, b, 0, n)
    _run_stage(log, "estimate", c, s_estimate(dev), h, b, 0, n)
    _run_stage(log, "viz", c, s_viz(dev), h, b, 0, n)
    _stamp(b, n)
    out = _run_stage(log, "resample", c, s_resample(dev, c), h, b, 0, n)
    b.live = 1 - b.live
    return out["other"]


def _kidnap(dev, h, b, log, c, n):
    first = n // 2
    _run_stage(log, "kidnap_uniform", c, s_init_uniform(dev, fc.KIDNAP_EPOCH), h, b, first, n - first)
    _run_stage(log, "kidnap_constrain", c, s_constrain(dev), h, b, first, n - first)


@pytest.fixture(scope="module")
def dev(ra, orc, ctx):
    if _T0[0] is None:
        _T0[0] = time.time()
    d = _Device(ra, orc, ctx)
    yield d
    d.close()


@pytest.fixture(scope="module")
def run(dev):
    """the scenario on one long-lived set of handles: (handles, buffers, the stages' records, n of every cycle and after the last)"""
    h, b = _Handles(dev), _Buffers(dev, (fc.CAPACITY, fc.CAPACITY), fc.GUARD)
    log, ns = [], []
    n = _start(dev, h, b, log)
    for c in range(fc.N_CYCLES):
        ns.append(n)
        n = _cycle(dev, h, b, log, c, n)
        if c == fc.KIDNAP_AFTER:
            _kidnap(dev, h, b, log, c, n)
    ns.append(n)
    yield h, b, log, ns
    h.close()
    b.free()


# ---- bytes ------------------------------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _same(got, ref):
    """tests/test_gpu_band_field.py's: equal to the bit, a NaN matching any NaN"""
    got, ref = np.asarray(got, F), np.asarray(ref, F)
    nan = np.isnan(ref)
    return got.shape == ref.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got)[~nan], _bits(ref)[~nan])


def _canon(x):
    """a result of the binding as something == compares byte for byte"""
    if isinstance(x, dict):
        return tuple((k, _canon(x[k])) for k in sorted(x))
    if isinstance(x, (list, tuple)):
        return tuple(_canon(v) for v in x)
    if isinstance(x, (np.ndarray, np.generic)):
        return np.asarray(x).tobytes()
    if isinstance(x, float):
        return struct.pack("<d", x)
    return x


def _outputs(rec):
    """everything a stage produced, as bytes: the records it may have written, the heads of its output buffers, its result"""
    g, live, after, out = rec["guard"], rec["live"], rec["after"], rec["out"]
    sl = slice(rec["first"], rec["first"] + rec["count"])
    got = {"result": _canon(out["result"]), "poses": _records(after, "p", live, g)[sl].tobytes(), "attrs": _records(after, "a", live, g)[sl].tobytes()}
    if out.get("other"):
        got["other"] = (_records(after, "p", 1 - live, g)[:out["other"]].tobytes(), _records(after, "a", 1 - live, g)[:out["other"]].tobytes())
    for name, nbytes in out.get("aux", {}).items():
        got[name] = after[name][:nbytes].tobytes()
    return got


def _differences(a, b):
    return [k for k in sorted(set(a) | set(b)) if a.get(k) != b.get(k)]


def _replay(dev, rec, call=None):
    """the stage of a record on fresh handles and fresh buffers of exactly `count` records holding its downloaded input: its _outputs"""
    h = _Handles(dev)
    b = _Buffers(dev, (rec["count"], rec["cap"][1 - rec["live"]] if rec["name"] == "resample" else 1), 0)
    try:
        poses, attrs = _cloud(rec["before"], rec["live"], rec["guard"], rec["first"], rec["count"])
        b.put(0, 0, poses, attrs)
        out = (rec["call"] if call is None else call)(h, b, 0, rec["count"], rec["first"], True)
        return _outputs(dict(rec, first=0, live=0, guard=0, after=b.snapshot(), out=out))
    finally:
        h.close()
        b.free()


# ---- (c): the buffers themselves ---------------------------------------------------------------------------------------------------------
def _touched_outside(rec):
    """names of the regions that changed although the stage may not write them"""
    g, live, before, after, out = rec["guard"], rec["live"], rec["before"], rec["after"], rec["out"]
    bad = []
    for kind, key, size in (("p", "poses", POSE), ("a", "attrs", ATTR)):
        for pair in (live, 1 - live):
            name = "%s%d" % (kind, pair)
            may = np.zeros(len(before[name]) // size, bool)
            if pair == live and out.get(key):
                may[g + rec["first"]:g + rec["first"] + rec["count"]] = True
            if pair != live and out.get("other"):
                may[g:g + out["other"]] = True
            same = (before[name].reshape(-1, size) == after[name].reshape(-1, size)).all(axis=1)
            if not same[~may].all():
                bad.append("%s records %s" % (name, (np.flatnonzero(~same & ~may)[:4] - g).tolist()))
    for name in AUX:
        nbytes = out.get("aux", {}).get(name, 0)
        if before[name][nbytes:].tobytes() != after[name][nbytes:].tobytes():
            bad.append("%s past byte %d" % (name, nbytes))
    return bad


def test_every_stage_leaves_the_rest_of_the_buffers_untouched(run):
    """(c): after an in-place stage the records [n, C), both guards, the other pair and the tails of the output buffers hold their bytes;
    after a resampling [n_new, C) of the destination and the whole source pair do"""
    h, b, log, ns = run
    assert len(log) == 3 + 8 * fc.N_CYCLES + 2
    for rec in log:
        assert _touched_outside(rec) == [], (rec["name"], rec["cycle"])
    # the guards were 0xFF when the buffers were made, so they still are
    last = log[-1]["after"]
    for name in ("p0", "a0", "p1", "a1"):
        size = POSE if name[0] == "p" else ATTR
        assert (last[name][:fc.GUARD * size] == 0xFF).all() and (last[name][-fc.GUARD * size:] == 0xFF).all()


def test_the_run_resized_the_cloud(run):
    """the device's own run met the conditions the CPU chain was chosen for: below 512, up again, never two wave multiples in a row"""
    h, b, log, ns = run
    print("[filter-cycle] n per cycle:", ns)
    small = [i for i, v in enumerate(ns) if v < 512]
    assert ns[0] == fc.N0 and small and any(ns[j] > ns[j - 1] for j in range(small[0] + 1, len(ns))), ns
    assert not any(ns[i] % 64 == 0 and ns[i + 1] % 64 == 0 for i in range(len(ns) - 1)), ns
    assert b.live == fc.N_CYCLES % 2 and h.rs.step == fc.N_CYCLES


# ---- (b): the replay on fresh handles -----------------------------------------------------------------------------------------------------
def test_every_stage_equals_its_replay_on_fresh_handles(dev, run):
    """(b): poses, attributes, result rows, errors, labels, counts and statistics of the long-lived handles are the bytes fresh handles
    give on fresh buffers of exactly n records holding the stage's downloaded input"""
    h, b, log, ns = run
    for rec in log:
        diff = _differences(_outputs(rec), _replay(dev, rec))
        assert diff == [], (rec["name"], rec["cycle"], rec["count"], diff)


# ---- (a): the restatements --------------------------------------------------------------------------------------------------------------
def _io(rec):
    """(poses, attrs) before and after, of the records the stage works on"""
    g, live = rec["guard"], rec["live"]
    return _cloud(rec["before"], live, g, rec["first"], rec["count"]) + _cloud(rec["after"], live, g, rec["first"], rec["count"])


def _check_init(rec, w, info):
    from test_gpu_particle_init import _assert_cloud
    _, _, p, a = _io(rec)
    what = "%s cycle %d" % (rec["name"], rec["cycle"])
    if rec["name"] == "init_pose":
        from rmcl_amd import types as T
        ref = pref.init_pose(rec["first"], rec["count"], T.transform_from_rpy(*fc.TRUTH0), fc.POSE_COV, fc.SEED, fc.EPOCH)
        assert rec["out"]["result"] == pref.chol6(fc.POSE_COV)[1]
        _assert_cloud(p, a, ref[0], ref[1], False, what)
    else:
        epoch = fc.EPOCH if rec["name"] == "init_uniform" else fc.KIDNAP_EPOCH
        ref = pref.init_uniform(rec["first"], rec["count"], fc.BOX[0], fc.BOX[1], fc.SEED, epoch)
        _assert_cloud(p, a, ref[0], ref[1], True, what)


def _check_constrain(rec, w, info):
    p0, a0, p, a = _io(rec)
    ref = fc.constrain(w, p0, a0)
    assert rec["out"]["result"] == ref[2] and p.tobytes() == ref[0].tobytes() and a.tobytes() == ref[1].tobytes()
    assert ref[2]["n_snapped"] > 0 and ref[2]["n_missed"] > 0


def _check_motion(rec, w, info):
    p0, a0, p, a = _io(rec)
    ref = fc.motion(w, rec["cycle"], p0, a0)
    assert rec["out"]["result"] == ref[2], (rec["out"]["result"], ref[2])
    assert p.tobytes() == ref[0].tobytes(), pc.first_difference("motion %d" % rec["cycle"], "poses", p, ref[0])
    assert a.tobytes() == ref[1].tobytes(), pc.first_difference("motion %d" % rec["cycle"], "attributes", a, ref[1])
    info.update(killed=int(ref[3].sum()), surface=ref[2])


def _check_sensor(rec, w, info):
    p0, a0, p, a = _io(rec)
    n = rec["count"]
    e_ref, a_ref, stored = fc.sensor(w, rec["cycle"], p0, a0)
    e = rec["after"]["errors"][:n * AUX["errors"]].view(F).reshape(n, fc.N_BEAMS)
    assert _same(e, e_ref), "%d errors differ" % (_bits(e) != _bits(e_ref)).sum()
    assert np.array_equal(a["likelihood"]["n_meas"], a_ref["likelihood"]["n_meas"])
    assert _same(a["likelihood"]["mean"], a_ref["likelihood"]["mean"]) and _same(a["likelihood"]["sigma"], a_ref["likelihood"]["sigma"])
    assert a["state_sigma"].tobytes() == a0["state_sigma"].tobytes()
    if rec["name"] == "sensor":
        info.update(far=int((~stored).sum()), stored=int(stored.sum()))


def _check_move(rec, w, info):
    p0, a0, p, a = _io(rec)
    n = rec["count"]
    ref = fc.move(w, rec["cycle"], p0)
    rows = rec["after"]["rows"][:n * AUX["rows"]]
    assert rows.tobytes() == ref[1].tobytes(), "%s rows: %d differ" % (rec["name"], (rows.view(ref[1].dtype) != ref[1]).sum())
    assert p.tobytes() == ref[0].tobytes(), pc.first_difference("%s %d" % (rec["name"], rec["cycle"]), "poses", p, ref[0])
    got = rec["out"]["result"]
    if rec["name"] == "refine":         # (tests/test_gpu_refine.py holds the cost sums to the bit for up to five particles only)
        assert all(got[k] == ref[2][k] for k in ("n_particles", "n_moved", "n_no_beams", "n_not_finite")), (got, ref[2])
        assert ref[2]["n_moved"] > 0
    else:
        assert all(got[k] == ref[2][k] for k in ("n_particles", "n_not_finite", "n_no_beams", "n_bins", "n_thinned_bins")), (got, ref[2])
        assert struct.pack("<d", got["cost_sum"]) == struct.pack("<d", ref[2]["cost_sum"])
        assert p.tobytes() != p0.tobytes()
    info["moved"] = ref[2]


def _check_hypotheses(rec, w, info):
    from test_gpu_hypotheses import _check_estimate
    p0, a0, _, _ = _io(rec)
    n = rec["count"]
    got = rec["out"]["result"]
    labels = rec["after"]["labels"][:n * 4].view(np.uint32)
    und = fc.undecided(p0, a0, fc.KLD)
    ref = fc.clusters(p0, a0)
    info.update(n_clusters=got["n_clusters"], undecided=int(und.sum()), counted=int(ar.counted_mask(p0, a0, fc.KLD).sum()))
    assert len(got["hypotheses"]) == min(got["n_clusters"], fc.MAX_HYPOTHESES) >= 1
    if not und.any():
        assert got["n_clusters"] == ref["n_clusters"] and np.array_equal(labels, ref["labels"])
        for r, (g, x) in enumerate(zip(got["hypotheses"], ref["hypotheses"])):
            for k in ("key_min", "weight", "n_bins", "nparticles"):
                assert g[k] == x[k], (rec["cycle"], r, k, g[k], x[k])
            assert g["weight_share"] == float(x["weight"]) / float(ref["total"])
    # every hypothesis's estimate, over the members the device's own labels name
    for r, g in enumerate(got["hypotheses"]):
        m = np.flatnonzero(labels == r)
        assert len(m) == g["nparticles"] > 0
        _check_estimate(p0[m], a0[m], g, pc.estimate_ref(p0[m], a0[m]), g["n_bins"] == 1 or len(m) == 1, "cycle %d, hypothesis %d" % (rec["cycle"], r))


def _check_estimate_stage(rec, w, info):
    from test_gpu_hypotheses import _check_estimate
    p0, a0, _, _ = _io(rec)
    got = rec["out"]["result"]
    assert got["nparticles"] == rec["count"]
    _check_estimate(p0, a0, got, pc.estimate_ref(p0, a0), False, "cycle %d, the estimate" % rec["cycle"])
    info["error"] = fc.position_error(got["pose"], w.truth[rec["cycle"] + 1][0])


def _check_viz(rec, w, info):
    p0, a0, _, _ = _io(rec)
    n = rec["count"]
    ref = pref.pack_visualization(p0, a0, fc.MAX_N_MEAS)
    got = rec["out"]["result"]
    assert list(got) == list(ref)
    for k in ref:
        assert got[k].tobytes() == ref[k].tobytes(), k
    assert rec["after"]["viz"][:n * AUX["viz"]].tobytes() == np.concatenate([ref[k] for k in ref]).tobytes()


def _check_resample(rec, w, info, tol=fc.UNDECIDED_TOL):
    from test_gpu_particle_init import _assert_cloud
    p0, a0, _, _ = _io(rec)
    c, n = rec["cycle"], rec["count"]
    res = rec["out"]["result"]
    assert np.array_equal(p0["stamp"], np.arange(n))
    u = int(fc.undecided(p0, a0, fc.KLD, tol).sum())
    k_ref = ar.count_bins(p0, a0, fc.KLD)[0]
    assert abs(res["bins"] - k_ref) <= u, (res["bins"], k_ref, u)
    n_new = res["n_particles"]
    assert n_new == fc.n_new_of(res["bins"])                                  # always: the bound of the device's own k, clamped
    pn_ref, an_ref, src = ar.systematic(p0, a0, n_new, ar.gladiator_cfg(**fc.NOISE), fc.SEED, c)
    pn, an = _cloud(rec["after"], 1 - rec["live"], rec["guard"], 0, n_new)
    assert np.array_equal(pn["stamp"], src)                                   # the source of every slot
    assert an.tobytes() == an_ref.tobytes()                                   # (the perturbed copies' scaled n_meas among them)
    first_of_run = np.ones(n_new, bool)
    first_of_run[1:] = src[1:] != src[:-1]
    assert pn[first_of_run].tobytes() == p0[src[first_of_run]].tobytes()      # first copies: the source's bytes
    if (~first_of_run).any():
        _assert_cloud(pn[~first_of_run], an[~first_of_run], pn_ref[~first_of_run], an_ref[~first_of_run], False, "cycle %d, perturbed copies" % c)
    info.update(n=n, n_new=n_new, k=res["bins"])


CHECKS = {"init_uniform": _check_init, "init_pose": _check_init, "kidnap_uniform": _check_init, "constrain": _check_constrain,
          "kidnap_constrain": _check_constrain, "motion": _check_motion, "sensor": _check_sensor, "sensor2": _check_sensor, "refine": _check_move,
          "stein": _check_move, "hypotheses": _check_hypotheses, "estimate": _check_estimate_stage, "viz": _check_viz, "resample": _check_resample}


@pytest.mark.parametrize("cycle", [-1] + list(range(fc.N_CYCLES)))
def test_every_stage_is_its_restatement(dev, run, cycle):
    """(a); cycle -1: the two init slices and the standalone constraint.  The kidnap is judged with the cycle it follows."""
    h, b, log, ns = run
    info = {}
    recs = [r for r in log if r["cycle"] == cycle]
    assert len(recs) == (3 if cycle < 0 else 8 + (2 if cycle == fc.KIDNAP_AFTER else 0))
    for rec in recs:
        CHECKS[rec["name"]](rec, dev.w, info)
    if cycle >= 0:
        info["cycle"] = cycle
        _LINES[cycle] = fc.line(info) + ", estimate %.3f m from the truth" % info["error"]
        print("[filter-cycle] " + _LINES[cycle])
        assert info["far"] >= 20 and info["stored"] >= 500


# ---- small after large, on every handle ------------------------------------------------------------------------------------------------------
def test_small_after_large_on_every_handle(dev):
    """the start and cycle 0 at n = 1025, then at n = 63 on the same handles and buffers (the small cloud: the head of a second init),
    against the same 63 on fresh handles and buffers: every stage's outputs byte for byte"""
    n_small, n_uniform, epoch = 63, 40, 5
    h, b = _Handles(dev), _Buffers(dev, (fc.CAPACITY, fc.CAPACITY), fc.GUARD)
    fh, fb = _Handles(dev), _Buffers(dev, (n_small, fc.CAPACITY), 0)
    try:
        _cycle(dev, h, b, None, 0, _start(dev, h, b, None))
        b.live, h.rs.step = 0, 0
        seen, fresh = [], []
        for hh, bb, log in ((h, b, seen), (fh, fb, fresh)):
            n = _start(dev, hh, bb, log, n_small, n_uniform, epoch)
            assert _cycle(dev, hh, bb, log, 0, n) >= 1
        assert len(seen) == len(fresh) == 11
        for r_seen, r_fresh in zip(seen, fresh):
            assert _touched_outside(r_seen) == [], r_seen["name"]
            diff = _differences(_outputs(r_seen), _outputs(r_fresh))
            assert diff == [], (r_seen["name"], diff)
        moved = [r for r in seen if r["name"] == "refine"][0]["out"]["result"]
        assert moved["n_particles"] == n_small and moved["n_moved"] > 0
    finally:
        for x in (h, fh):
            x.close()
        for x in (b, fb):
            x.free()


# ---- the sharded twin -----------------------------------------------------------------------------------------------------------------------
def test_sharded_twin_follows_the_chain(dev, run):
    """ShardedParticleFilterHip on a loopback communicator of three ranks, given the chain's state at every cycle's start (a ragged
    split whenever n is no multiple of 3): motion update, sensor update, on cycles 0 and 2 refine and the second update, and the pose
    hypotheses give the single-device chain's bytes.  The sharded API has neither a Stein step nor an adaptive resampler: on cycles 1
    and 3 the twin stops after the first sensor update, and no cycle resamples."""
    from test_gpu_hypotheses import _same as same_hypotheses
    h, b, log, ns = run
    ra, w = dev.ra, dev.w
    sh = ra.ShardedParticleFilterHip(w.v, w.f, devices=(0, 0, 0), loopback=True)
    est = ra.PoseEstimatorHip(dev.ctx)
    est.kld = _kld(ra)
    try:
        sh.config_ = _pf_params()
        sh.set_surface(sr.to_capi(ra, fc.SURFACE))
        ragged = 0
        for c in range(fc.N_CYCLES):
            recs = {r["name"]: r for r in log if r["cycle"] == c}
            n = recs["motion"]["count"]
            ragged += n % 3 != 0
            p0, a0, p1, a1 = _io(recs["motion"])
            sh.set_particles(p0, a0)
            if fc.field_kind(c) == "banded":
                sh.set_field_banded(cell=fc.CELL, band=fc.BAND)
            else:
                sh.set_field(cell=fc.CELL)
            sh.motion_update(w.steps[c], fc.FORGET_RATE, check_collision=True)
            assert sh.surface_stats() == recs["motion"]["out"]["result"]
            got = sh.download()
            assert got[0].tobytes() == p1.tobytes() and got[1].tobytes() == a1.tobytes(), ("motion", c)
            sh.update(w.beams[c], w.Tsb)
            want = _io(recs["sensor"])[2:]
            if fc.third_stage(c) == "refine":
                stats = sh.refine(w.beams[c], w.Tsb, params=_refine_capi(ra))
                single = recs["refine"]["out"]["result"]
                assert all(stats[k] == single[k] for k in ("n_particles", "n_moved", "n_no_beams", "n_not_finite"))
                sh.update(w.beams[c], w.Tsb)
                want = _io(recs["sensor2"])[2:]
            got = sh.download()
            assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), ("update", c)
            hyp = sh.pose_hypotheses(_kld(ra), fc.MAX_HYPOTHESES)
            d_p, d_a = ra.DeviceArray.from_host(dev.ctx, want[0]), ra.DeviceArray.from_host(dev.ctx, want[1])
            assert same_hypotheses(hyp, est.hypotheses(d_p, d_a, n, fc.MAX_HYPOTHESES)), c
            if fc.third_stage(c) == "refine":
                assert same_hypotheses(hyp, recs["hypotheses"]["out"]["result"]), c
        assert ragged >= 2
    finally:
        est.close()
        sh.close()


# ---- order between handles ------------------------------------------------------------------------------------------------------------------
def test_cycle_one_five_times_without_a_download_between_its_stages(dev, run):
    """every handle owns a stream and the buffers are shared: cycle 1 (update(sync=False) + sync()) from the same uploaded state, five
    times on the long-lived handles with nothing downloaded between its stages until the stamps are written, just before the
    resampling -- five identical results, the chain's"""
    h, b, log, ns = run
    c = fc.ASYNC_CYCLE
    recs = [r for r in log if r["cycle"] == c]
    start, end = recs[0], [r for r in recs if r["name"] == "resample"][0]
    live_end, step_end = b.live, h.rs.step
    want = (end["out"]["result"], end["after"])
    try:
        for rep in range(5):
            b.upload(start["before"])
            b.live, h.rs.step = start["live"], c
            n_new = _cycle(dev, h, b, None, c, start["count"])
            after = b.snapshot()
            assert n_new == want[0]["n_particles"]
            assert [k for k in after if after[k].tobytes() != want[1][k].tobytes()] == [], rep
    finally:
        b.upload(log[-1]["after"])
        b.live, h.rs.step = live_end, step_end


def test_zz_wall_time_of_this_module():
    """printed for the record: one line per cycle and the module's wall time"""
    for c in sorted(_LINES):
        print("[filter-cycle] " + _LINES[c])
    if _T0[0] is not None:
        print("[filter-cycle] wall time of tests/test_gpu_filter_cycle.py: %.1f s" % (time.time() - _T0[0]))
