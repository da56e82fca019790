"""Writes tests/golden/g11_micp_digests.json: sha256 of what every MICP entry point returns -- the transform, the statistics and, for one
sensor, the 96 folded moments of rmclhip_debug_micp_moments -- so that a change which only moves the kernels' text cannot move a bit
unseen (the other MICP tests allow 1e-6 on a pose: a reordered float expression passes them).

cases()  name -> function(ra, ctx) -> {field: sha256 hex, or an integer}; tests/test_gpu_micp_digests.py recomputes them one by one.
Every case pins its traversal kind and PROVES from rmclhip_rcc_micp_fast_info which loop form served the call: a case that lands in
another form fails instead of digesting other code.

One sensor (rmclhip_rcc_correct_once), the spherical scan of test_moments_formed_in_the_find_epilogue_equal_the_separate_pass scaled to
H x W on micp_multi_cases' meshes (room30k leaves correspondences undecided, cube none), gate 0.5 m, 8 iterations, three learning
calls in mode 3 first:
    iter_*      mode 0: n_iter 0 (k_micp_init), 1 and 8 (k_micp_iter, k_micp_close); an unmasked O1Dn dataset with NaN directions
    m3_*        mode 3 (k_micp_moments + k_micp_fast_loop in one workgroup): 64 x 512, 30 x 500 (ragged last mask word), cube (lone wave)
    m4_*        mode 4 (find epilogue + device loop): kind 23 64 x 512 (128 rows, one workgroup folds), kind 23 100 x 1000 (400 rows,
                eight workgroups fold), kind 2 30 x 500 (256 rows: the fold's threshold), kind 32 100 x 1000
    m1_*        mode 1 (k_micp_publish + host iterations): the same four, and kind 24 30 x 500 (no epilogue: 59 rows of k_micp_moments)
    fallback_*  a fresh operator whose pre-transform leaves the initial caps (code 1, gate 1 m) / under a 5 cm gate (code 2, more than
                4096 undecided); both served by the per-iteration form
Rigs (rmclhip_micp_correct_once, every operator at kind 2, the rule's choice for these sizes): mixed4, eight, cube6 and near in the
per-iteration, host and device form; mid (hand-over from the host form to the device loop); far (overflow, served per iteration).
Code that stays in kernels.hip: statistics_p2l on a 64 x 512 view, a batch correction of 4 poses.

Needs a GPU and the built library; the committed file holds what the kernels wrote BEFORE the MICP kernels moved into micp.hip:

    python tests/golden/make_g11_micp_digests.py
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

OUT = os.path.join(HERE, "g11_micp_digests.json")
N_ITER = 8
KEYS = ("attempts", "done", "cap_exits", "overflows", "host_loops")
TRUTH = ((1.5, -2.0, 1.6), (0.02, -0.03, 0.4))
PERT = ((0.03, -0.02, 0.015), (0.004, -0.003, 0.008))
FAR_PERT = ((0.12, 0.08, -0.03), (0.01, -0.01, 0.03))     # |t| above the initial tau cap of 0.1 m


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


_MAPS = {}


def hip_map(ra, ctx, name):
    import micp_multi_cases as mc
    if (id(ctx), name) not in _MAPS:
        v, f, _ = mc.mesh_arrays(name)
        _MAPS[(id(ctx), name)] = ra.import_hip_map(ctx, v, f)
    return _MAPS[(id(ctx), name)]


def scaled_model(H, W):
    from rmcl_amd import synthetic as syn
    model = syn.model_c2()
    model.phi.inc = model.phi.inc * 128.0 / H
    model.phi.size = H
    model.theta.inc = model.theta.inc * 1024.0 / W
    model.theta.size = W
    return model


def operator(ra, hm, H, W, kind, sensor="spherical"):
    """the operator of one scan measured at the truth, its traversal pinned"""
    from rmcl_amd import synthetic as syn, types as T
    truth = T.transform_from_rpy(*TRUTH)
    model = scaled_model(H, W)
    if sensor == "spherical":
        rcc = ra.RCCHipSpherical(hm)
        rcc.setTsb(T.identity())
        rcc.setModel(model)
        rcc.set_traversal(kind)
        rcc.find(truth)
        rcc.set_dataset_from_ranges(rcc.modelView()["ranges"])
    else:       # O1Dn with NaN directions, the dataset without a mask: NaN points fall to the gate's own comparison
        dirs = syn.model_directions(model).copy()
        dirs[11::131] = np.nan
        orig = np.float32([0.01, -0.02, 0.03])
        rcc = ra.RCCHipO1Dn(hm)
        rcc.setTsb(T.identity())
        rcc.setModel(W, H, 0.1, 100.0, tuple(float(x) for x in orig), dirs)
        rcc.set_traversal(kind)
        rcc.find(truth)
        mv = rcc.modelView()
        pts = (dirs * mv["ranges"].reshape(-1, 1) + orig).astype(np.float32)
        pts[mv["hits"].reshape(-1) == 0] = np.nan
        rcc.set_dataset(pts, None)
    assert rcc.find_variant(1) == kind, (rcc.find_variant(1), kind)
    return rcc


def prove_one(mode, n_iter, before, after, fallback=0):
    """the form one rmclhip_rcc_correct_once ended in, from the operator's fast_info before and after it"""
    d = {k: after[k] - before[k] for k in KEYS}
    tag = (mode, n_iter, fallback, d, after)
    if mode == 0 or n_iter < 2:             # the moment forms were not tried
        assert d["attempts"] == 0, tag
    elif fallback:                          # a moment form gave up, the per-iteration form served the call
        assert d["attempts"] == 1 and d["done"] == 0 and d["host_loops"] == 0 and after["last_code"] == fallback, tag
        assert d["cap_exits" if fallback == 1 else "overflows"] == 1, tag
    elif mode == 1:                         # moments published, the iterations on the host
        assert d["attempts"] == 1 and d["done"] == 1 and d["host_loops"] == 1 and after["last_code"] == 0, tag
    else:                                   # modes 3 and 4: the device loop
        assert d["attempts"] == 1 and d["done"] == 1 and d["host_loops"] == 0 and after["last_code"] == 0, tag


def digest_one(rcc, Tc, st):
    tot, rows, _ = rcc.debug_micp_moments()
    info = rcc.micp_fast_info()
    return {"transform": sha(Tc.tobytes()), "statistics": sha(st.tobytes()), "moments": sha(tot.tobytes()), "rows": int(rows),
            "last_code": int(info["last_code"]), "last_uncertain": int(info["last_uncertain"])}


def _scan(mesh, H, W, kind, mode, n_iter=N_ITER, sensor="spherical", rows=None, undecided=None):
    def run(ra, ctx):
        from rmcl_amd import types as T
        rcc = operator(ra, hip_map(ra, ctx, mesh), H, W, kind, sensor)
        est = T.mult(T.transform_from_rpy(*TRUTH), T.transform_from_rpy(*PERT))
        rcc.params.max_dist, rcc.adaptive_max_dist_min = 0.5, 0.2
        rcc.set_micp_fast(3)
        for _ in range(3):
            rcc.correct_once(est, T.identity(), N_ITER, 0.0, False)      # the caps are learnt with the separate pass
        rcc.set_micp_fast(mode)
        before = rcc.micp_fast_info()
        Tc, st = rcc.correct_once(est, T.identity(), n_iter, 0.0, False)
        prove_one(mode, n_iter, before, rcc.micp_fast_info())
        out = digest_one(rcc, Tc, st)
        if rows is not None and mode != 0:
            assert out["rows"] == rows, (out["rows"], rows)
        if undecided is not None and mode != 0:
            assert (out["last_uncertain"] > 0) == undecided, out
        rcc.close()
        return out
    return run


def _fallback(code):
    def run(ra, ctx):
        from rmcl_amd import types as T
        rcc = operator(ra, hip_map(ra, ctx, "room30k"), 64, 512, 23)
        est = T.mult(T.transform_from_rpy(*TRUTH), T.transform_from_rpy(*(FAR_PERT if code == 1 else PERT)))
        rcc.params.max_dist = rcc.adaptive_max_dist_min = 1.0 if code == 1 else 0.05
        rcc.set_micp_fast(4)
        before = rcc.micp_fast_info()
        Tc, st = rcc.correct_once(est, T.identity(), N_ITER, 0.0, False)
        prove_one(4, N_ITER, before, rcc.micp_fast_info(), fallback=code)
        out = digest_one(rcc, Tc, st)
        assert code == 1 or out["last_uncertain"] > 4096, out
        rcc.close()
        return out
    return run


def _rig(name, form):
    """form: per-iteration / host / device as tests/test_gpu_micp_multi.py runs and proves them; handover (mid); overflow (far)"""
    def run(ra, ctx):
        import micp_multi_cases as mc
        import test_gpu_micp_multi as tm
        case = mc.cases()[name]
        plain = mc.make_operator

        def pinned(ra_, hm_, s):
            rcc = plain(ra_, hm_, s)
            rcc.set_traversal(2)
            return rcc
        mc.make_operator = pinned
        try:
            loc = mc.make_localization(ra, hip_map(ra, ctx, case.mesh_name), case, {"handover": 1, "overflow": 1}.get(form) or tm.FORM_MODE[form])
        finally:
            mc.make_operator = plain
        assert all(s.correspondences_.find_variant(1) == 2 for s in loc.sensors_vec_)
        if form in ("host", "device", "handover"):
            for _ in range(2):
                mc.call(loc, case)
        Tc, merged, after = tm.proven_call(loc, case, {"handover": "device"}.get(form, form))
        if form == "handover":
            assert all(1024 < a["last_uncertain"] <= 4096 for a in after), after
        mc.close(loc)
        return {"transform": sha(Tc.tobytes()), "statistics": sha(merged.tobytes()), "last_code": int(after[0]["last_code"]),
                "last_uncertain": int(after[0]["last_uncertain"])}
    return run


def _statistics_p2l(ra, ctx):
    from rmcl_amd import synthetic as syn, types as T
    rcc = operator(ra, hip_map(ra, ctx, "room30k"), 64, 512, 23)
    rcc.find(T.mult(T.transform_from_rpy(*TRUTH), T.transform_from_rpy(*PERT)))
    mv = rcc.modelView()
    n = 64 * 512
    truth_ranges = operator(ra, hip_map(ra, ctx, "room30k"), 64, 512, 23)
    ranges = truth_ranges.modelView()["ranges"].reshape(-1, 1)
    D = (syn.model_directions(scaled_model(64, 512)) * ranges).astype(np.float32)
    up = lambda a: ra.DeviceArray.from_host(ctx, np.ascontiguousarray(a))
    hits = mv["hits"].reshape(-1).astype(np.uint8)
    st = ra.statistics_p2l(ctx, T.transform_from_rpy((0.01, -0.02, 0.005), (0.001, 0.002, -0.003)), up(D), up(hits),
                           up(mv["points"].reshape(-1, 3)), up(mv["normals"].reshape(-1, 3)), up(hits), n, 0.5)
    assert int(st["n_meas"]) > 1000
    rcc.close()
    truth_ranges.close()
    return {"statistics": sha(st.tobytes()), "n_meas": int(st["n_meas"])}


def _batch_4(ra, ctx):
    from rmcl_amd import types as T
    rcc = operator(ra, hip_map(ra, ctx, "room30k"), 64, 512, 23)
    rcc.params.max_dist, rcc.adaptive_max_dist_min = 0.5, 0.2
    truth = T.transform_from_rpy(*TRUTH)
    perts = [PERT, ((-0.02, 0.03, 0.0), (0.0, 0.002, -0.006)), ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)), ((0.05, 0.04, -0.02), (-0.003, 0.0, 0.01))]
    Tbm = np.array([T.mult(truth, T.transform_from_rpy(*p)) for p in perts])
    out, st = rcc.correct_batch(Tbm)
    assert all(int(s["n_meas"]) > 1000 for s in st)
    rcc.close()
    return {"transforms": sha(out.tobytes()), "statistics": sha(st.tobytes())}


def cases():
    c = {}
    for n_iter in (0, 1, 8):
        c["iter_64x512_n%d" % n_iter] = _scan("room30k", 64, 512, 23, 0, n_iter=n_iter)
    c["iter_64x512_o1dn_unmasked"] = _scan("room30k", 64, 512, 23, 0, sensor="o1dn")
    c["m3_64x512_room"] = _scan("room30k", 64, 512, 23, 3, rows=128, undecided=True)
    c["m3_30x500_room"] = _scan("room30k", 30, 500, 2, 3, rows=59, undecided=True)
    c["m3_64x512_cube_lone_wave"] = _scan("cube", 64, 512, 23, 3, rows=128, undecided=False)
    for mode in (4, 1):
        c["m%d_k23_64x512" % mode] = _scan("room30k", 64, 512, 23, mode, rows=128, undecided=True)
        c["m%d_k23_100x1000" % mode] = _scan("room30k", 100, 1000, 23, mode, rows=400, undecided=True)
        c["m%d_k2_30x500" % mode] = _scan("room30k", 30, 500, 2, mode, rows=256, undecided=True)
        c["m%d_k32_100x1000" % mode] = _scan("room30k", 100, 1000, 32, mode, rows=400, undecided=True)
    c["m1_k24_30x500_separate_pass"] = _scan("room30k", 30, 500, 24, 1, rows=59, undecided=True)
    c["fallback_cap_exit"] = _fallback(1)
    c["fallback_overflow"] = _fallback(2)
    for name in ("mixed4", "eight", "cube6", "near"):
        for form in ("per-iteration", "host", "device"):
            c["rig_%s_%s" % (name, form)] = _rig(name, form)
    c["rig_mid_handover"] = _rig("mid", "handover")
    c["rig_far_overflow"] = _rig("far", "overflow")
    c["statistics_p2l_64x512"] = _statistics_p2l
    c["batch_4_poses"] = _batch_4
    return c


if __name__ == "__main__":
    import rmcl_amd as ra
    ctx = ra.Context(0)
    out, failed = {}, []
    for name, fn in cases().items():
        try:
            out[name] = fn(ra, ctx)
        except AssertionError as e:      # reported together: a case in the wrong form is replaced, never recorded
            failed.append(name)
            print("FAILED %s: %r" % (name, e))
    path = sys.argv[1] if len(sys.argv) > 1 else OUT
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote %s: %d cases" % (path, len(out)))
    sys.exit(1 if failed else 0)
