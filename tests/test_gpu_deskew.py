"""GPU tests of the motion-compensated PointCloud2 input (rmclhip_rcc_set_input_pointcloud2_deskewed, rmclhip_pointcloud2_deskew;
kernel: rmcl_amd/csrc/deskew.hip) against the numpy restatement tests/deskew_ref.py: origins, directions, points, mask and the five
counters byte for byte; identity knots against rmclhip_rcc_set_input_pointcloud2; the operator's state against set_model_ondn +
set_dataset; the cloud form as the input of the spherical path and of closest-point correspondences; the premise of
tests/test_deskew_cpu.py through correct_once; every refusal.  Shapes are the smallest that reach every path: one point, one wave
minus / plus one, more than one workgroup (256 lanes), 2 / 3 / 64 knots.  A few seconds in all."""
import ctypes as C

import numpy as np
import pytest

import deskew_ref as dr

pytestmark = pytest.mark.gpu
F = np.float32
STATS = ("n_points", "n_finite", "n_valid", "n_time_clamped", "n_time_nonfinite")
LAYOUT_ARGS = ("width", "height", "point_step", "row_step", "offset_x", "offset_y", "offset_z")


def _knots(K, seed):
    """K knots at times k / 64 (exact in float32 and as 16 k ticks of 1 / 1024 s): a smooth turn about a tilted axis and a drift;
    for K >= 3 the second knot is stored as -q (the same rotation: the shortest-arc flip), the last knot is the identity"""
    rng = np.random.RandomState(seed)
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    u = (np.arange(K) - (K - 1)) / max(K - 1, 1)              # -1 .. 0: the reference time is the last knot
    ang = 0.3 * u
    q = np.c_[axis[None, :] * np.sin(ang / 2)[:, None], np.cos(ang / 2)]
    t = np.c_[0.5 * u, 0.2 * u * u, -0.1 * u]
    if K >= 3:
        q[1] = -q[1]
    return q.astype(F), t.astype(F), np.arange(K, dtype=np.float64) / 64.0


def _motion(ra, kq, kt, ktimes):
    knots = np.zeros(len(kq), ra.types.TRANSFORM)
    for i in range(len(kq)):
        knots[i] = ra.types.transform(tuple(float(x) for x in kq[i]), tuple(float(x) for x in kt[i]))
    return knots, np.asarray(ktimes, np.float64)


def _points_and_times(n, K, seed, time_dtype, nan_time=True, shrink=1.0):
    """n points with every edge the rules name (as many as n allows): times exactly on knots, before the first and after the last
    knot, NaN and inf coordinates, a NaN time, a point beyond range.max and one inside range.min.  Returns (xyz, raw time, scale)."""
    rng = np.random.RandomState(seed)
    p = rng.uniform(-9, 9, (n, 3)).astype(F)
    t_end = (K - 1) / 64.0
    ticks = rng.randint(0, int(1024 * t_end) + 1, n).astype(np.float64)        # 1 / 1024 s ticks: exact in every time datatype
    frac = rng.uniform(0, 1, n) if time_dtype != dr.UINT32 else np.zeros(n)
    t = np.minimum(ticks + frac, 1024 * t_end)
    edge = iter(rng.permutation(n))
    take = lambda: next(edge, None)
    for k in (0, K // 2, K - 1):
        i = take()
        if i is not None:
            t[i] = 16.0 * k                                                       # on a knot
    i = take()
    if i is not None:
        t[i] = 1024 * t_end + 40.0                                               # after the last knot
    if time_dtype != dr.UINT32:
        for val in (-3.0, np.nan) if nan_time else (-3.0,):                      # before the first knot; no time
            i = take()
            if i is not None:
                t[i] = val
    for col, val in ((0, np.nan), (1, np.inf), (2, -np.inf)):
        i = take()
        if i is not None:
            p[i, col] = val
    i = take()
    if i is not None:
        p[i] = (300.0, 0.0, 1.0)
    i = take()
    if i is not None:
        p[i] = (0.01, 0.02, 0.0)
    return p * F(shrink), t, 1.0 / 1024.0


RECORDS = {
    "v22": dict(gap=6),                                     # x y z intensity ring time: 22 bytes, every second record unaligned
    "f64": dict(xyz_dtype=dr.FLOAT64, lead=3),              # FLOAT64 coordinates at offset 3
    "wide": dict(point_step=40, lead=8),                    # a 40-byte record with other fields around
}


def _case(n, K, time_dtype, record, seed, width=None, **kw):
    kq, kt, ktimes = _knots(K, seed)
    p, t, scale = _points_and_times(n, K, seed, time_dtype, **kw)
    buf, lay, tf = dr.make_cloud(p, t, time_dtype, width=width, **RECORDS[record])
    return buf, lay, tf + (scale, 0.0), (kq, kt, ktimes)


def _assert_operator_equals_restatement(rcc, got, ref):
    w, h, stats = got
    assert (w, h) == (ref["width"], ref["height"])
    assert [stats[k] for k in STATS] == [ref["stats"][k] for k in STATS], (stats, ref["stats"])
    iv = rcc.inputView()
    for k in ("origs", "dirs", "points", "mask"):
        assert iv[k].tobytes() == ref[k].tobytes(), k


@pytest.fixture(scope="module")
def hm(ra, ctx, meshes):
    return ra.import_hip_map(ctx, *meshes("cube"))


@pytest.fixture(scope="module")
def rcc(ra, hm):
    return ra.RCCHipOnDn(hm)


CASES = [(n, K, (dr.UINT32, dr.FLOAT32, dr.FLOAT64)[(i + j) % 3], ("v22", "f64", "wide")[(i + 2 * j) % 3], (i + j) % 2 == 1)
         for i, n in enumerate((1, 63, 64, 65, 257, 1025)) for j, K in enumerate((2, 3, 64))]


@pytest.mark.parametrize("n,K,time_dtype,record,device", CASES)
def test_operator_form_equals_the_restatement(ra, ctx, rcc, n, K, time_dtype, record, device):
    """origins, directions, points, mask and the five counters, byte for byte; the same operator takes every case in turn (its
    buffers grow and are reused)"""
    buf, lay, tf, (kq, kt, ktimes) = _case(n, K, time_dtype, record, 1000 * n + K)
    ref = dr.deskew(buf, lay, tf, kq, kt, ktimes, 0.5, 100.0)
    if n >= 63:
        assert ref["stats"]["n_time_clamped"] >= 1 and ref["stats"]["n_finite"] == n - 3 and 0 < ref["stats"]["n_valid"] < n
        assert (ref["stats"]["n_time_nonfinite"] == 1) == (time_dtype != dr.UINT32)
    data = ra.DeviceArray.from_host(ctx, buf) if device else buf
    got = rcc.setInputPointCloud2Deskewed(data, *[lay[k] for k in LAYOUT_ARGS], tf, _motion(ra, kq, kt, ktimes), datatype=lay["datatype"],
                                          range_min=0.5, range_max=100.0, device=device, nbytes=len(buf))
    _assert_operator_equals_restatement(rcc, got, ref)


@pytest.mark.parametrize("shape,fh,fw", [((9, 37), (1, 2, 2), (3, 1, 3)), ((12, 131), (0, 1, 1), (2, 0, 2))])
def test_row_padding_and_both_filters(ra, ctx, rcc, shape, fh, fw):
    """an organised cloud with 7 bytes of padding behind every row, rows and columns picked by both filters: 3 x 11 and 11 x 64
    output points, indexed as rmclhip_rcc_set_input_pointcloud2 indexes them"""
    H, W = shape
    kq, kt, ktimes = _knots(5, 3)
    p, t, scale = _points_and_times(H * W, 5, 11, dr.FLOAT32)
    buf, lay, tf = dr.make_cloud(p, t, dr.FLOAT32, point_step=19, lead=1, row_pad=7, width=W)
    tf = tf + (scale, 0.0)
    ref = dr.deskew(buf, lay, tf, kq, kt, ktimes, 0.5, 100.0, fh, fw)
    assert ref["width"] * ref["height"] in (33, 704)
    for device in (False, True):
        data = ra.DeviceArray.from_host(ctx, buf) if device else buf
        got = rcc.setInputPointCloud2Deskewed(data, *[lay[k] for k in LAYOUT_ARGS], tf, _motion(ra, kq, kt, ktimes), range_min=0.5,
                                              range_max=100.0, filter_height=fh, filter_width=fw, device=device, nbytes=len(buf))
        _assert_operator_equals_restatement(rcc, got, ref)


def test_time_scale_and_offset_in_double(ra, rcc):
    """Ouster's t: UINT32 nanoseconds since the start of the scan, knots at epoch seconds -- t = offset_s + 1e-9 * raw in double
    (a float would hold 1.7e9 s to 128 s)"""
    rng = np.random.RandomState(4)
    n = 200
    p = rng.uniform(-9, 9, (n, 3)).astype(F)
    raw = rng.randint(0, 100_000_000, n).astype(np.float64)
    kq, kt, _ = _knots(9, 4)
    ktimes = 1.7e9 + np.arange(9) * 0.0125
    buf, lay, tf = dr.make_cloud(p, raw, dr.UINT32)
    tf = tf + (1e-9, 1.7e9)
    ref = dr.deskew(buf, lay, tf, kq, kt, ktimes, 0.5, 100.0)
    assert ref["stats"]["n_time_clamped"] == 0 and len(np.unique(ref["origs"], axis=0)) > 150
    got = rcc.setInputPointCloud2Deskewed(buf, *[lay[k] for k in LAYOUT_ARGS], tf, _motion(ra, kq, kt, ktimes), range_min=0.5, range_max=100.0)
    _assert_operator_equals_restatement(rcc, got, ref)


def test_identity_knots_equal_the_plain_pointcloud2_input(ra, hm, rcc):
    """with identity knots every array is, bit for bit, what rmclhip_rcc_set_input_pointcloud2 writes for the same bytes; origins 0"""
    plain = ra.RCCHipO1Dn(hm)
    ident = (np.array([ra.types.identity()] * 3, ra.types.TRANSFORM), [0.0, 0.4, 1.0])
    for record, n, width in (("v22", 1025, 1025), ("f64", 320, 64)):
        buf, lay, tf, _ = _case(n, 64, dr.FLOAT32, record, 77, width=width, nan_time=False)
        fh, fw = (None, None) if width == n else ((1, 0, 2), (0, 3, 1))
        args = [lay[k] for k in LAYOUT_ARGS]
        w0, h0, nv0 = plain.setInputPointCloud2(buf, *args, lay["datatype"], 0.5, 100.0, fh, fw)
        w1, h1, st = rcc.setInputPointCloud2Deskewed(buf, *args, tf, ident, datatype=lay["datatype"], range_min=0.5, range_max=100.0,
                                                     filter_height=fh, filter_width=fw)
        a, b = plain.inputView(), rcc.inputView()
        assert (w0, h0) == (w1, h1) and st["n_valid"] == nv0 and 0 < nv0 < w0 * h0
        assert st["n_time_nonfinite"] == 0 and (st["n_time_clamped"] >= 1 or width != n)   # (the filters may drop the early / late points)
        for k in ("dirs", "points", "mask"):
            assert b[k].tobytes() == a[k].tobytes(), k
        assert b["origs"].tobytes() == np.zeros((w1 * h1, 3), F).tobytes()


@pytest.mark.parametrize("kind", [2, 15, 23])
def test_operator_state_equals_set_model_ondn_plus_set_dataset(ra, orc, hm, kind):
    """after the call find() returns, byte for byte, what a second operator given set_model_ondn + set_dataset with the
    restatement's arrays returns; then a larger and a smaller cloud through the same operator"""
    from rmcl_amd import types as T
    est = T.transform_from_rpy((0.4, -0.2, 0.1), (0.01, -0.02, 0.3))
    a, b = ra.RCCHipOnDn(hm), ra.RCCHipOnDn(hm)
    for n in (257, 1025, 65):
        buf, lay, tf, (kq, kt, ktimes) = _case(n, 3, dr.FLOAT32, "v22", 5 * n, shrink=0.3)   # inside the 10 m room: the rays hit
        ref = dr.deskew(buf, lay, tf, kq, kt, ktimes, 0.1, 100.0)
        a.setInputPointCloud2Deskewed(buf, *[lay[k] for k in LAYOUT_ARGS], tf, _motion(ra, kq, kt, ktimes), range_min=0.1, range_max=100.0)
        b.setModel(n, 1, 0.1, 100.0, ref["origs"], ref["dirs"])
        b.set_dataset(ref["points"], ref["mask"])
        outs = []
        for r in (a, b):
            r.set_traversal(kind)
            r.params.max_dist = 20.0      # the points are scattered inside the room, metres off its walls
            r.find(est)
            outs.append((r.modelView(), r.computeCrossStatistics(T.identity())))
        for k in ("hits", "face_ids", "ranges", "points", "normals"):
            assert outs[0][0][k].tobytes() == outs[1][0][k].tobytes(), (n, k)
        assert outs[0][1].tobytes() == outs[1][1].tobytes() and int(outs[0][1]["n_meas"]) > n // 2
        assert a.find_variant() == b.find_variant()


def test_cloud_form(ra, orc, ctx, hm, rcc):
    """records byte-equal to the operator form's points, NaN where masked; as the device input of the spherical path they equal the
    host-bytes path; through set_dataset_view + find_cpc they equal find_cpc on the restatement's points"""
    from rmcl_amd import synthetic as syn, types as T
    n = 1025
    buf, lay, tf, (kq, kt, ktimes) = _case(n, 64, dr.FLOAT64, "v22", 31)
    motion = _motion(ra, kq, kt, ktimes)
    ref = dr.deskew(buf, lay, tf, kq, kt, ktimes, 0.5, 100.0)
    for device in (False, True):
        data = ra.DeviceArray.from_host(ctx, buf) if device else buf
        d_cloud, stats = ra.wire.pointcloud2_deskew(ctx, data, *[lay[k] for k in LAYOUT_ARGS], tf, motion, range_min=0.5, range_max=100.0,
                                                    device=device, nbytes=len(buf))
        cloud = d_cloud.download().reshape(-1, 3)
        assert [stats[k] for k in STATS] == [ref["stats"][k] for k in STATS]
        assert cloud.tobytes() == ref["cloud"].tobytes()
    rcc.setInputPointCloud2Deskewed(buf, *[lay[k] for k in LAYOUT_ARGS], tf, motion, range_min=0.5, range_max=100.0)
    pts = rcc.inputView()["points"]
    valid = ref["mask"] != 0
    assert cloud[valid].tobytes() == pts[valid].tobytes() and np.isnan(cloud[~valid]).all() and 0 < valid.sum() < n
    # the spherical fast path: points moved, rays from the reference pose
    model = syn.model_c1()
    s_dev, s_host = ra.RCCHipSpherical(hm), ra.RCCHipSpherical(hm)
    s_dev.setModel(model)
    s_host.setModel(model)
    st_dev = s_dev.setInputPointCloud2(d_cloud, n, 1, 12, 12 * n, 0, 4, 8, flags=7, device=True, nbytes=12 * n)
    st_host = s_host.setInputPointCloud2(ref["cloud"].tobytes(), n, 1, 12, 12 * n, 0, 4, 8, flags=7)
    assert st_dev == st_host and st_dev["n_cells_filled"] > 100
    assert s_dev.rangesView().download().tobytes() == s_host.rangesView().download().tobytes()
    assert s_dev.inputView()["points"].tobytes() == s_host.inputView()["points"].tobytes()
    # closest-point correspondences need no rays: exact
    est = T.transform_from_rpy((0.3, 0.1, 0.0), (0.0, 0.0, 0.2))
    mask = ra.DeviceArray.from_host(ctx, ref["mask"])
    c_view, c_ref = ra.CPCHip(hm), ra.CPCHip(hm)
    _capi = ra._capi
    _capi.check(_capi.lib().rmclhip_rcc_set_dataset_view(c_view._h, C.c_void_p(d_cloud.ptr), C.c_void_p(mask.ptr), n))
    c_view._model_shape = (1, n)
    c_ref.set_dataset(ref["points"], ref["mask"])
    outs = []
    for c in (c_view, c_ref):
        c.params.max_dist = 2.0
        c.find(est)
        outs.append((c.modelView(), c.computeCrossStatistics(T.identity())))
    assert outs[0][1].tobytes() == outs[1][1].tobytes() and int(outs[0][1]["n_meas"]) > 100
    for k in ("hits", "face_ids", "ranges", "points", "normals"):
        assert outs[0][0][k][valid].tobytes() == outs[1][0][k][valid].tobytes(), k


def test_premise_end_to_end_on_the_device(ra, orc, ctx, hm, meshes):
    """tests/test_deskew_cpu.py's premise through correct_once, 40 re-finding iterations: the raw scan (rmclhip_rcc_set_input_pointcloud2)
    ends more than 0.1 m from the truth, the deskewed input within 1e-3 m and 1e-3 rad"""
    from rmcl_amd import types as T
    sc = dr.premise_scene(orc.Mesh(*meshes("cube")))
    lay, tf = sc["layout"], sc["time_field"]
    kq, kt, ktimes = sc["knots"]
    start = dr.premise_start(sc["truth"])
    args = [lay[k] for k in LAYOUT_ARGS]
    raw = ra.RCCHipO1Dn(hm)
    raw.setInputPointCloud2(sc["cloud"], *args, 7, 0.1, 100.0)
    desk = ra.RCCHipOnDn(hm)
    w, h, st = desk.setInputPointCloud2Deskewed(sc["cloud"], *args, tf, _motion(ra, kq, kt, ktimes), range_min=0.1, range_max=100.0)
    assert (w, h) == (sc["W"], sc["H"]) and st["n_valid"] == w * h and st["n_time_clamped"] == 0
    errs = []
    for r in (raw, desk):
        r.params.max_dist = 1.0
        r.adaptive_max_dist_min = 1.0
        T_onew_oold, _ = r.correct_once(start, T.identity(), dr.PREMISE_ITERATIONS, 0.0, True)
        errs.append(dr.pose_error(T.mult(start, T_onew_oold), sc["truth"]))
    print("raw %.4f m %.4f rad | deskewed %.2e m %.2e rad" % (errs[0] + errs[1]))
    assert errs[0][0] > 0.1
    assert errs[1][0] < 1e-3 and errs[1][1] < 1e-3


def test_refusals_leave_outputs_and_state_untouched(ra, ctx, hm):
    """every refusal of rmclhip.h: RMCLHIP_ERR_INVALID (UNSUPPORTED for the datatypes) before anything is launched -- out_width /
    out_height / stats keep their values, the operator keeps its model and dataset (find returns the same bytes) -- for the
    operator form and the cloud form; an empty cloud is no error"""
    from rmcl_amd import types as T
    _capi, L = ra._capi, ra._capi.lib()
    n = 130
    buf, lay, tf, (kq, kt, ktimes) = _case(n, 3, dr.FLOAT32, "v22", 9)
    knots, times = _motion(ra, kq, kt, ktimes)
    op = ra.RCCHipOnDn(hm)
    op.setInputPointCloud2Deskewed(buf, *[lay[k] for k in LAYOUT_ARGS], tf, (knots, times), range_min=0.5, range_max=100.0)
    est = T.transform_from_rpy((0.4, -0.2, 0.1), (0.0, 0.0, 0.3))
    op.find(est)
    before_in, before_out = op.inputView(), op.modelView()
    d_out = ra.DeviceArray.from_host(ctx, np.full(3 * n, 7.0, F))

    def call(data=buf, nbytes=None, layout=lay, time=tf, knots_=knots, times_=times, n_knots=None, fh=None, fw=None, null=()):
        Lc = _capi.PointCloud2Layout(*[int(layout[k]) for k in LAYOUT_ARGS], int(layout["datatype"]))
        tfc = _capi.PointCloud2Time(int(time[0]), int(time[1]), float(time[2]), float(time[3]))
        k_arr = np.ascontiguousarray(knots_, T.TRANSFORM)
        t_arr = np.ascontiguousarray(times_, np.float64)
        mo = _capi.ScanMotion(None if "knots" in null else k_arr.ctypes.data, None if "times" in null else t_arr.ctypes.data,
                              len(k_arr) if n_knots is None else n_knots)
        dp = None if "data" in null else data.ctypes.data_as(C.c_void_p)
        nb = len(data) if nbytes is None else nbytes
        ow, oh, st = C.c_uint32(777), C.c_uint32(778), _capi.DeskewStats(1, 2, 3, 4, 5)
        fhc = _capi.Filter1D(*fh) if fh else None
        fwc = _capi.Filter1D(*fw) if fw else None
        rc = L.rmclhip_rcc_set_input_pointcloud2_deskewed(
            op._h, dp, nb, None if "layout" in null else C.byref(Lc), None if "time" in null else C.byref(tfc),
            C.byref(fhc) if fhc else None, C.byref(fwc) if fwc else None, _capi.Interval(0.5, 100.0), 0,
            None if "motion" in null else C.byref(mo), C.byref(ow), C.byref(oh), C.byref(st))
        assert (ow.value, oh.value) == (777, 778) and [getattr(st, k) for k in STATS] == [1, 2, 3, 4, 5]
        st2 = _capi.DeskewStats(1, 2, 3, 4, 5)
        rc2 = rc
        if not fh and not fw:
            rc2 = L.rmclhip_pointcloud2_deskew(ctx.handle, dp, nb, None if "layout" in null else C.byref(Lc),
                                               None if "time" in null else C.byref(tfc), 0, None if "motion" in null else C.byref(mo),
                                               _capi.Interval(0.5, 100.0), C.c_void_p(d_out.ptr), C.byref(st2))
            assert [getattr(st2, k) for k in STATS] == [1, 2, 3, 4, 5]
        assert rc == rc2
        return rc

    def knots_with(i, field, sub, val):
        k = knots.copy()
        k[i][field][sub] = val
        return k

    many = np.array([T.identity()] * 65, T.TRANSFORM)
    invalid = [
        dict(null=("layout",)), dict(null=("time",)), dict(null=("motion",)), dict(null=("data",)), dict(null=("knots",)), dict(null=("times",)),
        dict(nbytes=len(buf) - 1),                                   # the last record's time field ends at the buffer's last byte
        dict(n_knots=1), dict(n_knots=0), dict(knots_=many, times_=np.arange(65.0)),
        dict(times_=[0.0, np.nan, 2.0]), dict(times_=[0.0, 1.0, 1.0]), dict(times_=[0.0, 2.0, 1.0]), dict(times_=[0.0, 1.0, np.inf]),
        dict(knots_=knots_with(1, "t", "y", np.nan)), dict(knots_=knots_with(2, "R", "w", np.inf)),
        dict(knots_=knots_with(0, "R", "w", 1.01)), dict(knots_=knots_with(0, "R", "w", 0.0)),
        dict(time=(tf[0], tf[1], np.nan, 0.0)), dict(time=(tf[0], tf[1], 1.0, np.inf)),
        dict(fh=(0, 0, 0)), dict(fw=(100, 100, 1)), dict(fh=(1, 1, 1)),
    ]
    for kw in invalid:
        assert call(**kw) == _capi.ERR_INVALID, kw
        assert L.rmclhip_last_error()
    assert call(time=(tf[0], 2, 1.0, 0.0)) == _capi.ERR_UNSUPPORTED          # an INT8 time field
    assert call(layout=dict(lay, datatype=5)) == _capi.ERR_UNSUPPORTED       # INT32 coordinates
    assert L.rmclhip_rcc_set_input_pointcloud2_deskewed(None, None, 0, None, None, None, None, _capi.Interval(0, 1), 0, None, None, None, None) == _capi.ERR_INVALID
    assert L.rmclhip_pointcloud2_deskew(None, None, 0, None, None, 0, None, _capi.Interval(0, 1), None, None) == _capi.ERR_INVALID
    # nothing was touched: the cloud-form output, the operator's inputs, and what find makes of them
    assert (d_out.download() == 7.0).all()
    after_in = op.inputView()
    for k in ("origs", "dirs", "points", "mask"):
        assert after_in[k].tobytes() == before_in[k].tobytes(), k
    op.find(est)
    after_out = op.modelView()
    for k in ("hits", "face_ids", "ranges", "points", "normals"):
        assert after_out[k].tobytes() == before_out[k].tobytes(), k
    # an empty cloud is no error and empties the operator
    w, h, st = op.setInputPointCloud2Deskewed(b"", 0, 1, 22, 0, 0, 4, 8, tf, (knots, times))
    assert (w, h) == (0, 1) and st == dict.fromkeys(STATS, 0)
    assert op.inputView()["points"].shape == (0, 3)
    d0, st0 = ra.wire.pointcloud2_deskew(ctx, b"", 0, 1, 22, 0, 0, 4, 8, tf, (knots, times))
    assert st0 == dict.fromkeys(STATS, 0)
