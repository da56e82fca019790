"""The distance field on the device (include/rmclhip.h, DISTANCE FIELD): node values against the oracle and against the exact
closest-point update, the lookup against its numpy restatement (tests/field_ref.py) bit for bit, the error bound, the sensor update
answered from the field, the switches, the ranking a global localisation relies on, the sharded filter and the C++ example."""
import math
import struct
import subprocess

import numpy as np
import pytest

import cpc_cases as cc
import field_ref as fr
from conftest import assert_close_rel

pytestmark = pytest.mark.gpu
F = np.float32

# map, cell, margin
NODE_CASES = {"cube": (0.25, 0.5), "room30k": (0.4, 0.0), "floor": (0.5, 0.0), "farcube": (0.5, 0.0)}


@pytest.fixture(scope="module")
def world(ra, orc, ctx):
    """per map, made once: (vertices, faces, oracle mesh, device map, field, info, downloaded lattice)"""
    cache = {}

    def get(name):
        if name not in cache:
            v, f = cc.build_map(name)
            hm = ra.import_hip_map(ctx, v, f)
            cell, margin = NODE_CASES[name]
            fd = ra.DistanceFieldHip(hm, cell=cell, margin=margin)
            cache[name] = (v, f, orc.Mesh(v, f), hm, fd, fd.info(), fd.download())
        return cache[name]

    yield get
    for w in cache.values():
        w[4].close()


def _updater(ra, hm, field=None, correspondence_type=1):
    from rmcl_amd import types as T
    upd = ra.PCDSensorUpdaterHip(hm)
    upd.config = T.pf_params(correspondence_type=correspondence_type)
    upd.init()
    if field is not None:
        upd.set_field(field)
    return upd


def _run(ra, ctx, upd, poses, attrs, beams, Tsb, want_errors=True):
    """one update on fresh device copies: (attrs, errors [n_particles, n_beams])"""
    upd.setInput(beams, Tsb)
    d_poses, d_attrs = ra.DeviceArray.from_host(ctx, poses), ra.DeviceArray.from_host(ctx, attrs)
    d_err = ra.DeviceArray(ctx, np.float32, len(poses) * len(beams)) if want_errors else None
    upd.set_error_output(d_err)
    upd.update(d_poses, d_attrs)
    upd.set_error_output(None)
    return d_attrs.download(), (d_err.download().reshape(len(poses), len(beams)) if want_errors else None)


# ---- 1. node values -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(NODE_CASES))
def test_node_values(ra, orc, ctx, world, name):
    from rmcl_amd import synthetic as syn, types as T
    v, f, m, hm, fd, info, lat = world(name)
    cell, margin = NODE_CASES[name]
    assert fr.same_layout(fr.layout(v.min(0), v.max(0), cell=cell, margin=margin), info)
    assert lat.shape == (info["n"][2], info["n"][1], info["n"][0]) and not np.isnan(lat).any()
    if name == "floor":
        assert info["n"][2] == 2
    ref = fr.oracle_lattice(m, info)
    print("%s: %d nodes, max |device - oracle| = %.3g" % (name, lat.size, np.abs(lat.astype(np.float64) - ref).max()))
    assert_close_rel(lat, ref, 1e-5, 1e-6, "node values " + name)
    # ... and byte-equal to what the exact correspondence_type 1 update reports for beams that end on the nodes
    pos = fr.node_positions(info).reshape(-1, 3)
    poses, attrs = syn.uniform_particles(1, seed=1)
    poses[0] = T.identity()
    upd = _updater(ra, hm)
    got = np.empty(len(pos), F)
    for lo in range(0, len(pos), 8192):
        chunk = pos[lo:lo + 8192]
        beams = np.zeros(len(chunk), T.RANGE_MEASUREMENT)
        beams["orig"]["x"], beams["orig"]["y"], beams["orig"]["z"] = chunk[:, 0], chunk[:, 1], chunk[:, 2]
        beams["dir"]["x"] = 1.0
        got[lo:lo + 8192] = _run(ra, ctx, upd, poses, attrs, beams, T.identity())[1][0]
    upd.close()
    assert got.tobytes() == lat.tobytes()
    # the lookup at node (0, 0, 0) is that node's value
    assert fd.query(pos[:1])[0] == lat.reshape(-1)[0]


# ---- 2. the lookup --------------------------------------------------------------------------------------------------------------------
def _lookup_points(info, n_total=2560):
    info = fr.info_f32(info)
    rng = np.random.RandomState(21)
    n, cell = info["n"], info["cell"]
    origin = np.array(info["origin"], F)
    top = np.array([info["origin"][k] + F(n[k] - 1) * cell for k in range(3)], F)      # the last node per axis, as the lattice places it
    centre, half = 0.5 * (origin.astype(np.float64) + top), 0.5 * (top.astype(np.float64) - origin)
    inside = lambda k: (centre + rng.uniform(-1, 1, (k, 3)) * half).astype(F)
    parts, kinds = [], []

    def add(kind, p):
        p = np.asarray(p, F).reshape(-1, 3)
        parts.append(p)
        kinds.extend([kind] * len(p))

    pos = fr.node_positions(info).reshape(-1, 3)
    add("node", pos[rng.permutation(len(pos))[:300]])
    for k in range(3):                                   # on the max faces: u = n - 1
        p = inside(40)
        p[:, k] = top[k]
        add("maxface", p)
    add("maxface", top[None])
    add("origin", origin[None])
    for k in range(3):
        p = inside(10)
        p[:, k] = origin[k]
        add("origin", p)
    for sx in (-1, 0, 1):                                # outside every face, edge and corner
        for sy in (-1, 0, 1):
            for sz in (-1, 0, 1):
                if (sx, sy, sz) == (0, 0, 0):
                    continue
                p = inside(10).astype(np.float64)
                for k, s in enumerate((sx, sy, sz)):
                    if s:
                        p[:, k] = centre[k] + s * (half[k] + rng.uniform(0.01, 3.0, 10) * max(half))
                add("outside%+d%+d%+d" % (sx, sy, sz), p)
    add("far", [[centre[0] + 1e6, centre[1], centre[2]], [centre[0], centre[1] - 1e6, centre[2] + 1e6]])
    add("special", [[np.nan, centre[1], centre[2]], [centre[0], np.nan, np.nan], [np.inf, centre[1], centre[2]], [centre[0], -np.inf, centre[2]],
                    [centre[0], centre[1], np.inf], [-np.inf, np.inf, np.nan], [1e38, centre[1], centre[2]], [centre[0], -1e38, centre[2]],
                    [1e38, 1e38, -1e38], [3.4028235e38, centre[1], centre[2]]])
    add("inside", inside(n_total - sum(len(p) for p in parts)))
    pts, kinds = np.concatenate(parts), np.array(kinds)
    order = rng.permutation(len(pts))
    return pts[order], kinds[order]


@pytest.mark.parametrize("name", ["cube", "farcube"])
def test_lookup_is_the_numpy_restatement_bit_for_bit(ra, world, name):
    v, f, m, hm, fd, info, lat = world(name)
    pts, kinds = _lookup_points(info)
    assert len(pts) == 2560 and len(set(kinds)) == 26 + 6
    ref = fr.lookup(info, lat, pts)
    assert np.isnan(ref[kinds == "special"]).sum() == 6 and np.isinf(ref[kinds == "special"]).sum() == 4
    assert not np.isnan(ref[kinds != "special"]).any() and np.all(ref[kinds == "far"] > 9e5)
    for n in (1, 63, 65, 257, 2560):
        got = fd.query(pts[:n])
        assert np.array_equal(np.isnan(got), np.isnan(ref[:n]))
        assert got.tobytes() == ref[:n].tobytes(), "n = %d: %d of %d differ" % (n, (got.view(np.uint32) != ref[:n].view(np.uint32)).sum(), n)
    # device memory in, device memory out: the same bytes
    d_pts = ra.DeviceArray.from_host(fd.ctx, pts)
    d_out = ra.DeviceArray(fd.ctx, np.float32, len(pts))
    fd.query(d_pts, out_dev=d_out, n=len(pts))
    assert d_out.download().tobytes() == ref.tobytes()


def test_query_edges(ra, world):
    import ctypes as C
    v, f, m, hm, fd, info, lat = world("cube")
    L, E = ra._capi.lib(), ra._capi.ERR_INVALID
    three = np.zeros(3, F)
    one = np.full(1, 7.0, F)
    assert L.rmclhip_field_query(fd.handle, None, 0, 0, None) == ra._capi.OK                        # n == 0: nothing is touched
    assert L.rmclhip_field_query(fd.handle, None, 1, 0, one.ctypes.data_as(C.c_void_p)) == E and one[0] == 7.0
    assert L.rmclhip_field_query(fd.handle, three.ctypes.data_as(C.c_void_p), 1, 0, None) == E
    small = np.zeros(3, F)
    assert L.rmclhip_field_download(fd.handle, small.ctypes.data_as(C.c_void_p), 3) == E            # capacity below n_nodes
    assert fd.query(np.zeros((0, 3), F)).shape == (0,)
    # a mesh without faces never becomes a map, so no field can be asked of one
    with pytest.raises(ra.RmclHipError):
        ra.import_hip_map(fd.ctx, v, np.zeros((0, 3), np.uint32))
    # refused before anything is launched: the map's accounted bytes do not move
    before = hm.info()["device_bytes"]
    for bad in (dict(cell=-1.0), dict(cell=float("nan")), dict(margin=-0.5), dict(margin=float("inf")), dict(cell=0.01, max_nodes=1000)):
        with pytest.raises(ra.RmclHipError) as e:
            ra.DistanceFieldHip(hm, **bad)
        assert e.value.status == E
    assert hm.info()["device_bytes"] == before
    # the field's bytes are accounted for with the map while it lives
    extra = ra.DistanceFieldHip(hm, cell=1.0)
    assert hm.info()["device_bytes"] == before + extra.info()["bytes"]
    extra.close()
    assert hm.info()["device_bytes"] == before


# ---- 3. the bound ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cube", "room30k"])
def test_bound_inside_the_lattice(ra, world, name):
    v, f, m, hm, fd, info, lat = world(name)
    rng = np.random.RandomState(31)
    lo = np.array(info["origin"], np.float64)
    hi = lo + (np.array(info["n"]) - 1) * float(info["cell"])
    pts = rng.uniform(lo + 1e-3, hi - 1e-3, (5000, 3)).astype(F)
    got = fd.query(pts).astype(np.float64)
    exact = fr.oracle_distances(m, pts).astype(np.float64)
    err = np.abs(got - exact)
    print("%s: max |query - oracle| = %.4g of the bound %.4g" % (name, err.max(), 0.8661 * info["cell"]))
    assert np.all(err <= 0.8661 * info["cell"] + 1e-5 * exact + 1e-6), err.max()


# ---- 4. the update --------------------------------------------------------------------------------------------------------------------
def _room_case(ra, m, n_particles, n_beams):
    from rmcl_amd import synthetic as syn, types as T
    truth = T.transform_from_rpy((1.0, -1.5, 1.2), (0.0, 0.0, 0.5))
    cloud = m.simulate_spherical(syn.model_c1(), T.identity(), truth, bvh=True)["points"]
    beams = ra.sample_beams(cloud, n_beams, seed=7)
    poses, attrs = syn.uniform_particles(n_particles, seed=6, bb_min=(-9, -9, 0.2, 0, 0, -math.pi), bb_max=(9, 9, 3.0, 0, 0, math.pi))
    return poses, attrs, beams, syn.tsb_offset()


@pytest.mark.parametrize("n_beams", [1, 9, 100, 257])
@pytest.mark.parametrize("n_particles", [1, 63, 65, 257, 500])
def test_update_from_the_field(ra, orc, ctx, world, n_particles, n_beams):
    from rmcl_amd import types as T
    v, f, m, hm, fd, info, lat = world("room30k")
    poses, attrs, beams, Tsb = _room_case(ra, m, n_particles, n_beams)
    upd = _updater(ra, hm, fd)
    a_gpu, e_gpu = _run(ra, ctx, upd, poses, attrs, beams, Tsb)
    upd.close()
    # the pose restatement of tests/surface_ref.py (the oracle's transform arithmetic) gives the device's end points to the bit, so
    # the errors are the numpy lookup's bytes
    e_ref = fr.lookup(info, lat, fr.end_points(poses, Tsb, beams).reshape(-1, 3)).reshape(n_particles, n_beams)
    assert_close_rel(e_gpu, e_ref, 1e-5, 1e-6, "field errors")
    assert e_gpu.tobytes() == e_ref.tobytes()
    p = T.pf_params(correspondence_type=1)
    mean, sigma, n_meas = fr.chain(attrs, e_gpu, p.dist_sigma, p.max_n_meas)
    assert np.array_equal(a_gpu["likelihood"]["n_meas"], n_meas) and np.all(n_meas == attrs["likelihood"]["n_meas"] + n_beams)
    assert_close_rel(a_gpu["likelihood"]["mean"], mean, 1e-5, 1e-12, "field mean")
    assert_close_rel(a_gpu["likelihood"]["sigma"], sigma, 1e-4, 1e-10, "field sigma")
    assert a_gpu["state_sigma"].tobytes() == attrs["state_sigma"].tobytes()


def test_update_nan_beam_repeat_and_mapping(ra, orc, ctx, world):
    from rmcl_amd import types as T
    v, f, m, hm, fd, info, lat = world("room30k")
    poses, attrs, beams, Tsb = _room_case(ra, m, 257, 100)
    upd, exact = _updater(ra, hm, fd), _updater(ra, hm)
    first = _run(ra, ctx, upd, poses, attrs, beams, Tsb)
    again = _run(ra, ctx, upd, poses, attrs, beams, Tsb)
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()       # the same call twice
    # a shuffled particle-minor order: the same attributes
    order = ra.DeviceArray.from_host(ctx, np.random.RandomState(5).permutation(257).astype(np.uint32))
    upd.set_mapping(1, 16, order)
    mapped = _run(ra, ctx, upd, poses, attrs, beams, Tsb)
    upd.set_mapping(0, 0, None)
    assert mapped[0].tobytes() == first[0].tobytes() and mapped[1].tobytes() == first[1].tobytes()
    # a beam with a NaN direction poisons exactly the particles it poisons in the exact mode
    bad = beams.copy()
    bad["dir"]["y"][37] = np.nan
    a_f, e_f = _run(ra, ctx, upd, poses, attrs, bad, Tsb)
    a_x, e_x = _run(ra, ctx, exact, poses, attrs, bad, Tsb)
    assert np.array_equal(np.isnan(e_f), np.isnan(e_x)) and np.isnan(e_f[:, 37]).all() and np.isnan(e_f).sum() == 257
    assert np.array_equal(np.isnan(a_f["likelihood"]["mean"]), np.isnan(a_x["likelihood"]["mean"])) and np.isnan(a_f["likelihood"]["mean"]).all()
    assert np.array_equal(a_f["likelihood"]["n_meas"], a_x["likelihood"]["n_meas"])
    # the two modes differ by the lookup's error, within its bound for the end points inside the lattice
    e_exact = _run(ra, ctx, exact, poses, attrs, beams, Tsb)[1]
    ends = fr.end_points(poses, Tsb, beams)
    lo = np.array(info["origin"], np.float64)
    hi = lo + (np.array(info["n"]) - 1) * float(info["cell"])
    inside = ((ends >= lo) & (ends <= hi)).all(axis=2)
    assert inside.mean() > 0.3
    assert np.all(np.abs(first[1].astype(np.float64) - e_exact)[inside] <= 0.8661 * info["cell"] + 1e-5 * e_exact[inside] + 1e-6)
    upd.close()
    exact.close()


# ---- 5. the switches ------------------------------------------------------------------------------------------------------------------
def test_switches(ra, orc, ctx, world):
    from rmcl_amd import types as T
    v, f, m, hm, fd, info, lat = world("room30k")
    poses, attrs, beams, Tsb = _room_case(ra, m, 65, 9)
    never = _updater(ra, hm)
    base = _run(ra, ctx, never, poses, attrs, beams, Tsb)
    upd = _updater(ra, hm, fd)
    on = _run(ra, ctx, upd, poses, attrs, beams, Tsb)
    assert on[1].tobytes() != base[1].tobytes()
    upd.set_field(None)                                    # off after on: the bytes of a handle that never had one
    off = _run(ra, ctx, upd, poses, attrs, beams, Tsb)
    assert off[0].tobytes() == base[0].tobytes() and off[1].tobytes() == base[1].tobytes()
    # every other mode is untouched by a field that was switched off, too
    for ct in (0, 2, 3):
        upd.config = T.pf_params(correspondence_type=ct)
        never.config = T.pf_params(correspondence_type=ct)
        assert _run(ra, ctx, upd, poses, attrs, beams, Tsb)[0].tobytes() == _run(ra, ctx, never, poses, attrs, beams, Tsb)[0].tobytes()
    # a field set with correspondence_type 0 is refused, and attrs are untouched
    upd.set_field(fd)
    upd.config = T.pf_params(correspondence_type=0)
    upd.setInput(beams, Tsb)
    d_poses, d_attrs = ra.DeviceArray.from_host(ctx, poses), ra.DeviceArray.from_host(ctx, attrs)
    for sync in (True, False):
        with pytest.raises(ra.RmclHipError) as e:
            upd.update(d_poses, d_attrs, sync=sync)
        assert e.value.status == ra._capi.ERR_INVALID
    upd.sync()
    assert d_attrs.download().tobytes() == attrs.tobytes()
    upd.config = T.pf_params(correspondence_type=1)
    assert _run(ra, ctx, upd, poses, attrs, beams, Tsb)[0].tobytes() == on[0].tobytes()
    # a field of another map is refused, and the handle keeps the one it has
    other = world("cube")[4]
    with pytest.raises(ra.RmclHipError) as e:
        upd.set_field(other)
    assert e.value.status == ra._capi.ERR_INVALID
    assert _run(ra, ctx, upd, poses, attrs, beams, Tsb)[0].tobytes() == on[0].tobytes()
    # the field outlives a close() of its Python object while an updater holds it
    own = ra.DistanceFieldHip(hm, cell=0.4)
    upd.set_field(own)
    own.close()
    assert _run(ra, ctx, upd, poses, attrs, beams, Tsb)[0].tobytes() == on[0].tobytes()
    upd.close()
    never.close()


# ---- 6. ranking -----------------------------------------------------------------------------------------------------------------------
def test_the_truth_ranks_first_in_both_modes(ra, orc, ctx, world):
    v, f, m, hm, _, _, _ = world("room30k")
    poses, attrs, beams, Tsb = fr.ranking_case(m)
    fine = ra.DistanceFieldHip(hm, cell=fr.RANKING_CELL)
    assert fine.info()["cell"] == F(0.1) and fine.info()["n_nodes"] > 2000000
    with_field, exact = _updater(ra, hm, fine), _updater(ra, hm)
    fine.close()
    mean_f = _run(ra, ctx, with_field, poses, attrs, beams, Tsb, want_errors=False)[0]["likelihood"]["mean"]
    mean_x = _run(ra, ctx, exact, poses, attrs, beams, Tsb, want_errors=False)[0]["likelihood"]["mean"]
    assert int(np.argmax(mean_f)) == fr.RANKING_TRUTH_INDEX == int(np.argmax(mean_x))
    assert not np.isnan(mean_f).any()
    with_field.close()
    exact.close()


# ---- 7. sharded -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ranks", [2, 3])
def test_sharded_update_equals_the_unsharded_one(ra, orc, ctx, world, ranks):
    from rmcl_amd import types as T
    v, f, m, hm, fd, info, lat = world("room30k")
    poses, attrs, beams, Tsb = _room_case(ra, m, 257, 9)          # 257 particles: a ragged split over 2 and over 3 ranks
    upd = _updater(ra, hm, fd)
    single = _run(ra, ctx, upd, poses, attrs, beams, Tsb, want_errors=False)[0]
    upd.close()
    spf = ra.ShardedParticleFilterHip(v, f, devices=(0,) * ranks, loopback=True)
    spf.config_ = T.pf_params(correspondence_type=1)
    spf.set_particles(poses, attrs)
    spf.update(beams, Tsb)
    exact = spf.download()[1]
    spf.set_particles(poses, attrs)
    spf.set_field(cell=NODE_CASES["room30k"][0], margin=NODE_CASES["room30k"][1])
    w = spf.update(beams, Tsb)
    got = spf.download()[1]
    assert got.tobytes() == single.tobytes() and got.tobytes() != exact.tobytes()
    assert w.tobytes() == single["likelihood"]["mean"].tobytes()
    spf.set_particles(poses, attrs)
    spf.set_field(None)                                          # off: the exact mode's bytes again
    spf.update(beams, Tsb)
    assert spf.download()[1].tobytes() == exact.tobytes()
    with pytest.raises(ra.RmclHipError):
        spf.set_field(cell=-1.0)
    spf.close()


# ---- 8. the example -------------------------------------------------------------------------------------------------------------------
def test_example_matches_the_python_binding(ra, orc, ctx, world, tmp_path):
    from rmcl_amd import types as T
    exe = fr.build_example(tmp_path)
    v, f, m, hm, fd, info, lat = world("room30k")
    poses, attrs, beams, _ = _room_case(ra, m, 65, 9)
    with open(tmp_path / "mesh.bin", "wb") as fh:
        fh.write(struct.pack("<II", len(v), len(f)))
        fh.write(np.ascontiguousarray(v, np.float32).tobytes())
        fh.write(np.ascontiguousarray(f, np.uint32).tobytes())
    with open(tmp_path / "particles.bin", "wb") as fh:
        fh.write(struct.pack("<I", len(poses)) + poses.tobytes() + attrs.tobytes())
    with open(tmp_path / "beams.bin", "wb") as fh:
        fh.write(struct.pack("<I", len(beams)) + beams.tobytes())
    cell, margin = NODE_CASES["room30k"]
    r = subprocess.run([exe, str(tmp_path / "mesh.bin"), str(tmp_path / "particles.bin"), str(tmp_path / "beams.bin"), repr(cell), repr(margin)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = {ln.split()[0]: ln.split()[1:] for ln in r.stdout.strip().splitlines()}
    assert tuple(int(x) for x in out["nodes"]) == info["n"]
    assert np.array([float(x) for x in out["origin"]], F).tobytes() == np.array(info["origin"], F).tobytes()
    assert np.array([float(x) for x in out["cell"]], F).tobytes() == np.array([info["cell"], info["inv_cell"]], F).tobytes()
    assert [int(x) for x in out["size"]] == [info["n_nodes"], info["bytes"]]
    where = np.array([[poses[i]["t"][k] for k in "xyz"] for i in range(3)], F)
    assert np.array([float(x) for x in out["query"]], F).tobytes() == fd.query(where).tobytes()
    upd = _updater(ra, hm, fd)
    a, e = _run(ra, ctx, upd, poses, attrs, beams, T.identity())
    upd.close()
    assert np.array([float(x) for x in out["errors"]], F).tobytes() == e.reshape(-1)[:3].tobytes()
    assert np.array([float(x) for x in out["means"]], F).tobytes() == a["likelihood"]["mean"][:3].tobytes()
