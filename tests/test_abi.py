"""CPU tests of the drop-in boundary: librmclhip.so loads, exports every symbol include/rmclhip.h declares,
fails loudly (no CPU fallback) without a device, and its host-side pieces (transform algebra, Umeyama,
BVH builder) agree with the oracle.  No compute entry point is called here.
"""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols(header="rmclhip.h"):
    with open(os.path.join(ROOT, "include", header)) as fh:
        src = fh.read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(rmclhip_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol(ra):
    names = _declared_symbols()
    assert len(names) >= 45
    L = C.CDLL(ra._capi.LIB_PATH)
    missing = [n for n in names if not hasattr(L, n)]
    assert not missing, missing
    # the public header carries no diagnostics, experiments or measurement loops (round 5: the timing entry points moved to rmclhip_bench.h)
    assert not [n for n in names if "debug" in n or "lab" in n or "_time_" in n or "kernel_ms" in n or "kernel_timing" in n]
    bench_names = _declared_symbols("rmclhip_bench.h")
    assert "rmclhip_rcc_time_find" in bench_names and "rmclhip_pf_time_update" in bench_names and "rmclhip_pf_time_update_unfused" in bench_names and len(bench_names) == 10
    assert not [n for n in bench_names if not hasattr(L, n)]
    # the experiments' header: its two instrumentation entry points are exported by the product library (they need the handle's
    # internals; they report UNSUPPORTED until librmclhip_lab.so is loaded), the rest by the experiments library itself
    lab_names = _declared_symbols("rmclhip_lab.h")
    assert "rmclhip_lab_version" in lab_names and "rmclhip_debug_wave_clock" in lab_names
    lab = C.CDLL(ra._capi.LAB_PATH)
    for n in lab_names:
        assert hasattr(lab if n == "rmclhip_lab_version" else L, n), n
    # and the Python binding covers exactly the three headers
    assert sorted(ra._capi.SIGNATURES) == sorted(set(names) | set(bench_names) | (set(lab_names) - {"rmclhip_lab_version"}))


def test_only_the_owners_allocate():
    """Device, pinned and host-mapped memory of the library is allocated and freed in ONE place, the owning buffer types of
    capi_internal.h (DevBuf, PinnedBuf, MappedBuf): no other source names HIP's allocation and free functions.  The exception is
    the pair of public functions of capi_map.cpp that hand memory to the caller, rmclhip_malloc and rmclhip_free."""
    import glob
    calls = re.compile(r"\b(hipMalloc|hipFree|hipHostMalloc|hipHostFree|hipHostGetDevicePointer)\b")
    csrc = os.path.join(ROOT, "rmcl_amd", "csrc")
    files = sorted(p for ext in ("*.cpp", "*.hip", "*.h") for p in glob.glob(os.path.join(csrc, ext)))
    assert len(files) > 60
    found = {}
    for path in files:
        with open(path) as fh:
            src = fh.read()
        name = os.path.basename(path)
        if name == "capi_map.cpp":
            # cut the bodies of the two exempt functions out: each runs from its signature to the closing brace in column 0
            for fn, call in (("rmclhip_malloc", "hipMalloc"), ("rmclhip_free", "hipFree")):
                m = re.search(r"^rmclhip_status %s\(.*?^}\n" % fn, src, flags=re.S | re.M)
                assert m and call in m.group(0), fn
                src = src[:m.start()] + src[m.end():]
        hits = sorted(set(calls.findall(src)))
        if hits:
            found[name] = hits
    assert sorted(found) == ["capi_internal.h"], found
    assert found["capi_internal.h"] == ["hipFree", "hipHostFree", "hipHostGetDevicePointer", "hipHostMalloc", "hipMalloc"]


def test_pod_layouts(ra):
    T = ra.types
    assert T.TRANSFORM.itemsize == 32 and T.TRANSFORM.fields["t"][1] == 16 and T.TRANSFORM.fields["stamp"][1] == 28
    assert T.CROSS_STATISTICS.itemsize == 64 and T.CROSS_STATISTICS.fields["n_meas"][1] == 60
    assert T.PARTICLE_ATTRIBUTES.itemsize == 36 and T.RANGE_MEASUREMENT.itemsize == 64
    assert C.sizeof(ra._capi.SphericalModel) == 32 and C.sizeof(ra._capi.PFParams) == 32


def test_no_device_is_a_loud_error_not_a_fallback(ra):
    """In a GPU-less container ctx_create must fail with RMCLHIP_ERR_NO_DEVICE (on a GPU box it succeeds);
    null handles are rejected with RMCLHIP_ERR_INVALID and a message."""
    L = ra._capi.lib()
    h = C.c_void_p()
    st = L.rmclhip_ctx_create(0, C.byref(h))
    if st != ra._capi.OK:
        assert st == ra._capi.ERR_NO_DEVICE
        assert b"no CPU fallback" in L.rmclhip_last_error()
        with pytest.raises(ra.NoDeviceError):
            ra.Context(0)
    else:
        L.rmclhip_ctx_destroy(h)
    out = C.c_void_p()
    assert L.rmclhip_rcc_create(None, None, C.byref(out)) == ra._capi.ERR_INVALID
    assert b"NO MAP" in L.rmclhip_last_error()
    assert L.rmclhip_pf_create(None, None, C.byref(out)) == ra._capi.ERR_INVALID
    assert L.rmclhip_rcc_find(None, None) == ra._capi.ERR_INVALID
    # round-2 entry points: null handles / arguments are rejected the same way
    info = ra._capi.MicpFastInfo()
    assert L.rmclhip_rcc_set_micp_fast(None, 1) == ra._capi.ERR_INVALID
    assert L.rmclhip_rcc_micp_fast_info(None, C.byref(info)) == ra._capi.ERR_INVALID
    assert L.rmclhip_micp_correct_once(None, 0, None, None, None, 1, 0.0, None, None) == ra._capi.ERR_INVALID
    assert L.rmclhip_comm_create(None, 0, C.byref(out)) == ra._capi.ERR_INVALID
    assert L.rmclhip_pf_update_sharded(None, None, 0, None) == ra._capi.ERR_INVALID
    # round-4 entry points
    ci = ra._capi.CcsInfo()
    assert L.rmclhip_rcc_ccs_info(None, C.byref(ci)) == ra._capi.ERR_INVALID
    assert L.rmclhip_rcc_set_cpc_grid(None, 1) == ra._capi.ERR_INVALID
    assert L.rmclhip_pf_set_mapping(None, 1, 16, None, 0) == ra._capi.ERR_INVALID
    ms = C.c_float(0)
    assert L.rmclhip_rcc_time_caller_loop(None, None, None, 5, 0.0, 1, None, None, C.byref(ms)) == ra._capi.ERR_INVALID
    assert L.rmclhip_rcc_sharded_create(None, 0, None, 0, None, 0, C.byref(out)) == ra._capi.ERR_INVALID
    assert L.rmclhip_rcc_sharded_correct_batch(None, None, 0, None, None) == ra._capi.ERR_INVALID
    assert L.rmclhip_rcc_sharded_size(None) == 0
    assert L.rmclhip_comm_create_loopback(None, 0, C.byref(out)) == ra._capi.ERR_INVALID
    if st != ra._capi.OK:   # no device: the multi-device constructors fail loudly too
        assert L.rmclhip_comm_create_loopback(None, 2, C.byref(out)) == ra._capi.ERR_NO_DEVICE
        one = (C.c_int * 1)(0)
        assert L.rmclhip_rcc_sharded_create(one, 1, None, 0, None, 0, C.byref(out)) == ra._capi.ERR_NO_DEVICE
    tr = ra.types.identity().reshape(1) if hasattr(ra.types.identity(), "reshape") else None
    cs = np.zeros(1, ra.types.CROSS_STATISTICS)
    assert L.rmclhip_host_moment_statistics(None, None, None, None, 3, 1.0, 1.0, 0.0, 0.0, None, 1.0, cs.ctypes.data, None, None) == ra._capi.ERR_INVALID
    # ... and an empty correspondence set is Identity statistics, covered
    Tid = np.ascontiguousarray(ra.types.identity(), dtype=ra.types.TRANSFORM).reshape(1)
    cov = C.c_int(0)
    assert L.rmclhip_host_moment_statistics(None, None, None, None, 0, 1.0, 1.0, 0.01, 0.01, Tid.ctypes.data, 1.0, cs.ctypes.data, None, C.byref(cov)) == ra._capi.OK
    assert cov.value == 1 and int(cs[0]["n_meas"]) == 0
    assert L.rmclhip_version().startswith(b"rmclhip")


def test_host_algebra_bit_exact_with_oracle(ra, orc):
    """rmclhip_transform_mult / _inv / cross_statistics_* are the same operation-order spec as the oracle."""
    T = ra.types
    rng = np.random.RandomState(0)
    for _ in range(30):
        qa, qb = rng.normal(size=4), rng.normal(size=4)
        A = T.transform(qa / np.linalg.norm(qa), rng.uniform(-5, 5, 3))
        B = T.transform(qb / np.linalg.norm(qb), rng.uniform(-5, 5, 3))
        assert T.mult(A, B).tobytes() == orc.tmult(A, B).tobytes()
        assert T.inv(A).tobytes() == orc.tinv(A).tobytes()
        s1, s2 = np.zeros((), T.CROSS_STATISTICS), np.zeros((), T.CROSS_STATISTICS)
        for s in (s1, s2):
            for k in "xyz":
                s["dataset_mean"][k], s["model_mean"][k] = rng.uniform(-3, 3, 2)
            s["covariance"] = rng.normal(size=9)
            s["n_meas"] = rng.randint(1, 1000)
        assert T.cross_statistics_merge(s1, s2).tobytes() == orc.cs_merge(s1, s2).tobytes()
        assert T.cross_statistics_transform(A, s1).tobytes() == orc.cs_transform(A, s1).tobytes()
        tu, to = T.umeyama_transform(s1), orc.umeyama(s1)
        assert np.allclose([tu["R"][k] for k in "xyzw"], [to["R"][k] for k in "xyzw"], atol=1e-6)
        assert np.allclose([tu["t"][k] for k in "xyz"], [to["t"][k] for k in "xyz"], atol=1e-5)
    ident = T.cross_statistics_merge(T.cross_statistics_identity(), T.cross_statistics_identity())
    assert int(ident["n_meas"]) == 0 and not np.isnan(ident["covariance"]).any()


@pytest.mark.parametrize("name", ["cube", "sphere20k", "room30k", "chain200", "chain2000", "nested200", "fan20k", "cadmix20k"])
def test_bvh_builder_invariants(ra, orc, meshes, name):
    """Host-only build (rmclhip_bvh_build_host): every record in exactly one leaf and every face in at least one (round 6: a face the
    builder's SPATIAL splits cut is referenced from several leaves, each with the box of its part there, through identical records),
    triangle records bit-equal to the oracle's, every child box contains its subtree (a cut face: the union of the leaf boxes that
    reference it covers the triangle -- sampled), BFS node order, stack bound respected, and the oracle's intersector walking THESE
    arrays reproduces brute force.  chain* / nested200 are meshes whose SAH tree is far deeper than the kernels' 64-entry stack (round 5:
    the builder bounds the stack by construction instead of refusing the mesh); fan20k / cadmix20k / sphere20k's polar slivers take
    spatial splits."""
    v, f = meshes(name)
    info, nodes, tris = ra.build_bvh_host(v, f)
    if name.startswith("chain"):
        assert info["height_fallbacks"] + info["guarded_nodes"] > 0, "this mesh was meant to exercise the stack bound"
    elif name in ("cube", "sphere20k", "room30k"):
        assert info["height_fallbacks"] == 0 and info["guarded_nodes"] == 0
    m = orc.Mesh(v, f)
    nf = len(f)
    nrec = info["n_tri_records"]
    assert info["n_faces"] == nf and nodes.shape == (info["n_nodes"], 32) and tris.shape == (nrec, 16) and nrec >= nf
    fid = tris[:, 15]
    refs_of = np.bincount(fid, minlength=nf)
    assert len(refs_of) == nf and refs_of.min() >= 1                   # every face is referenced, no record names a face that does not exist
    assert (nrec > nf) == (info["spatial_splits"] > 0)
    if name in ("cube", "room30k", "chain200", "chain2000", "nested200"):
        assert nrec == nf                                               # regular meshes / chains: the plain builder's tree
    if name in ("fan20k", "sphere20k"):
        assert info["spatial_splits"] > 0 and nrec <= 2 * nf            # the reference budget: at most alpha = 1 extra records per face
    assert np.array_equal(tris.view(np.float32)[:, :15].view(np.uint32), m.tri_records()[fid].view(np.uint32))
    fl = nodes.view(np.float32)
    leaf_seen = np.zeros(nrec, dtype=np.int32)
    cut_boxes = {}                                                      # face -> [(lo, hi)] of the leaf boxes that reference a cut face
    v0 = tris.view(np.float32)[:, 0:3]
    v1 = v0 - tris.view(np.float32)[:, 3:6]
    v2 = v0 + tris.view(np.float32)[:, 6:9]

    def subtree_bounds(ref, depth, stack, box=None):
        if ref & 0x80000000:
            first, cnt = ref & 0x0FFFFFFF, ((ref >> 28) & 7) + 1
            assert cnt <= 4
            leaf_seen[first:first + cnt] += 1
            whole = [r for r in range(first, first + cnt) if refs_of[fid[r]] == 1]
            for r in range(first, first + cnt):
                if refs_of[fid[r]] > 1:
                    cut_boxes.setdefault(int(fid[r]), []).append(box)
            if not whole:                       # only parts of cut faces: the stored box is all there is to say
                return box[0], box[1], depth, stack
            pts = np.concatenate([v0[whole], v1[whole], v2[whole]])
            lo_, hi_ = pts.min(0), pts.max(0)
            if len(whole) < cnt:
                lo_, hi_ = np.minimum(lo_, box[0]), np.maximum(hi_, box[1])
            return lo_, hi_, depth, stack
        assert ref < info["n_nodes"]
        lo, hi, dmax, smax = np.full(3, np.inf), np.full(3, -np.inf), depth, stack
        nk = int(nodes[ref, 28])
        assert 1 <= nk <= 4
        kids = list(range(nk))
        for c in range(nk, 4):   # unused slots: unreachable point box + harmless leaf reference
            assert fl[ref, c] == fl[ref, 4 + c] >= 1e30 and nodes[ref, 24 + c] == 0x80000000
        for c in kids:
            child = int(nodes[ref, 24 + c])
            if not child & 0x80000000:
                assert child > ref  # breadth-first order: children come later
            bmin = np.array([fl[ref, 0 + c], fl[ref, 8 + c], fl[ref, 16 + c]])
            bmax = np.array([fl[ref, 4 + c], fl[ref, 12 + c], fl[ref, 20 + c]])
            clo, chi, d, s = subtree_bounds(child, depth + 1, stack + len(kids) - 1, (bmin, bmax))
            assert np.all(bmin <= clo) and np.all(bmax >= chi)       # (padded) box contains the subtree
            lo, hi, dmax, smax = np.minimum(lo, clo), np.maximum(hi, chi), max(dmax, d), max(smax, s)
        return lo, hi, dmax, smax

    import sys
    sys.setrecursionlimit(10000)
    lo, hi, dmax, smax = subtree_bounds(0, 1, 0)
    assert np.all(leaf_seen == 1)
    # a cut face: every point of the triangle lies in a leaf box that references the face (random barycentric samples + the corners)
    rs = np.random.RandomState(7)
    for face in list(cut_boxes)[:400]:
        r = int(np.nonzero(fid == face)[0][0])
        assert len(cut_boxes[face]) == refs_of[face]
        w = np.concatenate([rs.dirichlet((1, 1, 1), 24), np.eye(3)])
        pts = w[:, :1] * v0[r].astype(np.float64) + w[:, 1:2] * v1[r].astype(np.float64) + w[:, 2:3] * v2[r].astype(np.float64)
        inside = np.zeros(len(pts), bool)
        for blo, bhi in cut_boxes[face]:
            inside |= np.all(pts >= blo - 1e-6, axis=1) & np.all(pts <= bhi + 1e-6, axis=1)
        assert inside.all(), "face %d: part of the triangle lies in none of the %d leaf boxes that reference it" % (face, len(cut_boxes[face]))
    assert smax + 1 <= info["stack_need"] <= 64
    # (a leaf that holds only parts of cut faces contributes its STORED, padded box: the scene's padding is 1e-4 of its extent)
    slack = (2e-4 * float(np.max(np.abs(np.array(info["bbox_max"]) - np.array(info["bbox_min"])) + np.abs(info["bbox_max"]))) + 1e-5) if nrec > nf else 1e-5
    assert np.allclose(lo, info["bbox_min"], atol=slack) and np.allclose(hi, info["bbox_max"], atol=slack)
    rng = np.random.RandomState(1)
    n_hit = 0
    for k in range(200):
        O = rng.uniform(-3, 3, 3).astype(np.float32)
        O[2] = abs(O[2]) + 0.1
        D = rng.normal(size=3).astype(np.float32)
        if name.startswith(("chain", "nested", "fan")) and k % 2:   # aim at a triangle: these meshes fill little of the view
            tri = rng.randint(nf)
            w = rng.dirichlet((1, 1, 1))
            D = (w[0] * v0[tri] + w[1] * v1[tri] + w[2] * v2[tri] - O).astype(np.float32)
        D /= np.linalg.norm(D)
        got = orc.trace_bvh4(nodes, tris, O, D, 0.0, 1e30)
        assert got == m.intersect(O, D, 0.0, 1e30)
        n_hit += bool(got[0])
    assert n_hit >= 20


def test_bvh_builder_is_independent_of_the_thread_count(ra, meshes):
    """the threaded build (bvh_build.cpp: large nodes with the passes spread over the threads, subtrees handed out whole, stable
    partitions) returns the same bytes for 1, 3 and the default number of threads -- checked in child processes, the thread count is
    read once per build from RMCLHIP_BUILD_THREADS"""
    import hashlib, os, subprocess, sys
    code = ("import sys, hashlib; sys.path.insert(0, %r); import rmcl_amd as ra; from rmcl_amd import synthetic as syn\n"
            "for v, f in (syn.uv_sphere(200000), syn.noisy_room(30000), syn.exp_chain(200, 1.5), syn.sliver_fan(6000), syn.cad_mix(20000)):\n"
            "    i, n, t = ra.build_bvh_host(v, f); ip, npf, q = ra.build_bvh_host_pf(v, f)\n"
            "    print(hashlib.sha256(n.tobytes() + t.tobytes() + npf.tobytes() + q.tobytes()).hexdigest())\n") % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for nt in ("1", "3", None):
        env = dict(os.environ)
        env.pop("RMCLHIP_BUILD_THREADS", None)
        if nt:
            env["RMCLHIP_BUILD_THREADS"] = nt
        outs.append(subprocess.check_output([sys.executable, "-c", code], env=env).decode().split())
    assert len(outs[0]) == 5 and outs[0] == outs[1] == outs[2]   # (the fan and the CAD mix take spatial splits: their reference budget is handed down the tree, not drawn from a shared counter)


@pytest.mark.parametrize("name", ["cube", "sphere20k", "room30k"])
def test_quantised_nodes_contain_the_full_precision_boxes(ra, meshes, name):
    """Node4Q twins (layout.h): same child references; the 8-bit boxes decode (origin + q * scale, fp32) to boxes
    that contain the padded Node4 boxes -- culling on them is conservative, so results cannot change --, and lose
    little (at most two grid steps per plane); unused slots are inverted."""
    v, f = meshes(name)
    info, nodes, _ = ra.build_bvh_host(v, f)
    q = ra.build_bvh_host_quantised(v, f, info["n_nodes"])
    fl, qf = nodes.view(np.float32), q.view(np.float32)
    assert np.array_equal(q[:, 12:16], nodes[:, 24:28])
    for a in range(3):
        origin, scale = qf[:, a], qf[:, 3 + a]
        assert np.all(scale > 0)
        for c in range(4):
            valid = nodes[:, 28] > c
            ql = ((q[:, 6 + 2 * a] >> (8 * c)) & 0xFF).astype(np.float32)
            qh = ((q[:, 7 + 2 * a] >> (8 * c)) & 0xFF).astype(np.float32)
            lo, hi = fl[:, 8 * a + c], fl[:, 8 * a + 4 + c]
            dlo, dhi = origin + ql * scale, origin + qh * scale
            assert np.all(dlo[valid] <= lo[valid]) and np.all(dhi[valid] >= hi[valid])
            assert np.all(lo[valid] - dlo[valid] <= 2.0001 * scale[valid]) and np.all(dhi[valid] - hi[valid] <= 2.0001 * scale[valid])
            assert np.all(ql[~valid] == 255) and np.all(qh[~valid] == 0)


def test_bvh_builder_rejects_bad_meshes(ra):
    L = ra._capi.lib()
    v = np.zeros((3, 3), np.float32)
    bad = np.array([[0, 1, 7]], np.uint32)
    with pytest.raises(ra.RmclHipError):
        ra.build_bvh_host(v, bad)
    v[0, 0] = np.nan
    with pytest.raises(ra.RmclHipError):
        ra.build_bvh_host(v, np.array([[0, 1, 2]], np.uint32))
    assert b"bvh_build_host" in L.rmclhip_last_error()


def test_tiny_meshes_build(ra, orc):
    """1 triangle and 5 triangles: the root is still an inner Node4."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.5], [2, 2, 2], [3, 1, 0]], np.float32)
    for f in (np.array([[0, 1, 2]], np.uint32), np.array([[0, 1, 2], [1, 3, 2], [2, 3, 4], [3, 5, 4], [0, 2, 4]], np.uint32)):
        info, nodes, tris = ra.build_bvh_host(v, f)
        assert info["n_nodes"] >= 1 and 1 <= nodes[0, 28] <= 4
        m = orc.Mesh(v, f)
        for O, D in (((0.2, 0.2, 3), (0, 0, -1)), ((0.7, 0.7, 3), (0, 0, -1)), ((5, 5, 5), (1, 0, 0))):
            assert orc.trace_bvh4(nodes, tris, O, D) == m.intersect(O, D)


def test_umeyama_special_cases_match_the_svd_definition(ra, orc):
    """rmclhip_umeyama_transform solves the rotation through Horn's quaternion eigenproblem (largest root of a
    quartic by Newton, eigenvector from the adjugate) and falls back to the Jacobi SVD for degenerate inputs; covariances
    of rank <= 1, where the SVD definition R = U diag(1, 1, det) V^T leaves a family of rotations, get the shortest one
    (tests/umeyama_cases.py: the cases and the float64 definition).  Half turns (w ~ 0), reflections (det < 0), planar and
    collinear point sets, rank one along every axis, noise-free data and tiny / huge scales must all agree -- with the
    definition and with the oracle."""
    import umeyama_cases as uc
    T = ra.types
    cases = uc.crafted_cases()
    assert len(cases) > 200 and sum(fam == "general" for fam, _, _ in cases) > 60
    for fam, name, s in cases:
        tu, to = T.umeyama_transform(s), orc.umeyama(s)
        uc.assert_matches_ref(tu, s, "%s/%s" % (fam, name))
        qu, qo = uc.quat_of(tu), uc.quat_of(to)
        assert min(np.abs(qu - qo).max(), np.abs(qu + qo).max()) < 2e-6, (fam, name, qu, qo)
        assert np.allclose(uc.trans_of(tu), uc.trans_of(to), atol=2e-5), (fam, name)
    z = T.umeyama_transform(uc.make_stats(np.zeros((3, 3))))                           # zero covariance: the identity rotation
    assert [float(z["R"][k]) for k in "xyzw"] == [0.0, 0.0, 0.0, 1.0]
