"""Every handle of the C ABI gives back what it took: the library's live-bytes counters (rmclhip_debug_live_bytes, include/rmclhip_lab.h)
-- device bytes, and pinned + host-mapped bytes -- are read, handles are made and every feature that allocates lazily is exercised,
everything is closed, and both counters must equal their first reading EXACTLY.  The shapes are tiny (the 972-triangle cube room, a
16 x 8 spherical model, two to four poses, 64 particles, 16 beams): a buffer is either freed or not, whatever its size.

Memory the caller owns (DeviceArray: rmclhip_malloc) is not counted.  The counters are process-wide, so every case first collects
Python's garbage: a handle an earlier test left to the collector must not go in the middle of the case."""
import contextlib
import ctypes as C
import gc
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_PARTICLES, N_BEAMS = 64, 16
BOX_LO, BOX_HI = (-4.0, -4.0, -3.0, 0.0, 0.0, -math.pi), (4.0, 4.0, 3.0, 0.0, 0.0, math.pi)


def _live(ra):
    dev, host = C.c_uint64(0), C.c_uint64(0)
    ra._capi.check(ra._capi.lib().rmclhip_debug_live_bytes(C.byref(dev), C.byref(host)))
    return dev.value, host.value


@contextlib.contextmanager
def _accounted(ra):
    """the case's own Context(0); on the way out the context is closed and both counters must be back at their first reading"""
    gc.collect()
    ctx = ra.Context(0)
    first = _live(ra)
    yield ctx
    ctx.close()
    last = _live(ra)
    assert last == first, "live (device, host) bytes %s before, %s after: %s bytes are still held" % (
        first, last, (last[0] - first[0], last[1] - first[1]))


def _model(ra):
    """16 columns x 8 rows, 30 degrees of elevation, the full circle"""
    f = np.float32
    return ra.types.spherical_model(f(-15.0 * math.pi / 180), f((30.0 * math.pi / 180) / 7), 8, f(-math.pi), f(2 * math.pi / 16), 16, f(0.1), f(100.0))


def _poses(ra):
    from rmcl_amd import synthetic as syn
    truth = syn.pose_c2_truth()
    est = ra.types.mult(truth, syn.pose_c2_perturbation())
    return truth, est


def _scan(ra, hm, model, Tsb, pose):
    """what the sensor measures at `pose`: (ranges [128], points in the sensor frame [128, 3])"""
    from rmcl_amd import synthetic as syn
    rcc = ra.RCCHipSpherical(hm)
    rcc.setTsb(Tsb)
    rcc.setModel(model)
    rcc.find(pose)
    ranges = rcc.modelView(("ranges",))["ranges"]
    rcc.close()
    assert np.isfinite(ranges).all() and (ranges > 0.1).all()        # a closed room: every ray hits
    return ranges, (syn.model_directions(model) * ranges[:, None]).astype(np.float32)


def _cloud_with_times(points):
    """PointCloud2 bytes of {x, y, z, t} float32 records (point_step 16), the layout arguments, the time field, an identity motion"""
    from rmcl_amd import types as T
    n = len(points)
    rec = np.zeros((n, 4), np.float32)
    rec[:, :3] = points
    rec[:, 3] = np.linspace(0.0, 1.0, n, dtype=np.float32)
    motion = (np.array([T.identity(), T.identity()], dtype=T.TRANSFORM), np.array([0.0, 1.0]))
    return rec.view(np.uint8).reshape(-1), (n, 1, 16, 16 * n, 0, 4, 8), (12, 7), motion


def _operator(ra, hm, model, Tsb, ranges):
    rcc = ra.RCCHipSpherical(hm)
    rcc.setTsb(Tsb)
    rcc.setModel(model)
    assert rcc.set_dataset_from_ranges(ranges) == len(ranges)
    rcc.params.max_dist = 1.0
    rcc.adaptive_max_dist_min = 0.15
    return rcc


def test_operator_gives_everything_back(ra, meshes):
    from rmcl_amd import synthetic as syn, types as T
    with _accounted(ra) as ctx:
        hm = ra.import_hip_map(ctx, *meshes("cube"))
        model, Tsb = _model(ra), syn.tsb_offset()
        truth, est = _poses(ra)
        ranges, points = _scan(ra, hm, model, Tsb, truth)
        rcc = _operator(ra, hm, model, Tsb, ranges)
        # model and dataset, find, the reduction, pose information
        rcc.find(est)
        assert int(rcc.computeCrossStatistics(T.identity())["n_meas"]) > 0
        assert int(rcc.computePoseInformation(T.identity())["n_meas"]) > 0
        # a pose batch that went in world order, its pose information, correct_batch
        batch = np.array([est, truth, est], dtype=T.TRANSFORM)
        rcc.find_batch(batch)
        keys, order, ngroups = rcc.debug_batch_order()
        assert ngroups > 0 and len(order) == len(batch) * ngroups, "the batch went pose-major: the case proves nothing"
        assert len(rcc.computePoseInformationBatch(len(batch))) == len(batch)
        Td, st = rcc.correct_batch(batch)
        assert (st["n_meas"] > 0).all()
        # correct_once: the per-iteration form replayed from its graph, then the moment forms (host iterations, the two device loops)
        for mode in (0, 1, 3, 4):
            rcc.set_micp_fast(mode)
            for _ in range(2):
                rcc.correct_once(est, T.identity(), 3)
        rcc.set_micp_fast(1)
        # the N-sensor correction over two sensors
        other = _operator(ra, hm, model, T.identity(), _scan(ra, hm, model, T.identity(), truth)[0])
        loc = ra.MICPLocalization([ra.MICPSensor("a", rcc, Tsb=Tsb), ra.MICPSensor("b", other, Tsb=T.identity())], optimization_iterations=3)
        loc.Tom_ = est
        for _ in range(2):
            loc.correctOnce(device_loop=True)
        other.close()
        # segmentation
        seg = rcc.segment(est, ranges)
        assert len(seg["labels"]) == len(ranges)
        # the PointCloud2 scan input
        stats = rcc.setInputPointCloud2(points.view(np.uint8).reshape(-1), len(points), 1, 12, 12 * len(points), 0, 4, 8)
        assert stats["n_points"] == len(points) and stats["n_cells_filled"] > 0
        rcc.find(est)
        rcc.close()
        # the deskewed input
        buf, layout, tf, motion = _cloud_with_times(points)
        desk = ra.RCCHipOnDn(hm)
        desk.setTsb(Tsb)
        w, h, dstats = desk.setInputPointCloud2Deskewed(buf, *layout, tf, motion, range_min=0.1, range_max=100.0)
        assert w * h == len(points) and dstats["n_valid"] > 0
        desk.find(est)
        desk.close()
        # closest-point correspondences: builds the map's near grid
        cpc = ra.CPCHip(hm)
        cpc.setTsb(Tsb)
        cpc.set_dataset(points)
        before_grid = hm.info()["device_bytes"]
        cpc.find(est)
        assert hm.info()["device_bytes"] > before_grid
        cpc.find(est)                                                   # (tracking: the records of the first call seed the second)
        cpc.close()
        hm.release()


@pytest.mark.lab
def test_debug_probes_give_everything_back(ra, meshes):
    from rmcl_amd import synthetic as syn
    with _accounted(ra) as ctx:
        hm = ra.import_hip_map(ctx, *meshes("cube"))
        model, Tsb = _model(ra), syn.tsb_offset()
        truth, est = _poses(ra)
        rcc = _operator(ra, hm, model, Tsb, _scan(ra, hm, model, Tsb, truth)[0])
        assert len(rcc.debug_probe_find(est)) > 0
        assert len(rcc.debug_wave_clock(est)) > 0
        rcc.close()
        hm.release()


def test_filter_side_gives_everything_back(ra, meshes):
    from rmcl_amd import synthetic as syn, types as T
    with _accounted(ra) as ctx:
        hm = ra.import_hip_map(ctx, *meshes("cube"))
        model, Tsb = _model(ra), syn.tsb_offset()
        truth, est = _poses(ra)
        ranges, points = _scan(ra, hm, model, Tsb, truth)
        beams = ra.sample_beams(points, N_BEAMS, seed=7)
        assert len(beams) == N_BEAMS
        poses, attrs = syn.uniform_particles(N_PARTICLES, seed=3, bb_min=BOX_LO, bb_max=BOX_HI)
        d_poses, d_attrs = ra.DeviceArray.from_host(ctx, poses), ra.DeviceArray.from_host(ctx, attrs)
        d_poses2, d_attrs2 = ra.DeviceArray.from_host(ctx, poses), ra.DeviceArray.from_host(ctx, attrs)
        # the sensor update by ray casting and by closest point (the full near grid), then from a dense and from a banded field
        upd = ra.PCDSensorUpdaterHip(hm)
        upd.init()
        upd.setInput(beams, Tsb)
        for ct in (0, 1):
            upd.config.correspondence_type = ct
            upd.update(d_poses, d_attrs)
        dense = ra.DistanceFieldHip(hm, cell=0.25)
        banded = ra.DistanceFieldHip.banded(hm, cell=0.25, band=0.5)
        for fd in (dense, banded):
            upd.set_field(fd)
            upd.update(d_poses, d_attrs)
        dense.close()                                                   # (the updater dropped it for the banded one)
        # refinement on the handle and on the field, a query, the Stein step with statistics and no result rows
        assert upd.refine(d_poses, iterations=2, max_dist=0.4)["n_particles"] == N_PARTICLES
        assert banded.refine(d_poses, beams, Tsb, iterations=2, max_dist=0.4)["n_particles"] == N_PARTICLES
        assert len(banded.query(points[:5])) == 5
        assert upd.stein_step(d_poses, iterations=1, max_dist=0.4)["n_particles"] == N_PARTICLES
        banded.close()                                                  # (the updater still holds it)
        upd.close()
        # the surface constraint with a motion update
        mot = ra.TFMotionUpdaterHip(hm)
        mot.surface = T.surface_params(height=0.2)
        mot.update(d_poses, d_attrs, N_PARTICLES, T.transform_from_rpy((0.1, 0.0, 0.0), (0.0, 0.0, 0.05)), 0.0)
        assert mot.surface_stats()["n_particles"] > 0
        mot.close()
        # the particle initialisations and the visualisation pack
        ra.init_particles_uniform(ctx, d_poses, d_attrs, BOX_LO, BOX_HI, seed=5)
        ra.init_particles_pose(ctx, d_poses, d_attrs, truth, np.diag([0.04] * 3 + [0.0, 0.0, 0.01]), seed=5)
        assert len(ra.pack_visualization(ctx, d_poses, d_attrs, N_PARTICLES)["x"]) == N_PARTICLES
        upd = ra.PCDSensorUpdaterHip(hm)                                # likelihoods for the resamplers
        upd.init()
        upd.setInput(beams, Tsb)
        upd.update(d_poses, d_attrs)
        upd.close()
        # the resamplers: tournament, residual, adaptive, systematic; the pose estimate and the hypotheses
        glad = ra.GladiatorResamplerHip(ctx)
        assert glad.compute_stats(d_attrs, N_PARTICLES)["sum"] > 0.0
        glad.update(d_poses, d_attrs, d_poses2, d_attrs2, N_PARTICLES)
        glad.close()
        res = ra.ResidualResamplerHip(ctx)
        res.update(d_poses, d_attrs, d_poses2, d_attrs2, N_PARTICLES)
        res.close()
        ada = ra.AdaptiveResamplerHip(ctx)
        ada.kld = T.kld_params(n_min=16)
        assert 16 <= ada.update(d_poses, d_attrs, d_poses2, d_attrs2, N_PARTICLES)["n_particles"] <= N_PARTICLES
        ada.update_systematic(d_poses, d_attrs, d_poses2, d_attrs2, N_PARTICLES)
        ada.close()
        pe = ra.PoseEstimatorHip(ctx)
        assert pe.estimate(d_poses, d_attrs, N_PARTICLES)["nparticles"] == N_PARTICLES
        assert pe.hypotheses(d_poses, d_attrs, N_PARTICLES)["n_clusters"] >= 1
        pe.close()
        # the surface sampler with an injection
        sm = ra.SurfaceSamplerHip(hm)
        assert sm.info()["n_eligible"] > 0
        sm.init(d_poses, d_attrs, seed=9)
        assert 0 < sm.inject(d_poses, d_attrs, 0.5, seed=9, step=0) < N_PARTICLES
        sm.close()
        # the context's free functions
        rcc = _operator(ra, hm, model, Tsb, ranges)
        rcc.find(est)
        mv = rcc.modelView()
        rcc.close()
        views = [ra.DeviceArray.from_host(ctx, a) for a in (points, mv["points"], mv["normals"], mv["hits"])]
        args = (ctx, T.identity(), views[0], None, views[1], views[2], views[3], len(points), 1.0)
        assert int(ra.statistics_p2l(*args)["n_meas"]) > 0
        assert int(ra.pose_information_p2l(*args)["n_meas"]) > 0
        image, pstats = ra.wire.pointcloud2_to_scan(ctx, points.view(np.uint8).reshape(-1), len(points), 1, 12, 12 * len(points), 0, 4, 8, model)
        assert pstats["n_cells_filled"] > 0
        buf, layout, tf, motion = _cloud_with_times(points)
        d_cloud, dstats = ra.wire.pointcloud2_deskew(ctx, buf, *layout, tf, motion, range_min=0.1, range_max=100.0)
        assert dstats["n_valid"] > 0
        for d in views + [d_cloud, d_poses, d_attrs, d_poses2, d_attrs2]:
            d.free()
        hm.release()


def test_sharded_handles_give_everything_back(ra, meshes):
    from rmcl_amd import synthetic as syn, types as T
    with _accounted(ra) as ctx:
        v, f = meshes("cube")
        hm = ra.import_hip_map(ctx, v, f)
        model, Tsb = _model(ra), syn.tsb_offset()
        truth, est = _poses(ra)
        ranges, points = _scan(ra, hm, model, Tsb, truth)
        hm.release()
        # a loopback communicator of two ranks: one step of the sharded filter with a resample
        pf = ra.ShardedParticleFilterHip(v, f, devices=(0, 0), loopback=True)
        pf.init_uniform(N_PARTICLES, BOX_LO, BOX_HI, seed=5)
        st = pf.step(ra.sample_beams(points, N_BEAMS, seed=7), Tsb, T_bnew_bold=T.transform_from_rpy((0.1, 0.0, 0.0), (0.0, 0.0, 0.05)),
                     resample="gladiator", seed=11, step=0)
        assert st["sum"] > 0.0 and len(pf.download()[0]) == N_PARTICLES
        pf.close()
        # pose batches sharded over two operator replicas
        sc = ra.ShardedCorrectorHip((0, 0), v, f)
        for rep in sc.replicas:
            rep.setTsb(Tsb)
            rep.setModel(model)
            rep.set_dataset_from_ranges(ranges)
        Td, stats = sc.correct_batch(np.array([est, truth, est, truth], dtype=T.TRANSFORM))
        assert (stats["n_meas"] > 0).all()
        sc.close()


def test_refused_creates_and_regrown_datasets_give_everything_back(ra, meshes):
    from rmcl_amd import synthetic as syn, types as T
    with _accounted(ra) as ctx:
        hm = ra.import_hip_map(ctx, *meshes("cube"))
        held = _live(ra)
        # a banded field refused AFTER its first allocations: the stored bricks exceed max_nodes, known once they are classified
        ok = ra.DistanceFieldHip.banded(hm, cell=0.25, band=0.5)
        bi = ok.band_info()
        need = 729 * bi["n_stored"] + bi["n_coarse"]
        ok.close()
        assert _live(ra) == held
        with pytest.raises(ra.RmclHipError, match="max_nodes"):
            ra.DistanceFieldHip.banded(hm, cell=0.25, band=0.5, max_nodes=need - 1)
        assert _live(ra) == held
        for kw in (dict(band=0.0), dict(band=math.nan), dict(cell=-1.0), dict(cell=1e-6)):
            with pytest.raises(ra.RmclHipError):
                ra.DistanceFieldHip.banded(hm, **kw)
        assert _live(ra) == held
        # a dataset that grows, then shrinks: the ray-casting operator (model buffers of the model) and the closest-point operator
        # (model buffers of the dataset)
        model, Tsb = _model(ra), syn.tsb_offset()
        truth, est = _poses(ra)
        rng = np.random.RandomState(4)
        rcc, cpc = ra.RCCHipSpherical(hm), ra.CPCHip(hm)
        rcc.setTsb(Tsb)
        rcc.setModel(model)
        grown = 0
        for n in (64, 4099, 16):
            pts = rng.uniform(-4.0, 4.0, (n, 3)).astype(np.float32)
            for op in (rcc, cpc):
                op.set_dataset(pts, np.ones(n, np.uint8))
                op.find(est)
                op.computeCrossStatistics(T.identity())
            grown = max(grown, _live(ra)[0])
            assert _live(ra)[0] == grown                                # grow-only: shrinking the dataset frees nothing
        rcc.close()
        cpc.close()
        hm.release()
