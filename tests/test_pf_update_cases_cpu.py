"""The cases of tests/pf_update_cases.py are what they claim to be -- checked on the CPU oracle alone, so that the GPU test
(tests/test_gpu_pf_update_hard.py) cannot pass vacuously: every class of beam occurs on every map in a stated share, the oracle's BVH walk
equals its brute force bit for bit, the deep maps need more stack rows than the kernel keeps in LDS, the duplicated maps have more
records than faces, the filter trees have leaves of one and of two records, EVERY ray of every case lies inside the envelope in which
the slab test stays in float32, every row of the edge table produces the class written next to it, and the three modes differ."""
import numpy as np
import pytest

import pf_update_cases as uc

# shares of the beam classes on the oracle's brute force, mode 0: (geometric, -100, -101, -102) at least
SHARE_FLOOR = {name: (0.25, 0.05, 0.03, 0.03) for name in uc.MAPS}
for _name in uc.SMALL_MAPS + ("nested200",):
    SHARE_FLOOR[_name] = (0.10, 0.05, 0.03, 0.03)


@pytest.mark.parametrize("name", uc.MAPS)
def test_map_case_holds_every_class_and_the_bvh_walk_agrees(orc, name):
    c = uc.update_case(name, orc)
    out = {}
    for mode in uc.MODES:
        a, e = uc.reference(c, orc, mode)
        a2, e2 = uc.reference(c, orc, mode, bvh=True)
        msg = uc.first_beam_difference("%s mode %d (BVH walk, brute force)" % (name, mode), e2, e)
        assert msg is None, msg
        assert a2.tobytes() == a.tobytes(), "%s mode %d: attributes of the BVH walk and of brute force differ" % (name, mode)
        assert np.array_equal(a["state_sigma"], c["attrs"]["state_sigma"])
        sh = uc.shares(e)
        fresh = c["attrs"]["likelihood"]["n_meas"] == 0
        pos = float((a["likelihood"]["mean"][fresh] > 0).mean())
        geo = e[uc.beam_class(e) == uc.GEO]
        print("[pf-update] %-10s mode %d  geometric %.3f  -100 %.3f  -101 %.3f  -102 %.3f  NaN %.3f  | mean > 0: %.2f of the particles without history"
              " | geometric errors %.3g .. %.3g" % ((name, mode) + tuple(sh) + (pos, geo[geo > 0].min() if (geo > 0).any() else 0.0, geo.max())))
        if mode == 0:
            for k, floor in enumerate(SHARE_FLOOR[name]):
                assert sh[k] >= floor, "%s: share of %s is %.3f, below %.2f" % (name, uc.CLASS_NAMES[k], sh[k], floor)
        assert pos >= 1.0 / 3.0, "%s mode %d: only %.2f of the particles end with likelihood.mean > 0" % (name, mode, pos)
        out[mode] = e
    for m1, m2 in ((0, 2), (0, 3), (2, 3)):
        differ = out[m1].view(np.uint32) != out[m2].view(np.uint32)
        assert differ.any(), "%s: modes %d and %d agree on every beam" % (name, m1, m2)
    # the real-miss beams are the ones made for it, on every particle and in every mode
    miss = np.isin(uc.beam_class(out[0]), (uc.C_RMSH, uc.C_RMSM))
    assert np.array_equal(miss | (uc.beam_class(out[0]) == uc.C_NAN), np.broadcast_to(c["real_miss"], miss.shape) | (uc.beam_class(out[0]) == uc.C_NAN))
    assert (c["beams"]["orig"]["x"] != 0).sum() >= 4


@pytest.mark.parametrize("name", uc.MAPS)
def test_every_ray_is_inside_the_float32_envelope(orc, name):
    c = uc.update_case(name, orc)
    ok = uc.in_envelope(c["v"], c["poses"], c["beams"])
    assert ok.all(), "%s: %d of %d rays leave the envelope, first %s" % (name, (~ok).sum(), ok.size, np.argwhere(~ok)[:4].tolist())
    O, D = uc.rays(c["poses"], c["beams"])
    assert (D != 0).all(), "%s: a direction component is exactly 0" % name


def test_table_rays_are_inside_the_envelope(orc):
    cases = [uc.edge_case(), uc.sigma_case(orc)] + [uc.tfar_case(o) for o in uc.TFAR_OFFSETS] + [uc.shape_case(*s) for s in uc.SHAPES]
    for c in cases:
        ok = uc.in_envelope(c["v"], c["poses"], c["beams"])
        assert ok.all(), "%s: %d rays leave the envelope" % (c["name"], (~ok).sum())


def test_filter_trees_are_deep_duplicated_and_mixed():
    """the filter's own tree (leaves of at most two records, the one k_pf_update_v3 walks by default), built on the host"""
    one_and_two = [0, 0]
    for name in uc.MAPS:
        info, n1, n2 = uc.filter_tree(name)
        print("[pf-update] %-10s n_faces %6d n_tri_records %6d n_nodes %6d stack_need %2d leaves of one record %5d, of two %5d" % (
            name, info["n_faces"], info["n_tri_records"], info["n_nodes"], info["stack_need"], n1, n2))
        if name in uc.SPILL_MAPS:
            assert uc.PF_ROWS < info["stack_need"] <= 64, name
        if name in uc.DEEP_MAPS:
            assert info["stack_need"] >= 59, name
        if name in uc.DUPLICATE_MAPS:
            assert info["n_tri_records"] > info["n_faces"], name
        else:
            assert info["n_tri_records"] >= info["n_faces"], name
        if info["n_faces"] > 3:
            # (maps whose every leaf holds two records exist: an even count of equal quads; the mix is asked of the hard maps)
            if name in uc.SPILL_MAPS + ("farsoup", "degcube"):
                assert n1 > 0 and n2 > 0, name
            assert n2 > 0, name
        else:
            one_and_two[0] += n1
            one_and_two[1] += n2
    assert one_and_two[0] > 0 and one_and_two[1] > 0       # tri1: one leaf of one record (the tree IS that leaf); tri2: one of two; tri3: both


def _edge_refs(orc):
    c = uc.with_mesh(uc.edge_case(), orc)
    return c, {mode: uc.reference(c, orc, mode) for mode in uc.MODES}


def test_edge_table_rows_produce_the_class_written_next_to_them(orc):
    c, refs = _edge_refs(orc)
    bad = []
    for label, pi, bi, expect in c["rows"]:
        got = {mode: int(uc.beam_class(refs[mode][1])[pi, bi]) for mode in uc.MODES}
        print("[pf-update] edge: %-45s particle %-15s beam %-9s -> %s" % (label, c["pnames"][pi], c["bnames"][bi], "  ".join(
            "mode %d %s (%.9g)" % (m, uc.CLASS_NAMES[got[m]], refs[m][1][pi, bi]) for m in uc.MODES)))
        if got != expect:
            bad.append((label, got, expect))
    assert not bad, "rows whose class is not the table's: %s" % bad
    for pi, bi, want in c["analytic"]:
        for mode in (0, 3):
            got = float(refs[mode][1][pi, bi])
            assert abs(got - want) <= 1e-5 * want, "edge (%s, %s) mode %d: error %r, analytic %r" % (c["pnames"][pi], c["bnames"][bi], mode, got, want)
    # the NaN pattern of the attributes: the oracle's brute force defines it, and it is not empty (a NaN range poisons nothing, a NaN pose
    # gives penalties) -- printed for the record
    for mode in uc.MODES:
        a = refs[mode][0]
        print("[pf-update] edge mode %d: %d particles with a NaN mean, %d NaN beam errors" % (mode, np.isnan(a["likelihood"]["mean"]).sum(), np.isnan(refs[mode][1]).sum()))


def test_edge_table_bvh_walk_agrees(orc):
    c, refs = _edge_refs(orc)
    for mode in uc.MODES:
        a2, e2 = uc.reference(c, orc, mode, bvh=True)
        msg = uc.first_beam_difference("edge mode %d (BVH walk, brute force)" % mode, e2, refs[mode][1])
        assert msg is None, msg
        assert a2.tobytes() == refs[mode][0].tobytes()


def test_tfar_cases_split_mode_3_from_mode_0(orc):
    for off in uc.TFAR_OFFSETS:
        c = uc.with_mesh(uc.tfar_case(off), orc)
        cls = {mode: uc.beam_class(uc.reference(c, orc, mode)[1]) for mode in uc.MODES}
        print("[pf-update] tfar %g: classes %s" % (off, {m: cls[m].tolist() for m in uc.MODES}))
        assert (cls[0][:, :2] == uc.GEO).all() and (cls[2][:, :2] == uc.GEO).all() and (cls[0][:, 2] == uc.C_RMSH).all()
        if off < 1.0e4:
            assert (cls[3][:, :2] == uc.GEO).all() and (cls[3][:, 2] == uc.C_RMSH).all()
        else:
            assert (cls[3][:, :2] == uc.C_RHSM).all() and (cls[3][:, 2] == uc.C_RMSM).all()


def test_shape_table_covers_the_workgroup_rules():
    """particles per workgroup of rmclhip_pf_update (capi_pf.cpp: pf_enqueue), restated: 2048 / n_beams in [1, 64]; at most 16 in the
    accumulating form; halved while the launch has fewer than 1024 workgroups and half a workgroup still holds 256 rays"""
    def ppb(n, nb, accum):
        pb = min(max(2048 // nb, 1), 64)
        if accum:
            pb = min(pb, 16)
        halved = False
        while pb > 1 and n // pb < 1024 and (pb >> 1) * nb >= 256:
            pb >>= 1
            halved = True
        return pb, halved
    seen = set()
    for n, nb in uc.SHAPES:
        assert nb <= uc.MAX_BEAMS
        for accum in (True, False):
            pb, halved = ppb(n, nb, accum)
            first = min(max(2048 // nb, 1), 64)
            seen.add("capped" if accum and first > 16 else "quotient")
            seen.add("halved" if halved else "kept")
            if n % pb:
                seen.add("partial")
            if pb == 1:
                seen.add("one particle")
            if nb == 1:
                seen.add("one beam")
            print("[pf-update] shape %5d x %4d %s: %2d particles per workgroup%s" % (n, nb, "accumulating" if accum else "stored      ", pb, ", partial last" if n % pb else ""))
    assert seen == {"capped", "quotient", "halved", "kept", "partial", "one particle", "one beam"}


def test_sigma_case_sits_at_the_peak(orc):
    c = uc.sigma_case(orc)
    a, e = uc.reference(c, orc, 0)
    assert (e[:c["n_truth"]] == 0).all(), "particles at the truth: errors %s" % e[:c["n_truth"]].max()
    peak = 1.0 / np.sqrt(2.0 * np.pi * float(np.float32(uc.SIGMA_MIN)) ** 2)
    fresh = c["attrs"]["likelihood"]["n_meas"][:c["n_truth"]] == 0
    got = a["likelihood"]["mean"][:c["n_truth"]][fresh]
    print("[pf-update] dist_sigma %.9g: peak eval %.6g (2^32 = %.6g), means at the truth %.6g .. %.6g" % (uc.SIGMA_MIN, peak, 2.0 ** 32, got.min(), got.max()))
    assert 3.9e9 < peak < 2.0 ** 32 and np.allclose(got, peak, rtol=1e-5)
    assert np.isfinite(a["likelihood"]["mean"]).all() and (a["likelihood"]["mean"][c["n_truth"]:][c["attrs"]["likelihood"]["n_meas"][c["n_truth"]:] == 0] == 0).all()
    assert uc.SIGMA_BELOW < uc.SIGMA_MIN == float(np.float32(1e-10))
