"""One localisation run of the particle filter, stage after stage, as a node makes it -- the scenario tests/test_gpu_filter_cycle.py runs
on long-lived handles and tests/test_filter_cycle_cpu.py proves non-vacuous on the restatements alone.

The map is the 12-face cube of band_field_ref.cube_mesh (walls at +-2 m), its fields the REFINE_CELL / REFINE_BAND fields of
tests/test_gpu_band_field.py (81^3 logical nodes, 216 of the 1000 bricks FAR).  A robot drives four odometry steps over the floor; after
every step a scan of 33 beams is taken at the true pose.  The cloud starts as 700 particles spread over the room plus 325 around the
truth, and every cycle runs

    motion update with the surface constraint and the collision test -> sensor update from the field (banded on even cycles, dense on
    odd ones) -> refine (even) or a Stein step (odd) and a second sensor update -> hypotheses and estimate -> visualisation pack ->
    adaptive resampling into the other buffer pair

with a kidnap after cycle 1: the upper half of the live cloud is spread over the room again and put on the floor.

The cube looks the same after a quarter turn about z, so a cloud spread over every heading has four equal modes and nothing to
converge to: the spread clouds draw their yaw from +-0.7 rad around the odometry's first heading, as a node with a compass would.  On
the flat floor the aligned particles have roll = pitch = 0 up to rounding, and (0 + pi) / 0.17453292 is 18 to the last bit -- a bin
edge: the roll and pitch bins are 0.2 rad wide (pi / 0.2 = 15.7), the yaw bins the usual 0.17453292.

Every function below is a pure function of its stage's input, built from the restatements the stages' own tests use; chain() strings
them together.  Not a test module.
"""

import numpy as np

import adaptive_ref as ar
import band_field_ref as bfr
import field_ref as fr
import hypotheses_ref as hr
import particle_init_ref as pref
import pf_cycle_cases as pc
import refine_ref as rr
import stein_ref as st
import surface_ref as sr

F = np.float32
CAPACITY, GUARD = 1537, 3                       # records per buffer, and 0xFF records on both sides of it
N0, N_UNIFORM, N_BEAMS = 1025, 700, 33          # slots [0, 700) uniform, [700, 1025) around the truth; one beam more than half a wave
CELL, BAND = 0.05, 0.3
SEED = 0xC0FFEE1234567
EPOCH, KIDNAP_EPOCH = 1, 2
N_CYCLES, KIDNAP_AFTER, ASYNC_CYCLE = 4, 1, 1
MAX_N_MEAS, DIST_SIGMA, FORGET_RATE = 10000, 0.05, 0.1
MAX_HYPOTHESES = 8
UNDECIDED_TOL = 1e-5                            # of a bin width: seven times an ulp of an angle <= pi (2.4e-7 rad) over the 0.1745 rad bin

HEIGHT = 0.3
SURFACE = sr.params(axis=0, height=HEIGHT, probe_up=0.5, probe_down=1.0, min_up_cos=0.7, align=1, on_miss=1)
YAW0 = 0.5
TRUTH0 = ((-0.6, -0.5, -2.0 + HEIGHT), (0.0, 0.0, YAW0))           # on the floor
# x y z roll pitch yaw: over the room, from on the floor to too high for the probe (z > -0.7: a miss), a quarter-turn window of yaw
BOX = ((-1.8, -1.8, -1.9, -0.1, -0.1, YAW0 - 0.7), (1.8, 1.8, -0.3, 0.1, 0.1, YAW0 + 0.7))
POSE_COV = np.diag([0.04, 0.04, 0.0025, 0.0004, 0.0004, 0.02])
# T_bnew_bold of the four cycles, in the body frame: (translation, rpy); 0.4 m and more carries particles near a wall through it
STEPS = (((0.4, 0.0, 0.0), (0.0, 0.0, 0.1)), ((0.3, 0.1, 0.0), (0.0, 0.0, -0.2)), ((0.45, 0.0, 0.0), (0.0, 0.0, 0.15)),
         ((0.2, -0.1, 0.0), (0.0, 0.0, 0.1)))
# The likelihood is a mean of per-beam densities, and a third of the beams end on the floor or the ceiling, which every particle on the
# floor matches: a stray scores a third to a half of what the truth scores.  The floor of 0.5 counts the particles that match the
# walls as well; the bins of 0.35 m keep the lucky strays apart from them.
KLD = ar.Kld(bin_xyz=(0.35, 0.35, 0.35), bin_rpy=(0.2, 0.2, 0.17453292), min_likelihood_rel=0.5, epsilon=0.05, n_min=64)
NOISE = dict(min_noise_tz=0.01, min_noise_roll=0.005, min_noise_pitch=0.005)
REFINE = rr.params(iterations=4, max_dist=BAND)
STEIN_MAX_PER_BIN = 64                          # a converged cloud fills one 0.25 m bin with more than that: the thinned path


def stein_params(cycle):
    return st.params(iterations=2, max_dist=BAND, max_per_bin=STEIN_MAX_PER_BIN, seed=SEED, step=cycle)


def field_kind(cycle):
    return "banded" if cycle % 2 == 0 else "dense"


def third_stage(cycle):
    return "refine" if cycle % 2 == 0 else "stein"


class World:
    """the map, the trajectory and the scans; the fields' arrays are given by the caller: the oracle's lattice on the CPU, the device's
    own downloads on the GPU (set_fields)"""

    def __init__(self, ra, orc):
        from rmcl_amd import synthetic as syn, types as T
        self.v, self.f = bfr.cube_mesh()
        assert len(self.f) == 12
        self.mesh = orc.Mesh(self.v, self.f)
        self.normals = self.mesh.face_normals()
        self.logical, self.bricks = bfr.layout(self.v.min(axis=0), self.v.max(axis=0), CELL, 0.0, BAND)
        self.Tsb = np.ascontiguousarray(syn.tsb_offset()).reshape(1)
        self.steps = [T.transform_from_rpy(t, rpy) for t, rpy in STEPS]
        self.truth = [np.array([T.transform_from_rpy(*TRUTH0)]).reshape(1)]       # truth[c]: before cycle c's motion
        self.beams = []
        for c in range(N_CYCLES):
            self.truth.append(np.array([orc.tmult(self.truth[c][0], self.steps[c])]).reshape(1))
            cloud = self.mesh.simulate_spherical(syn.model_c1(), self.Tsb[0], self.truth[c + 1][0], bvh=True)["points"]
            self.beams.append(ra.sample_beams(cloud, N_BEAMS, seed=7 + c))
            assert len(self.beams[c]) == N_BEAMS
        self.lattice = self.banded = None

    def set_fields(self, lattice, banded=None):
        """lattice: the dense field's nodes [n_z, n_y, n_x]; banded: dict(table, coarse, bricks), default the restatement's cut of it"""
        self.lattice = np.asarray(lattice, F)
        self.banded = bfr.build(self.logical, self.bricks, self.lattice) if banded is None else banded


# ---- the stages, each from its input alone ----------------------------------------------------------------------------------------------
def init_slices():
    """[(first, count, poses, attrs, translations exact)]: the two slices of the start"""
    pu, au = pref.init_uniform(0, N_UNIFORM, BOX[0], BOX[1], SEED, EPOCH)
    from rmcl_amd import types as T
    pp, ap = pref.init_pose(N_UNIFORM, N0 - N_UNIFORM, T.transform_from_rpy(*TRUTH0), POSE_COV, SEED, EPOCH)
    return [(0, N_UNIFORM, pu, au, True), (N_UNIFORM, N0 - N_UNIFORM, pp, ap, False)]


def kidnap_slice(n):
    """(first, count, poses, attrs): the upper half of a cloud of n, spread over the room again"""
    first = n // 2
    p, a = pref.init_uniform(first, n - first, BOX[0], BOX[1], SEED, KIDNAP_EPOCH)
    return first, n - first, p, a


def constrain(w, poses, attrs):
    """-> (poses', attrs', stats)"""
    return sr.constrain(w.mesh, poses, attrs, SURFACE, MAX_N_MEAS, normals=w.normals)[:3]


def motion(w, cycle, poses, attrs):
    """-> (poses', attrs', stats, killed)"""
    return sr.motion_update(w.mesh, poses, attrs, w.steps[cycle], FORGET_RATE, True, SURFACE, MAX_N_MEAS, normals=w.normals)


def end_points(w, cycle, poses):
    """[n, N_BEAMS, 3]: refine_ref's vectorised end points -- tests/test_filter_cycle_cpu.py holds them to field_ref.end_points' bytes"""
    R, t = rr.pose_arrays(poses)
    return rr.end_points(R, t, w.Tsb, w.beams[cycle])


def sensor(w, cycle, poses, attrs):
    """-> (errors [n, N_BEAMS], attrs', stored [n, N_BEAMS]: the end point's brick is STORED)"""
    ends = end_points(w, cycle, poses).reshape(-1, 3)
    if field_kind(cycle) == "banded":
        e = bfr.lookup(w.logical, w.bricks, w.banded, ends)
    else:
        e = fr.lookup(w.logical, w.lattice, ends)
    e = e.reshape(len(poses), N_BEAMS)
    mean, sigma, n_meas = fr.chain(attrs, e, DIST_SIGMA, MAX_N_MEAS)
    out = attrs.copy()
    out["likelihood"]["mean"], out["likelihood"]["sigma"], out["likelihood"]["n_meas"] = mean, sigma, n_meas
    return e, out, bfr.stored_mask(w.logical, w.bricks, w.banded["table"], ends).reshape(len(poses), N_BEAMS)


def move(w, cycle, poses):
    """stage 3 -> (poses', rows, stats): refine on even cycles, the Stein step on odd ones.  With max_dist <= the band the banded field
    answers refine with the dense lattice's bytes (tests/test_gpu_band_field.py), so the dense lattice serves both"""
    if third_stage(cycle) == "refine":
        return rr.refine(w.logical, w.lattice, poses, w.beams[cycle], w.Tsb, REFINE)
    return st.step(w.logical, w.lattice, poses, w.beams[cycle], w.Tsb, stein_params(cycle))


def undecided(poses, attrs, kld, tol=UNDECIDED_TOL):
    """[n] bool: counted particles whose roll, pitch or yaw bin coordinate lies within tol (of a bin width) of a bin edge -- where an ulp
    between the device's and numpy's atan2 / asin may move them to the other bin.  The translation bins are IEEE divisions, the same on
    both sides."""
    counted = ar.counted_mask(poses, attrs, kld)
    c = ar._coords(poses, kld)[:, 3:].astype(np.float64)
    frac = c - np.floor(c)
    near = np.minimum(frac, 1.0 - frac) < tol
    used = np.array([wd != 0 for wd in kld.bin_rpy])
    return counted & (near & used[None, :]).any(axis=1)


def clusters(poses, attrs):
    return hr.hypotheses(poses, attrs, KLD, MAX_HYPOTHESES)


def n_new_of(k, capacity=CAPACITY):
    n_max = min(KLD.n_max, capacity)
    return ar.kld_bound(k, KLD.epsilon, KLD.z, min(KLD.n_min, n_max), n_max)


def with_index_stamps(poses):
    """stamp = index, as adaptive_ref.cloud: the resampler copies the stamp, so the source of every new slot can be read back"""
    out = poses.copy()
    out["stamp"] = np.arange(len(out), dtype=np.uint32)
    return out


def resample(cycle, poses, attrs, k=None):
    """-> (k, counted, n_new, poses_new, attrs_new, src); k: the count to take the bound from (default: the restatement's own)"""
    k_ref, counted = ar.count_bins(poses, attrs, KLD)
    n_new = n_new_of(k_ref if k is None else k)
    pn, an, src = ar.systematic(poses, attrs, n_new, ar.gladiator_cfg(**NOISE), SEED, cycle)
    return k_ref, counted, n_new, pn, an, src


# ---- the chain on the restatements ------------------------------------------------------------------------------------------------------
def position_error(pose, truth):
    return float(np.sqrt(sum((float(pose["t"][k]) - float(truth["t"][k])) ** 2 for k in "xyz")))


def line(r):
    return ("cycle %d (%s, %s): n %d -> %d, k %d, clusters %d, killed %d, snapped/missed/steep %d/%d/%d, end points FAR %d STORED %d, "
            "undecided %d of %d counted" % (r["cycle"], field_kind(r["cycle"]), third_stage(r["cycle"]), r["n"], r["n_new"], r["k"], r["n_clusters"],
                                            r["killed"], r["surface"]["n_snapped"], r["surface"]["n_missed"], r["surface"]["n_steep"], r["far"],
                                            r["stored"], r["undecided"], r["counted"]))


def chain(w):
    """the whole run on the restatements: (rows: one dict per cycle, the last estimate, the state after the last resampling)"""
    poses = np.concatenate([s[2] for s in init_slices()])
    attrs = np.concatenate([s[3] for s in init_slices()])
    poses, attrs, _ = constrain(w, poses, attrs)
    n, rows, est = N0, [], None
    for c in range(N_CYCLES):
        poses, attrs, surf, killed = motion(w, c, poses, attrs)
        _, attrs, stored = sensor(w, c, poses, attrs)
        poses, _, moved = move(w, c, poses)
        _, attrs, _ = sensor(w, c, poses, attrs)
        hyp = clusters(poses, attrs)
        est = pc.estimate_ref(poses, attrs)
        und = undecided(poses, attrs, KLD)
        k, counted, n_new, pn, an, _ = resample(c, with_index_stamps(poses), attrs)
        rows.append(dict(cycle=c, n=n, n_new=n_new, k=k, counted=counted, n_clusters=hyp["n_clusters"], killed=int(killed.sum()), surface=surf,
                         far=int((~stored).sum()), stored=int(stored.sum()), undecided=int(und.sum()), moved=moved,
                         error=position_error(est["pose"], w.truth[c + 1][0])))
        poses, attrs, n = pn, an, n_new
        if c == KIDNAP_AFTER:
            first, count, kp, ka = kidnap_slice(n)
            poses[first:], attrs[first:], _ = constrain(w, kp, ka)
    return rows, est, (poses, attrs)
