"""Every size, correspondence set, model, pose list and scene of the pose information's edge tests
(tests/test_gpu_pose_information_edges.py), made from fixed seeds -- and proved fit for their purpose without a device by
tests/test_pose_information_cases_cpu.py.

What the sizes are for: k_pose_information_partials (rmcl_amd/csrc/pose_information.hip) writes one row of 32 doubles per workgroup,
rows(n, nposes) of them per pose, and k_pose_information_finalize folds a pose's rows with one wave: half-wave g = lane >> 5 takes the
rows g, g + 2, ..., eight of them per trip of its unrolled loop (entered while b + 14 < rows, b = g, g + 16, ...), the rest one by one.

FREE_SIZES    one n per row count 1, 2, 14, 15, 16, 17, 31, 32, 33, each ragged in its last row: below the unrolled loop; g = 0 alone
              in it (15); both halves in it (16, 17); a second trip, then tails of 0, 1 and 2 rows (31, 32, 33)
CAP_SIZE      above 1024 * 512 the row count stays 1024 and the lanes stride by gridDim.x * 256: a third trip for 257 lanes only
batch_model() 67 x 131 = 8777 rays: 18 rows per pose below four poses, 3 rows of 4096 correspondences from four poses on
SCENES        what a find returns in a scan of one plane, from the centre of a sphere, and between two parallel walls
"""
import math

import numpy as np

import cpc_cases
import pose_batch_cases as pc

F = np.float32
MAX_DIST = F(0.3)


# ---- the row rule -------------------------------------------------------------------------------------------------------------------
def rows(n, nposes=1):
    """reduce_num_blocks of rmcl_amd/csrc/kernels.hip, restated: 512 correspondences per workgroup below four poses, 4096 from four
    poses on, at least one row, at most 1024"""
    per_block = 4096 if nposes >= 4 else 512
    return min(max((n + per_block - 1) // per_block, 1), 1024)


FREE_ROWS = (1, 2, 14, 15, 16, 17, 31, 32, 33)
FREE_SIZES = (511, 513, 6911, 7169, 7937, 8193, 15361, 16383, 16385)
FAR_ROWS = (15, 17, 33)                     # the row counts that also run with far=True
CAP_SIZE = 1024 * 512 + 257
CAP_ROWS = 1024
MASK_SETTINGS = ((True, True), (False, True), (True, False))       # (dataset mask given, model mask given)
POISON_AT = (0, 63, 64, 255, 256)           # + n - 1: both ends of a wave, both ends of the first 256 lanes, the ragged end
POISON_KINDS = ("nan_dataset", "inf_model", "nan_normal")
FAR_CANCELLING = (0, 3)                     # the entry of A that free_case(far=True) makes cancel


def free_seed(n, far=False):
    return 4000 + n + (100000 if far else 0)


# ---- correspondences of the free function ---------------------------------------------------------------------------------------------
def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def poison_rows(n):
    """{index: kind} of the rows that must not reach the sums (both masks 1): POISON_AT and n - 1, as many as n allows"""
    at = sorted(set(i for i in POISON_AT + (n - 1,) if 0 <= i < n))
    return {i: POISON_KINDS[k % 3] for k, i in enumerate(at)}


def zero_normal_rows(n):
    """the rows with a zero normal (both masks 1, finite points): the lane neighbour i ^ 1 of every poisoned row, where that is a row
    and not poisoned itself.  They pass the gate (r = 0), count in n_meas and add zeros to every sum."""
    p = poison_rows(n)
    return sorted(i ^ 1 for i in p if (i ^ 1) < n and (i ^ 1) not in p)


def free_case(n, seed, far=False):
    """n random correspondences, the recipe of tests/test_gpu_pose_information.py _free_case: dataset points within +-10 m, unit
    normals, residuals uniform in +-0.6 m against a gate of 0.3 m (about half inside), model points off the foot point along the
    plane, dataset mask 90 % and model mask 85 % ones, model points and normals NaN where the model mask is 0 (I_nan, N_nan).

    poison_rows(n) and zero_normal_rows(n) are written over that.

    far=True: everything moves by cpc_cases.FAR_OFFSET, so the entries of D x N are some thousand metres, and the rows come in lane
    pairs (2 j, 2 j + 1) that share masks and residual, lie within half a metre of each other and mirror their normals in x.  A pair
    is kept or rejected as one under the identity pre-transform (no residual within 1 cm of the gate).  Its terms of sum N_x N_y and
    sum N_x N_z cancel exactly, those of A[0, 3] = sum N_x (D x N)_x to the 1e-4 by which the two points differ: FAR_CANCELLING
    names that entry, whose sum is far below 1e-3 of the sum of its terms' magnitudes and is not zero."""
    rng = np.random.RandomState(seed)
    D = rng.uniform(-10.0, 10.0, (n, 3))
    N = _unit(rng.normal(size=(n, 3))).astype(F)
    r = rng.uniform(-0.6, 0.6, n)
    side = rng.normal(size=(n, 3))
    dmask = (rng.uniform(size=n) < 0.9).astype(np.uint8)
    mmask = (rng.uniform(size=n) < 0.85).astype(np.uint8)
    if far:
        odd = np.arange(1, n, 2)
        D[odd] = D[odd - 1] + rng.uniform(-0.5, 0.5, (len(odd), 3))
        N[odd] = N[odd - 1] * np.array([-1.0, 1.0, 1.0], F)
        r[odd], dmask[odd], mmask[odd] = r[odd - 1], dmask[odd - 1], mmask[odd - 1]
        r = np.where(np.abs(np.abs(r) - float(MAX_DIST)) < 0.01, 0.5 * r, r)
        D = D + np.asarray(cpc_cases.FAR_OFFSET)
    D = D.astype(F)
    tang = np.cross(N.astype(np.float64), side) * 0.2
    I = (D.astype(np.float64) + N.astype(np.float64) * r[:, None] + tang).astype(F)
    poison, zero = poison_rows(n), zero_normal_rows(n)
    for i, kind in poison.items():
        dmask[i] = mmask[i] = 1
        if kind == "nan_dataset":
            D[i, i % 3] = np.nan
        elif kind == "inf_model":
            I[i, i % 3] = np.inf if i % 2 else -np.inf
        else:
            N[i, i % 3] = np.nan
    for i in zero:
        dmask[i] = mmask[i] = 1
        N[i] = 0.0
    I_nan, N_nan = I.copy(), N.copy()
    I_nan[mmask == 0] = np.nan
    N_nan[mmask == 0] = np.nan
    return dict(D=D, I=I, N=N, I_nan=I_nan, N_nan=N_nan, dmask=dmask, mmask=mmask, poison=poison, zero=zero, far=far)


def tpre_general(far=False):
    """a pre-transform of some hundredths of a radian and some centimetres; for the far cases it turns about FAR_OFFSET, so that the
    points stay beside their model points"""
    from rmcl_amd import types as T
    t, rpy = (0.03, -0.02, 0.04), (0.01, -0.02, 0.015)
    if not far:
        return T.transform_from_rpy(t, rpy)
    c = np.asarray(cpc_cases.FAR_OFFSET, np.float64)
    q = np.array(T.euler_to_quat(*rpy), np.float64)
    u, w = q[:3], q[3]
    rc = c + 2.0 * np.cross(u, np.cross(u, c) + w * c)
    return T.transform(tuple(float(x) for x in q), tuple(float(x) for x in (c - rc + np.asarray(t))))


def reference(c, Tpre, use_d, use_m, max_dist=MAX_DIST):
    """pose_information_ref.pose_information of a free case under one mask setting: without the model mask the model arrays are
    the ones without NaN"""
    import pose_information_ref as pir
    pts, nrm = ("I_nan", "N_nan") if use_m else ("I", "N")
    return pir.pose_information(Tpre, c["D"], c["dmask"] if use_d else None, c[pts], c[nrm], c["mmask"] if use_m else None, max_dist)


# ---- the batch form -------------------------------------------------------------------------------------------------------------------
BATCH_H, BATCH_W = 67, 131
BATCH_RAYS = BATCH_H * BATCH_W              # 8777
BATCH_COUNTS = (1, 3, 4, 5, 9)              # both sides of reduce_num_blocks' switch at four poses
BATCH_MAX_DIST, BATCH_MAX_DIST_MIN = 1.0, 0.05        # the estimates are up to 8 cm off: the narrow gate rejects
SHORT_DATASET = 5000                        # the operator form's n = min(n_dataset, n_model) as the smaller of the two: 10 rows, ragged


def batch_model():
    """the spherical model of pose_batch_cases at 67 x 131 rays"""
    return pc.spherical_model(BATCH_H, BATCH_W)


def batch_truth():
    return pc.truth_and_estimates(1)[0]


def batch_empty(k):
    """(index of the pose 500 m away, index of the pose with a NaN translation) in batch_poses(k), None below four poses"""
    return (1, k - 2) if k >= 4 else (None, None)


def batch_poses(k):
    """k estimates within 8 cm and 0.02 rad of batch_truth(), inside the cube room; from four poses on, two of them are replaced by
    a pose that sees nothing and a pose with a NaN translation (batch_empty)"""
    from rmcl_amd import types as T
    poses = pc.truth_and_estimates(9)[1][:k].copy()
    far, nan = batch_empty(k)
    if far is not None:
        poses[far] = pc.far_pose()
        poses[nan] = T.transform_from_rpy((float("nan"), 2.0, 1.0), (0.0, 0.0, 0.3))
    return poses


def adaptive(max_dist, amin, p):
    """CorrespondencesCPU.cpp:21-23: float operands, double arithmetic, float store"""
    return float(F(np.float64(F(max_dist)) * (1.0 - p) + np.float64(F(amin)) * p))


# ---- scenes of the degeneracy report ------------------------------------------------------------------------------------------------
def two_walls_map():
    """two 16 m x 16 m squares at y = -2 and y = +2 that face each other"""
    v = np.array([[-8.0, -2.0, -8.0], [8.0, -2.0, -8.0], [8.0, -2.0, 8.0], [-8.0, -2.0, 8.0],
                  [-8.0, 2.0, -8.0], [8.0, 2.0, -8.0], [8.0, 2.0, 8.0], [-8.0, 2.0, 8.0]], np.float32)
    return v, np.array([[0, 2, 1], [0, 3, 2], [4, 5, 6], [4, 6, 7]], np.uint32)


def _scan_model(phi_min, phi_max, h, w):
    from rmcl_amd import types as T
    return T.spherical_model(F(phi_min), F((phi_max - phi_min) / (h - 1)), h, F(-math.pi), F(2 * math.pi / w), w, F(0.1), F(40.0))


SCENES = ("plane", "sphere_centre", "two_walls")


def scene(name):
    """dict: map (v, f), model, truth, estimate (the sensor sits in the base's origin: Tsb is the identity), max_dist, params (the
    keyword arguments of types.pose_covariance), n_degenerate (trans, rot) at those parameters, n_deficient (eigenvalues of A at or
    below rcond * lam_max), zero_rows (the rows and columns of A that are exactly zero)

    plane          pose_batch_cases.quad_map(), the sensor 1.5 m above it with an identity quaternion at truth and estimate: every
                   normal is exactly (0, 0, 1), u = [0, 0, 1, D_y, -D_x, 0, r]: rows and columns 0, 1 and 5 of A are exact zeros.
                   Eigenvalues of A / n_meas (tests/test_pose_information_cases_cpu.py prints them), translation block
                   0, 0, 1; rotation block 0, 4.234, 4.336: min_eig 1e-3 for both.
    sphere_centre  sphere20k from (nearly) its centre: D is parallel to N up to the facets' tilt and the estimate's few centimetres,
                   so the rotation block is small and not zero.  Translation block 0.3140, 0.3144, 0.3716; rotation block
                   0.00683, 0.00774, 0.01662: min_eig_trans 1e-3, min_eig_rot 0.2 -- nothing degenerate among the translations,
                   every rotation reported.  rcond 1e-9 cuts nothing: the covariance is s2 inv(A).
    two_walls      two_walls_map() from a turned pose between the walls: every normal is +-a for one unit vector a, translation
                   across a and rotation about a are free, in directions that are no coordinate axes.  Translation block
                   -2.7e-17, 1.1e-18, 1; rotation block 2.1e-15, 6.576, 8.745: min_eig 1e-3 for both."""
    from rmcl_amd import synthetic as syn, types as T
    if name == "plane":
        return dict(map=pc.quad_map(), model=_scan_model(-1.3, 0.3, 33, 96), truth=T.transform_from_rpy((0.4, -0.7, 1.5), (0.0, 0.0, 0.0)),
                    estimate=T.transform_from_rpy((0.45, -0.73, 1.54), (0.0, 0.0, 0.0)), max_dist=1.0,
                    params=dict(sigma=0.02, degenerate_variance=50.0, rcond=1e-9, min_eig_trans=1e-3, min_eig_rot=1e-3),
                    n_degenerate=(2, 1), n_deficient=3, zero_rows=(0, 1, 5))
    if name == "sphere_centre":
        return dict(map=syn.uv_sphere(20000), model=_scan_model(-1.2, 1.2, 41, 88), truth=T.identity(),
                    estimate=T.transform_from_rpy((0.04, -0.03, 0.02), (0.01, -0.02, 0.015)), max_dist=1.0,
                    params=dict(sigma=0.02, degenerate_variance=50.0, rcond=1e-9, min_eig_trans=1e-3, min_eig_rot=0.2),
                    n_degenerate=(0, 3), n_deficient=0, zero_rows=())
    assert name == "two_walls"
    truth = T.transform_from_rpy((0.3, 0.1, -0.2), (0.05, -0.04, 0.3))
    return dict(map=two_walls_map(), model=_scan_model(-1.2, 1.2, 41, 88), truth=truth,
                estimate=T.mult(truth, T.transform_from_rpy((0.03, 0.04, -0.02), (0.01, -0.015, 0.02))), max_dist=1.0,
                params=dict(sigma=0.02, degenerate_variance=50.0, rcond=1e-9, min_eig_trans=1e-3, min_eig_rot=1e-3),
                n_degenerate=(2, 1), n_deficient=3, zero_rows=())


def scene_dataset(orc, mesh, s):
    """(points, mask): the scan the truth measures, as a dataset in the sensor frame"""
    from rmcl_amd import types as T
    meas = mesh.simulate_spherical(s["model"], T.identity(), s["truth"], bvh=False)
    return (orc.spherical_directions(s["model"]) * meas["ranges"][:, None]).astype(F), meas["hits"]


# ---- the covariance and the step, restated with numpy's eigh -------------------------------------------------------------------------
def covariance_by_eigh(A, g, s2, rcond, degenerate_variance):
    """(covariance, xi, V, kept): rmclhip_pose_covariance_host's and rmclhip_pose_information_solve_host's construction from numpy's
    eigenpairs of A with the same cut rcond * lam_max; the columns of V[:, ~kept] span the deficient directions"""
    lam, V = np.linalg.eigh(np.asarray(A, np.float64))
    kept = (lam > rcond * lam.max()) & (lam > 0.0)
    c = np.where(kept, s2 / np.where(kept, lam, 1.0), degenerate_variance)
    Vk = V[:, kept]
    return (V * c) @ V.T, Vk @ ((Vk.T @ np.asarray(g, np.float64)) / lam[kept]), V, kept


COV_TOL = 1e-10     # of the norm: what tests/test_pose_information_cpu.py holds the covariance to against s2 inv(A)


def check_host_algebra(T, info, s, what=""):
    """types.pose_covariance and types.pose_information_solve of the record `info` with the scene's parameters against
    covariance_by_eigh: the covariance as a whole and on the constrained subspace, the step, degenerate_variance along every deficient
    direction and no step along it, symmetry bit for bit, the report's counts.  Returns (cov, xi, V, kept)."""
    p = s["params"]
    cov = T.pose_covariance(info, **p)
    xi = T.pose_information_solve(info, p["rcond"])
    want, want_xi, V, kept = covariance_by_eigh(info["A"], info["g"], p["sigma"] ** 2, p["rcond"], p["degenerate_variance"])
    C = np.asarray(cov["covariance"], np.float64)
    assert np.array_equal(C, C.T), "%s: covariance not symmetric" % what
    assert float(cov["s2"]) == p["sigma"] ** 2
    assert np.linalg.norm(C - want) <= COV_TOL * np.linalg.norm(want), "%s: covariance" % what
    # on the constrained subspace: the stored entries are six-term sums that carry degenerate_variance, so each is rounded by some
    # 2^-52 of the whole covariance's size, which the projection cannot take back; with degenerate_variance 0 the constrained part
    # stands alone and meets the tolerance of its own size
    P = V[:, kept] @ V[:, kept].T
    assert np.linalg.norm(P @ (C - want) @ P) <= COV_TOL * np.linalg.norm(P @ want @ P) + 8.0 * 2.0 ** -52 * np.linalg.norm(want), \
        "%s: covariance on the constrained subspace" % what
    alone = np.asarray(T.pose_covariance(info, **dict(p, degenerate_variance=0.0))["covariance"], np.float64)
    want_alone = covariance_by_eigh(info["A"], info["g"], p["sigma"] ** 2, p["rcond"], 0.0)[0]
    assert np.array_equal(alone, alone.T), "%s: constrained part not symmetric" % what
    assert np.linalg.norm(alone - want_alone) <= COV_TOL * np.linalg.norm(want_alone), "%s: constrained part alone" % what
    assert np.linalg.norm(xi - want_xi) <= COV_TOL * np.linalg.norm(want_xi), "%s: step" % what
    for v in V[:, ~kept].T:
        assert abs(float(v @ C @ v) - p["degenerate_variance"]) <= COV_TOL * p["degenerate_variance"], "%s: variance along %s" % (what, v)
        assert abs(float(v @ xi)) <= COV_TOL * np.linalg.norm(xi), "%s: step along %s" % (what, v)
    assert (int(cov["n_degenerate_trans"]), int(cov["n_degenerate_rot"])) == s["n_degenerate"], what
    assert int((~kept).sum()) == s["n_deficient"], what
    return cov, xi, V, kept
