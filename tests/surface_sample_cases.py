"""Maps and shapes of the surface sampler's tests (CPU and GPU), each chosen for one way to go wrong.  Not a test module.

    twofloor     two 10 m squares at z = 0 and z = 3 (two faces each, one wound downwards: the flip), four vertical walls 6 m high (never
                 eligible) and one ramp of slope cosine 0.8 beside them: area 10 m^2, projected area 8 m^2 (density by area, not by
                 projection).  RAMP_ON / RAMP_OFF put min_up_cos on the ramp's float n.z and one ulp above it (the closed rule).
    cadmix20k    the builder takes spatial splits: n_tri_records > n_faces, every face weighs once; built again without them
                 (RMCLHIP_SBVH_ALPHA=0 in a child process) it gives the same table and the same clouds
    dupsoup      every face twice as distinct faces: both weigh
    degcube      zero-area faces weigh 0 and are never drawn
    scene        two instances of twofloor through rmclhip_map_create_scene: global face ids
    strip1025 / strip4097   equal floor triangles + one 2^20 times larger: the scan's block boundaries (1024 per block) and the weight range
    outside      the only up-facing face lies outside the region: creation is refused
    single       one eligible face beside a wall
    vertical     a wall with min_up_cos = 0 and align: the largest arc the alignment can turn (a quarter turn).  The half-turn branch
                 (w < 1e-6) of the surface constraint's step 5 cannot be reached by a draw: the normal is flipped to n.z >= 0 and the body z
                 before the arc is (0, 0, 1) up to rounding, so w = 1 + n.z >= 1; the restatement's align() is tested on that branch directly.
"""
import numpy as np

import field_cases as fc
import surface_sample_ref as ssr

F = np.float32
COUNTS = (1, 255, 256, 257, 4097)
SLICES = ((3, 300), (1021, 517))        # (first, count): the attribute stream starts off a 16-byte boundary
SEED = 0x5EEDF00D2468ACE1


def _quad(v, f, a, b, c, d, down=False):
    k = len(v)
    v += [a, b, c, d]
    f += [(k, k + 2, k + 1), (k, k + 3, k + 2)] if down else [(k, k + 1, k + 2), (k, k + 2, k + 3)]


def twofloor():
    v, f = [], []
    _quad(v, f, (0, 0, 0), (10, 0, 0), (10, 10, 0), (0, 10, 0))                    # faces 0 1: ground floor
    _quad(v, f, (0, 0, 3), (10, 0, 3), (10, 10, 3), (0, 10, 3))                    # faces 2 3: upper floor ...
    f[3] = (f[3][0], f[3][2], f[3][1])                                             # ... face 3 wound downwards
    for a, b in (((0, 0), (10, 0)), ((10, 0), (10, 10)), ((10, 10), (0, 10)), ((0, 10), (0, 0))):   # faces 4..11: walls
        _quad(v, f, (a[0], a[1], 0), (b[0], b[1], 0), (b[0], b[1], 6), (a[0], a[1], 6))
    _quad(v, f, (10, 0, 0), (14, 0, 3), (14, 2, 3), (10, 2, 0))                    # faces 12 13: the ramp, beside the floors
    return np.array(v, F), np.array(f, np.uint32)


TWOFLOOR_FLOOR0, TWOFLOOR_FLOOR1, TWOFLOOR_RAMP = (0, 1), (2, 3), (12, 13)


def strip(n):
    """n equal right triangles of legs 2^-4 on the floor + one of legs 64: 2^20 times their area"""
    d = 2.0 ** -4
    v, f = [], []
    for i in range(n):
        k = len(v)
        v += [(i * d, 0, 0), (i * d + d, 0, 0), (i * d, d, 0)]
        f.append((k, k + 1, k + 2))
    k = len(v)
    v += [(0, -100, 0), (64, -100, 0), (0, -36, 0)]
    f.insert(n // 2, (k, k + 1, k + 2))       # the large face in the middle of the ids
    return np.array(v, F), np.array(f, np.uint32)


def single():
    v = [(0, 0, 1), (2, 0, 1), (0, 3, 1), (0, 0, 0), (2, 0, 0), (2, 0, 2)]
    return np.array(v, F), np.array([(3, 4, 5), (0, 1, 2)], np.uint32)


def vertical():
    v = [(0, 0, 0), (4, 0, 0), (4, 0, 2), (0, 0, 2)]
    return np.array(v, F), np.array([(0, 1, 2), (0, 2, 3)], np.uint32)


def scene_parts():
    """(meshes, instances) of the two-instance scene: twofloor, and twofloor again 30 m along x and 1 m up"""
    A = np.eye(4, dtype=F)
    B = A.copy()
    B[0, 3], B[2, 3] = 30.0, 1.0
    return [twofloor()], [(0, A), (0, B)]


_maps = {}


def build_map(name):
    """(vertices, faces) made once per process; "scene" is the flattened scene (what the library's map holds)"""
    if name not in _maps:
        if name == "twofloor":
            _maps[name] = twofloor()
        elif name.startswith("strip"):
            _maps[name] = strip(int(name[5:]))
        elif name == "single":
            _maps[name] = single()
        elif name == "vertical":
            _maps[name] = vertical()
        elif name == "scene":
            import rmcl_amd as ra
            v, f, _ = ra.flatten_scene_host(*scene_parts())
            _maps[name] = (v, f)
        else:
            _maps[name] = fc.build_map(name)
    return _maps[name]


_records = {}


def records(name):
    """(record array [n_records, 16] uint32, n_faces, builder info) of the map, made once per process"""
    if name not in _records:
        import rmcl_amd as ra
        v, f = build_map(name)
        info, _, tris = ra.build_bvh_host(v, f)
        _records[name] = (tris, len(np.asarray(f).reshape(-1, 3)), info)
    return _records[name]


def ramp_cos():
    """the float n.z of the ramp's record (0.8 up to rounding)"""
    tris, _, _ = records("twofloor")
    nz = {int(r[15]): abs(float(r.view(F)[14])) for r in tris}
    assert nz[12] == nz[13]
    return F(nz[12])


def ramp_on():
    return dict(min_up_cos=ramp_cos())


def ramp_off():
    return dict(min_up_cos=np.nextafter(ramp_cos(), F(2)))


# name -> keyword arguments of surface_sample_ref.params; every (map, parameters) the byte comparison runs on
def parametrisations():
    return {
        "twofloor": ("twofloor", dict(height=0.2)),
        "twofloor_ramp_on": ("twofloor", dict(height=0.2, **ramp_on())),
        "twofloor_ramp_off": ("twofloor", dict(height=0.2, **ramp_off())),
        "twofloor_align": ("twofloor", dict(height=0.35, align=1, yaw_min=-1.0, yaw_max=2.5)),
        "twofloor_upper": ("twofloor", dict(region_min=(-1, -1, 2.5), region_max=(11, 11, 3.5), yaw_min=0.25, yaw_max=0.25)),
        "cadmix20k": ("cadmix20k", dict(min_up_cos=0.3, height=0.1, align=1)),
        "dupsoup": ("dupsoup", dict(min_up_cos=0.5, align=1)),
        "degcube": ("degcube", dict(min_up_cos=0.0, height=0.05)),
        "scene": ("scene", dict(height=0.2, align=1)),
        "strip1025": ("strip1025", dict()),
        "strip4097": ("strip4097", dict(align=1, height=1.0)),
        "strip4097_small": ("strip4097", dict(region_min=(-1, -1, -1), region_max=(np.inf, 1, 1))),   # without the large face: draws on every block
        "single": ("single", dict(height=0.5)),
        "vertical": ("vertical", dict(min_up_cos=0.0, align=1, height=0.25)),
    }


OUTSIDE = ("single", dict(region_min=(5, 5, -1), region_max=(6, 6, 2)))     # the only up-facing face is not inside: refused

_samplers = {}


def ref_sampler(key):
    """the restated sampler of a parametrisation, made once per process"""
    if key not in _samplers:
        name, kw = parametrisations()[key]
        tris, nf, _ = records(name)
        _samplers[key] = ssr.Sampler(tris, nf, ssr.params(**kw))
    return _samplers[key]


# which count runs on which parametrisation in the GPU byte comparison: every count on twofloor, one large and one odd elsewhere
def counts_of(key):
    return COUNTS if key in ("twofloor", "twofloor_align", "strip4097_small") else (257,)


BAD_PARAMS = (dict(min_up_cos=-0.1), dict(min_up_cos=1.5), dict(min_up_cos=np.nan), dict(height=np.inf), dict(height=np.nan),
              dict(region_min=(1, 0, 0), region_max=(0, 1, 1)), dict(region_min=(np.nan, 0, 0)), dict(region_max=(0, np.nan, 0)),
              dict(yaw_min=1.0, yaw_max=0.5), dict(yaw_min=-np.inf), dict(yaw_max=np.nan), dict(align=2), dict(align=-1))

# the recovery sequence: steady, a drop, recovery, reset (likelihood sums of n = 1000 particles)
RECOVERY_N = 1000
RECOVERY_SUMS = [800.0] * 6 + [80.0, 60.0, 50.0] + [400.0, 700.0, 800.0, 800.0]
RECOVERY_RESET_AFTER = 8           # the caller injected after this update
BAD_RECOVERY = (dict(alpha_slow=0.0), dict(alpha_slow=-0.1), dict(alpha_fast=1.5), dict(alpha_slow=0.2, alpha_fast=0.1),
                dict(alpha_slow=float("nan")), dict(p_max=-0.1), dict(p_max=1.1), dict(p_max=float("nan")))
