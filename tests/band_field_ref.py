"""The banded distance field (include/rmclhip.h, BANDED DISTANCE FIELD) restated in numpy: the logical lattice and its bricks, the
three arrays cut out of a dense lattice (table, coarse lattice, stored bricks) and the lookup, every operation in float32 and in the
header's order.  The dense field's restatement is field_ref.  Not a test module.
"""
import numpy as np

import field_ref as fr

F = fr.F
FAR = 0xFFFFFFFF
EDGE = 8
BRICK_NODES = 729
REACH_FACTOR = F(6.9282032)          # 4 sqrt(3), as the header writes it
MAX_AXIS_CELLS = 1 << 20


def layout(bbox_min, bbox_max, cell=0.0, margin=0.0, band=0.5):
    """rmclhip_band_field_layout_host: (logical, bricks).  logical is field_ref.layout's dict (no cap on the nodes) with bytes 0;
    bricks is dict(nb, brick_edge, n_bricks, n_stored, n_coarse, band, reach, bytes) with n_stored and bytes 0"""
    logical = fr.layout(bbox_min, bbox_max, cell, margin)
    logical["bytes"] = 0
    n = logical["n"]
    nb = tuple((n[k] - 1 + EDGE - 1) // EDGE for k in range(3))
    band = F(band)
    bricks = dict(nb=nb, brick_edge=EDGE, n_bricks=nb[0] * nb[1] * nb[2], n_stored=0,
                  n_coarse=(nb[0] + 1) * (nb[1] + 1) * (nb[2] + 1), band=band, reach=F(band + REACH_FACTOR * logical["cell"]), bytes=0)
    return logical, bricks


def same_layout(ref, got):
    """ref: (logical, bricks) of this module, got: (FieldInfo.as_dict(), BandFieldInfo.as_dict()) -- equal to the bit"""
    (rl, rb), (gl, gb) = ref, got
    fa = np.array([rb["band"], rb["reach"]], F)
    fb = np.array([gb["band"], gb["reach"]], F)
    return fr.same_layout(rl, gl) and tuple(rb["nb"]) == tuple(gb["nb"]) and fa.tobytes() == fb.tobytes() and \
        all(int(rb[k]) == int(gb[k]) for k in ("brick_edge", "n_bricks", "n_stored", "n_coarse", "bytes"))


def coarse_indices(n, nb):
    """per axis, the logical node of every coarse node: min(8 c, n - 1)"""
    return [np.minimum(EDGE * np.arange(nb[k] + 1), n[k] - 1) for k in range(3)]


def build(logical, bricks, lattice):
    """the three arrays of the banded field whose logical lattice holds `lattice` ([n_z, n_y, n_x], NaN allowed):
    dict(table uint32 [nb_z, nb_y, nb_x], coarse [nb_z + 1, nb_y + 1, nb_x + 1], bricks [n_stored, 9, 9, 9], n_stored, bytes)"""
    n = fr.info_f32(logical)["n"]
    nb = tuple(int(x) for x in bricks["nb"])
    lat = np.asarray(lattice, F).reshape(n[2], n[1], n[0])
    cx, cy, cz = coarse_indices(n, nb)
    coarse = lat[np.ix_(cz, cy, cx)].astype(F)
    reach = F(bricks["reach"])
    corners = np.stack([coarse[dz:dz + nb[2], dy:dy + nb[1], dx:dx + nb[0]] for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)], 0)
    with np.errstate(all="ignore"):
        stored = ~(corners > reach).all(axis=0)            # some corner <= reach, or NaN
    table = np.full(nb[0] * nb[1] * nb[2], FAR, np.uint32)
    flat = stored.reshape(-1)                               # brick order: x fastest
    table[flat] = np.arange(int(flat.sum()), dtype=np.uint32)
    n_stored = int(flat.sum())
    padded = np.full((EDGE * nb[2] + 1, EDGE * nb[1] + 1, EDGE * nb[0] + 1), np.nan, F)
    padded[:n[2], :n[1], :n[0]] = lat
    out = np.zeros((n_stored, 9, 9, 9), F)
    for s, b in enumerate(np.flatnonzero(flat)):
        bx, by, bz = b % nb[0], (b // nb[0]) % nb[1], b // (nb[0] * nb[1])
        out[s] = padded[EDGE * bz:EDGE * bz + 9, EDGE * by:EDGE * by + 9, EDGE * bx:EDGE * bx + 9]
    nbytes = 4 * (table.size + coarse.size + out.size)
    return dict(table=table.reshape(nb[2], nb[1], nb[0]), coarse=coarse, bricks=out, n_stored=n_stored, bytes=nbytes)


def locate(logical, points):
    """the dense lookup's first half at finite points: (i [m, 3] int64, f [m, 3], c [m, 3], off [m, 3], clamped [m])"""
    info = fr.info_f32(logical)
    n = info["n"]
    P = np.asarray(points, F).reshape(-1, 3)
    idx, frac, cc, off = [], [], [], []
    clamped = np.zeros(len(P), bool)
    with np.errstate(all="ignore"):
        for k in range(3):
            top = F(n[k] - 1)
            u = (P[:, k] - info["origin"][k]) * info["inv_cell"]
            c = np.minimum(np.maximum(u, F(0)), top)
            i = np.minimum(np.floor(c).astype(np.int64), n[k] - 2)
            out = (u < 0) | (u > top)
            off.append(np.where(out, P[:, k] - (info["origin"][k] + c * info["cell"]), F(0)).astype(F))
            idx.append(i)
            frac.append((c - i.astype(F)).astype(F))
            cc.append(c.astype(F))
            clamped |= out
    return np.stack(idx, -1), np.stack(frac, -1), np.stack(cc, -1), np.stack(off, -1), clamped


def stored_mask(logical, bricks, table, points):
    """per point: its cell's brick is STORED (False for a point that is not finite)"""
    P = np.asarray(points, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        fin = (np.abs(P) <= fr.FLT_MAX).all(axis=1)
    i = locate(logical, np.where(fin[:, None], P, F(0)))[0]
    b = i >> 3
    return fin & (np.asarray(table)[b[:, 2], b[:, 1], b[:, 0]] != FAR)


def lookup(logical, bricks, arrays, points):
    """the banded lookup at points [m, 3]: float32 [m]"""
    info = fr.info_f32(logical)
    n = info["n"]
    table, coarse, fine = np.asarray(arrays["table"]), np.asarray(arrays["coarse"], F), np.asarray(arrays["bricks"], F)
    P = np.asarray(points, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        fin = (np.abs(P) <= fr.FLT_MAX).all(axis=1)
        Q = np.where(fin[:, None], P, F(0))
        i, f, c, off, clamped = locate(logical, Q)
        b = i >> 3
        s = table[b[:, 2], b[:, 1], b[:, 0]]
        st = s != FAR
        l = i & 7
        v = np.zeros((len(P), 2, 2, 2), F)
        fr_ = f.copy()
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    if len(fine):
                        near = fine[np.where(st, s, 0), l[:, 2] + dz, l[:, 1] + dy, l[:, 0] + dx]
                    else:
                        near = np.zeros(len(P), F)
                    far = coarse[b[:, 2] + dz, b[:, 1] + dy, b[:, 0] + dx]
                    v[:, dz, dy, dx] = np.where(st, near, far)
        for k in range(3):
            e = np.minimum(EDGE, (n[k] - 1) - EDGE * b[:, k])
            Fk = ((c[:, k] - (EDGE * b[:, k]).astype(F)) / e.astype(F)).astype(F)
            fr_[:, k] = np.where(st, f[:, k], Fk)

        def lerp(a, bb, t):
            return (a + t * (bb - a)).astype(F)

        fx, fy, fz = fr_[:, 0], fr_[:, 1], fr_[:, 2]
        x00, x10 = lerp(v[:, 0, 0, 0], v[:, 0, 0, 1], fx), lerp(v[:, 0, 1, 0], v[:, 0, 1, 1], fx)
        x01, x11 = lerp(v[:, 1, 0, 0], v[:, 1, 0, 1], fx), lerp(v[:, 1, 1, 0], v[:, 1, 1, 1], fx)
        d = lerp(lerp(x00, x10, fy), lerp(x01, x11, fy), fz)
        outside = (d + np.sqrt((off[:, 0] * off[:, 0] + off[:, 1] * off[:, 1]) + off[:, 2] * off[:, 2])).astype(F)
        res = np.where(clamped, outside, d)
        return np.where(fin, res, F(np.nan)).astype(F)


# ---- the maps the tests share: the smallest that have a FAR, a STORED and (where it says so) a ragged brick ----
def cube_mesh(half=2.0):
    """(vertices [8, 3], faces [12, 3]): the six walls of a cube of side 2 * half about the origin"""
    h = half
    V = np.array([[x, y, z] for z in (-h, h) for y in (-h, h) for x in (-h, h)], F)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    Fc = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.uint32)
    return V, Fc


def quad_mesh(side=6.0):
    """a single flat quad in z = 0, its diagonals along x and y: the z axis of its field has n = 2, and the corners of its box are
    far from it"""
    h = side / 2
    V = np.array([[-h, 0, 0], [0, -h, 0], [h, 0, 0], [0, h, 0]], F)
    return V, np.array([[0, 1, 2], [0, 2, 3]], np.uint32)


def walls_mesh(lx=100.0, ly=100.0, h=3.0):
    """four wall quads, no floor: a building's outline a dense field at 0.05 m is refused for"""
    V = np.array([[0, 0, 0], [lx, 0, 0], [lx, ly, 0], [0, ly, 0], [0, 0, h], [lx, 0, h], [lx, ly, h], [0, ly, h]], F)
    quads = [(0, 1, 5, 4), (1, 2, 6, 5), (2, 3, 7, 6), (3, 0, 4, 7)]
    return V, np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.uint32)


def query_points(logical, seed=5, n_random=400):
    """(points [m, 3] float32, kinds [m]): random points inside the lattice, points exactly on brick faces (u a multiple of 8 on one,
    two and three axes), the top node and points on the top faces, points outside on one, two and three axes, and points with a NaN
    or an infinite component"""
    info = fr.info_f32(logical)
    n, o, cell = info["n"], np.array(info["origin"], F), info["cell"]
    rng = np.random.RandomState(seed)
    top = np.array([n[k] - 1 for k in range(3)], np.float64)
    pts, kinds = [], []

    def add(u, kind):
        u = np.atleast_2d(np.asarray(u, np.float64))
        pts.append((o + u.astype(F) * cell).astype(F))
        kinds.extend([kind] * len(u))

    add(rng.uniform(0, 1, (n_random, 3)) * top, "inside")
    for axes in ((0,), (1,), (2,), (0, 1), (1, 2), (0, 1, 2)):
        u = rng.uniform(0, 1, (40, 3)) * top
        for k in axes:
            u[:, k] = np.minimum(8 * rng.randint(0, (n[k] - 1) // 8 + 1, 40), n[k] - 1)
        add(u, "face%d" % len(axes))
    add(top, "top")
    for k in range(3):
        u = rng.uniform(0, 1, (10, 3)) * top
        u[:, k] = top[k]
        add(u, "top")
    for axes in ((0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2)):
        u = rng.uniform(0, 1, (30, 3)) * top
        for k in axes:
            u[:, k] = np.where(rng.randint(0, 2, 30) == 0, -rng.uniform(0.01, 9, 30), top[k] + rng.uniform(0.01, 9, 30))
        add(u, "outside%d" % len(axes))
    centre = (o + (top / 2).astype(F) * cell).astype(F)
    for k in range(3):
        for bad in (np.nan, np.inf, -np.inf):
            p = centre.copy()
            p[k] = bad
            pts.append(p[None])
            kinds.append("special")
    return np.concatenate(pts).astype(F), np.array(kinds)


def build_example(tmp_path):
    """examples/band_field_cpp_example.cpp compiled with plain g++ against the C ABI: the executable's path"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    source = "band_field_cpp_example.cpp"
    exe = str(tmp_path / source.replace(".cpp", ""))
    libdir = os.path.join(root, "rmcl_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "examples", source), "-L" + libdir, "-lrmclhip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib",
                           "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


# name: (mesh function, cell, margin, band)
CASES = {
    "cube": (cube_mesh, 0.1, 0.0, 0.05),          # 41^3 nodes, 5 bricks per axis, the centre brick FAR
    "cube_ragged": (cube_mesh, 0.1, 0.15, 0.05),  # 44^3 nodes: 6 bricks per axis, the last of 3 cells
    "quad": (quad_mesh, 0.1, 0.0, 0.05),          # n_z = 2: one brick of one cell along z
    "cube_pow2": (cube_mesh, 0.125, 0.0, 0.05),   # 33^3 nodes and every u exact: points on brick faces are on them to the bit
}
RAGGED = ("cube_ragged", "quad")


def case(name):
    """(vertices, faces, logical, bricks) of a named case"""
    mesh, cell, margin, band = CASES[name]
    v, f = mesh()
    logical, bricks = layout(v.min(axis=0), v.max(axis=0), cell, margin, band)
    return v, f, logical, bricks


def is_ragged(logical):
    return any((logical["n"][k] - 1) % EDGE != 0 for k in range(3))
