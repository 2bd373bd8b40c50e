"""Synthetic inputs of BASELINE.json's configs, seeded with PCG32 streams
(the reference's generator, src/core/rng.rs:46-93, vectorised over independent sequences).

  sphere_scene        C1: analytic sphere + point light, direct lighting
  check_sphere_scene  C0-like: scenes/check-sphere.pbrt's mirror sphere over a ground plane
  random_mesh_scene   C2 / C3: N random triangles in a box with a ceiling area light
  cornell_scene       C4: Cornell-style box
  glass_sphere_scene  a glass sphere and a glass cube in a Cornell-style box (= scenes/glass_sphere.pbrt)
  plastic_scene       a plastic floor and two plastic spheres in a Cornell-style box (= scenes/plastic_spheres.pbrt)
  substrate_scene     a substrate floor and two substrate spheres in a Cornell-style box (= scenes/substrate_spheres.pbrt)
  spot_scene          a plastic and a matte sphere in a Cornell-style box lit by two spot lights (= scenes/spot_cornell.pbrt)
  sphere_light_scene  the same box lit by two sphere lamps, with a plastic and a mirror sphere (= scenes/sphere_light_cornell.pbrt)
  projector_scene     the same box lit by a projection light that throws a slide onto the back wall and a goniometric light (DESIGN.md 3.23;
                      = scenes/projector_cornell.pbrt)
  envmap_scene        a matte ground, a glass and a mirror sphere under an environment map (= scenes/envmap_spheres.pbrt)
  icosphere_scene     C1 with its sphere tessellated, with or without shading normals
  smooth_mesh_scene   two octahedra with per-vertex normals over a flat ground (= scenes/smooth_mesh.pbrt)
"""
import numpy as np

from .api import GLASS, PLASTIC, SUBSTRATE, roughness_to_alpha, LIGHT_DISTANT, LIGHT_ENVMAP, LIGHT_INFINITE, LIGHT_POINT, MATTE, MIRROR, SceneData, look_at

MESH_SEED = 0x5EED0001

_MULT = np.uint64(0x5851F42D4C957F2D)
_DEFAULT_STATE = np.uint64(0x853C49E6748FEA9B)


class PcgStreams:
    """n independent PCG32 generators, one per sequence index (Rng::new(seq), rng.rs:46-59)."""

    def __init__(self, seqs):
        seqs = np.asarray(seqs, np.uint64)
        self.inc = (seqs << np.uint64(1)) | np.uint64(1)
        self.state = np.zeros_like(seqs)
        self.u32()
        with np.errstate(over="ignore"):
            self.state = self.state + _DEFAULT_STATE
        self.u32()

    def u32(self):  # rng.rs:62-76
        old = self.state
        with np.errstate(over="ignore"):
            self.state = old * _MULT + self.inc
        xs = (((old >> np.uint64(18)) ^ old) >> np.uint64(27)).astype(np.uint32)
        rot = (old >> np.uint64(59)).astype(np.uint32)
        return (xs >> rot) | (xs << ((~rot + np.uint32(1)) & np.uint32(31)))

    def uniform(self):  # rng.rs:91-93
        f = self.u32().astype(np.float32) * np.float32(2.3283064365386963e-10)
        return np.minimum(f, np.float32(1.0) - np.finfo(np.float32).eps)


def _mat(t, k, le=(0, 0, 0)):
    return [t, k[0], k[1], k[2], le[0], le[1], le[2]]


def _quad(p0, p1, p2, p3):
    """two triangles (p0 p1 p2), (p0 p2 p3)"""
    return [p0, p1, p2, p3], [[0, 1, 2], [0, 2, 3]]


def _camera(eye, look, up):
    return look_at(eye, look, up)[1]


def sphere_scene(xres=1024, yres=1024, crop=(0.0, 1.0, 0.0, 1.0)):
    """C1: sphere r=1 at the origin, matte Kd=.5; point light I=10 at (2,2,3); camera of
    scenes/check-sphere.pbrt:1-4."""
    return SceneData(
        materials=np.array([_mat(MATTE, (0.5, 0.5, 0.5))], np.float32),
        lights=np.array([[LIGHT_POINT, 2, 2, 3, 10, 10, 10]], np.float32),
        spheres=np.array([[0, 0, 0, 1, 0]], np.float32),
        cam_to_world=_camera((3, 4, 1.5), (0.5, 0.5, 0), (0, 0, 1)), fov=45.0, xres=xres, yres=yres, crop=crop,
    ).normalized()


def icosphere(level):
    """(P[n, 3] float64 on the unit sphere, idx[m, 3]) of an icosahedron subdivided `level` times, every face wound so that its normal
    points outwards: 20 x 4^level triangles"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    P = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    P = [np.array(p, np.float64) / np.linalg.norm(p) for p in P]
    F = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(int(level)):
        mid, G = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = P[a] + P[b]
                P.append(m / np.linalg.norm(m))
                mid[key] = len(P) - 1
            return mid[key]

        for a, b, c in F:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            G += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        F = G
    return np.array(P, np.float64), np.array(F, np.uint32)


def icosphere_scene(level=4, smooth=True, xres=1024, yres=1024, crop=(0.0, 1.0, 0.0, 1.0), centre=(0.0, 0.0, 0.0), radius=1.0):
    """C1's scene (sphere_scene's camera, light and material) with the sphere tessellated into 20 x 4^level triangles whose vertices lie on
    it.  smooth: every corner carries the normal p - c of its vertex -- deliberately not unit length (the radius is its length) --, else the
    scene has no normals and renders faceted."""
    U, F = icosphere(level)
    c = np.asarray(centre, np.float64)
    P = (c + radius * U).astype(np.float32)
    kw = {}
    if smooth:
        kw["tri_n"] = (P.astype(np.float64) - c)[F].reshape(-1, 9).astype(np.float32)
    return SceneData(
        P=P, idx=F, mat_id=np.zeros(len(F), np.uint16),
        materials=np.array([_mat(MATTE, (0.5, 0.5, 0.5))], np.float32),
        lights=np.array([[LIGHT_POINT, 2, 2, 3, 10, 10, 10]], np.float32),
        cam_to_world=_camera((3, 4, 1.5), (0.5, 0.5, 0), (0, 0, 1)), fov=45.0, xres=xres, yres=yres, crop=crop, **kw,
    ).normalized()


def smooth_mesh_scene(xres=128, yres=128, crop=(0.0, 1.0, 0.0, 1.0)):
    """The shading normals' scene, array for array what scenes/smooth_mesh.pbrt loads to: a flat matte ground z = 0 without
    normals (zero rows of `tri_n`) and two octahedra of radius 0.9 at (-1.1, 0, 1) and (1.1, 0, 1), a matte and a mirror one, whose
    corners carry their vertex's position about the centre as the normal; a point light and a constant sky."""
    GROUND, BALL, MIRROR_M = range(3)
    mats = [_mat(MATTE, (0.5, 0.48, 0.45)), _mat(MATTE, (0.7, 0.3, 0.25)), _mat(MIRROR, (0.9, 0.9, 0.9))]
    verts, tris = _quad((-6, -6, 0), (6, -6, 0), (6, 6, 0), (-6, 6, 0))
    P, I, M, N = [np.array(verts, np.float32)], [np.array(tris, np.uint32)], [GROUND, GROUND], [np.zeros((2, 9), np.float32)]
    octa = np.array([(.9, 0, 0), (-.9, 0, 0), (0, .9, 0), (0, -.9, 0), (0, 0, .9), (0, 0, -.9)], np.float32)
    faces = np.array([(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)], np.uint32)
    for centre, m in (((-1.1, 0, 1), BALL), ((1.1, 0, 1), MIRROR_M)):
        base = sum(len(p) for p in P)
        P.append(octa + np.array(centre, np.float32))  # (fp32, as the parser's Translate moves the vertices)
        I.append(faces + np.uint32(base))
        M += [m] * len(faces)
        N.append(octa[faces].reshape(-1, 9))
    return SceneData(
        P=np.concatenate(P), idx=np.concatenate(I), mat_id=np.array(M, np.uint16), materials=np.array(mats, np.float32),
        lights=np.array([[LIGHT_POINT, 2, -3, 5, 40, 38, 34], [LIGHT_INFINITE, 0, 0, 0, .3, .35, .4]], np.float32),
        tri_n=np.concatenate(N), cam_to_world=_camera((0, -5, 2.2), (0, 0, 0.8), (0, 0, 1)), fov=40.0, xres=xres, yres=yres, crop=crop,
    ).normalized()


def check_sphere_scene(xres=256, yres=256, crop=(0.0, 1.0, 0.0, 1.0)):
    """scenes/check-sphere.pbrt with the pieces this path covers: mirror sphere, matte ground
    quad at z=-1 (constant Kd .45 in place of the checkerboard texture, which is out of scope),
    constant infinite light (.4 .45 .5) and a distant light from (-30, 40, 100) (the file's
    blackbody 3000K x 1.5 replaced by its approximate RGB)."""
    verts, tris = _quad((-20, -20, -1), (20, -20, -1), (20, 20, -1), (-20, 20, -1))
    d = np.array([-30, 40, 100], np.float64)
    d = (d / np.linalg.norm(d)).astype(np.float32)
    return SceneData(
        P=np.array(verts, np.float32), idx=np.array(tris, np.uint32), mat_id=np.array([1, 1], np.uint16),
        materials=np.array([_mat(MIRROR, (0.9, 0.9, 0.9)), _mat(MATTE, (0.45, 0.45, 0.45))], np.float32),
        lights=np.array([[LIGHT_INFINITE, 0, 0, 0, 0.4, 0.45, 0.5],
                         [LIGHT_DISTANT, d[0], d[1], d[2], 1.5 * 1.0, 1.5 * 0.55, 1.5 * 0.25]], np.float32),
        spheres=np.array([[0, 0, 0, 1, 0]], np.float32),
        cam_to_world=_camera((3, 4, 1.5), (0.5, 0.5, 0), (0, 0, 1)), fov=45.0, xres=xres, yres=yres, crop=crop,
    ).normalized()


def random_mesh_scene(n_tris=100_000, xres=1024, yres=1024, crop=(0.0, 1.0, 0.0, 1.0), seed=MESH_SEED):
    """C2 / C3: n random triangles (centre ~ U[-1,1]^3, vertices centre + U[-s,s]^3, s = n^(-1/3))
    inside the box [-2,2]^3 (12 matte triangles, Kd .7) lit by a 1x1 ceiling area light at z=1.99
    (2 emissive triangles, Le 20, facing down).  Triangle i uses material i % 250: every fifth one
    is a mirror (Kr .9), the others matte with Kd ~ U[.2,.8]^3.  Camera at (0,-1.95,0) looking at the
    origin, up +z, fov 60."""
    n = int(n_tris)
    s = np.float32(float(n) ** (-1.0 / 3.0)) if n > 0 else np.float32(1)
    rng = PcgStreams(np.uint64(seed) + np.arange(n, dtype=np.uint64))
    centre = np.stack([rng.uniform() for _ in range(3)], axis=1) * np.float32(2) - np.float32(1)
    offs = np.stack([rng.uniform() for _ in range(9)], axis=1).reshape(n, 3, 3)
    offs = (offs * np.float32(2) - np.float32(1)) * s
    verts = (centre[:, None, :] + offs).astype(np.float32).reshape(-1, 3)
    idx = np.arange(3 * n, dtype=np.uint32).reshape(n, 3)
    mat_id = (np.arange(n) % 250).astype(np.uint16)
    mrng = PcgStreams(np.uint64(seed) + np.uint64(1 << 40) + np.arange(250, dtype=np.uint64))
    kd = np.stack([mrng.uniform() for _ in range(3)], axis=1) * np.float32(0.6) + np.float32(0.2)
    mats = [_mat(MIRROR, (0.9, 0.9, 0.9)) if i % 5 == 0 else _mat(MATTE, kd[i]) for i in range(250)]
    BOX, LIGHT = 250, 251
    mats.append(_mat(MATTE, (0.7, 0.7, 0.7)))
    mats.append(_mat(MATTE, (0.0, 0.0, 0.0), (20, 20, 20)))
    b = 2.0
    c = [(-b, -b, -b), (b, -b, -b), (b, b, -b), (-b, b, -b), (-b, -b, b), (b, -b, b), (b, b, b), (-b, b, b)]
    faces = [(0, 1, 2, 3), (4, 5, 6, 7), (0, 1, 5, 4), (3, 2, 6, 7), (0, 3, 7, 4), (1, 2, 6, 5)]
    extra_v, extra_i, extra_m = [], [], []
    for f in faces:
        base = 3 * n + len(extra_v)
        v, t = _quad(*[c[i] for i in f])
        extra_v += v
        extra_i += [[base + a for a in tri] for tri in t]
        extra_m += [BOX, BOX]
    base = 3 * n + len(extra_v)
    v, t = _quad((-0.5, -0.5, 1.99), (-0.5, 0.5, 1.99), (0.5, 0.5, 1.99), (0.5, -0.5, 1.99))  # normal -z
    extra_v += v
    extra_i += [[base + a for a in tri] for tri in t]
    extra_m += [LIGHT, LIGHT]
    return SceneData(
        P=np.concatenate([verts, np.array(extra_v, np.float32)]),
        idx=np.concatenate([idx, np.array(extra_i, np.uint32)]),
        mat_id=np.concatenate([mat_id, np.array(extra_m, np.uint16)]),
        materials=np.array(mats, np.float32),
        cam_to_world=_camera((0, -1.95, 0), (0, 0, 0), (0, 0, 1)), fov=60.0, xres=xres, yres=yres, crop=crop,
    ).normalized()


def cornell_scene(xres=4096, yres=4096, crop=(0.0, 1.0, 0.0, 1.0)):
    """C4: Cornell-style box [-1,1]^3 open towards the camera: white floor / ceiling / back wall, red
    left and green right walls, two white boxes, a 0.5 x 0.5 ceiling light with Le (17, 12, 4)."""
    WHITE, RED, GREEN, LIGHT = 0, 1, 2, 3
    mats = [_mat(MATTE, (0.73, 0.73, 0.73)), _mat(MATTE, (0.65, 0.05, 0.05)), _mat(MATTE, (0.12, 0.45, 0.15)),
            _mat(MATTE, (0, 0, 0), (17, 12, 4))]
    V, I, M = [], [], []

    def add(q, m):
        base = len(V)
        v, t = _quad(*q)
        V.extend(v)
        I.extend([[base + a for a in tri] for tri in t])
        M.extend([m, m])

    add(((-1, -1, -1), (1, -1, -1), (1, 1, -1), (-1, 1, -1)), WHITE)  # floor
    add(((-1, -1, 1), (-1, 1, 1), (1, 1, 1), (1, -1, 1)), WHITE)      # ceiling
    add(((-1, 1, -1), (1, 1, -1), (1, 1, 1), (-1, 1, 1)), WHITE)      # back wall (y = +1)
    add(((-1, -1, -1), (-1, 1, -1), (-1, 1, 1), (-1, -1, 1)), RED)    # left
    add(((1, -1, -1), (1, -1, 1), (1, 1, 1), (1, 1, -1)), GREEN)      # right
    add(((-0.25, -0.25, 0.999), (-0.25, 0.25, 0.999), (0.25, 0.25, 0.999), (0.25, -0.25, 0.999)), LIGHT)  # normal -z

    def box(cx, cy, hx, hy, z0, z1, ang):
        ca, sa = np.cos(ang), np.sin(ang)
        cor = [(cx + ca * dx - sa * dy, cy + sa * dx + ca * dy) for dx, dy in ((-hx, -hy), (hx, -hy), (hx, hy), (-hx, hy))]
        lo = [(x, y, z0) for x, y in cor]
        hi = [(x, y, z1) for x, y in cor]
        add((hi[0], hi[1], hi[2], hi[3]), WHITE)
        for k in range(4):
            add((lo[k], lo[(k + 1) % 4], hi[(k + 1) % 4], hi[k]), WHITE)

    box(-0.35, 0.3, 0.3, 0.3, -1.0, 0.2, 0.3)
    box(0.35, -0.25, 0.3, 0.3, -1.0, -0.4, -0.3)
    return SceneData(
        P=np.array(V, np.float32), idx=np.array(I, np.uint32), mat_id=np.array(M, np.uint16),
        materials=np.array(mats, np.float32),
        cam_to_world=_camera((0, -3.6, 0), (0, 0, 0), (0, 0, 1)), fov=40.0, xres=xres, yres=yres, crop=crop,
    ).normalized()


def glass_sphere_scene(xres=256, yres=256, crop=(0.0, 1.0, 0.0, 1.0), glass=True):
    """The glass material's scene, array for array what scenes/glass_sphere.pbrt loads to: the Cornell-style box
    [-1, 1]^3 open towards the camera (white floor / ceiling / back wall, red left and green right walls), a 1 x 1 ceiling emitter with Le
    (10, 9, 7), a glass triangle-mesh cube (12 triangles, eta 1.33, a greenish Kt) standing on the floor and a glass sphere (eta 1.5, Kr = Kt =
    1) hovering beside it.  `glass=False`: the same scene with the two glass materials replaced by mirrors (Kr = the glass's Kr): the
    throughput comparison of profiles/glass_vs_mirror.txt."""
    WHITE, RED, GREEN, LIGHT, CUBE, BALL = range(6)  # (numbered in the order the scene file's shapes first use them)
    mats = [_mat(MATTE, (0.73, 0.73, 0.73)), _mat(MATTE, (0.65, 0.05, 0.05)), _mat(MATTE, (0.12, 0.45, 0.15)), _mat(MATTE, (0, 0, 0), (10, 9, 7)),
            _mat(GLASS, (1, 1, 1), (0.8, 0.95, 0.85)), _mat(GLASS, (1, 1, 1), (1, 1, 1))]  # a glass row: (GLASS, Kr, Kt)
    eta = [1.5, 1.5, 1.5, 1.5, 1.33, 1.5]
    if not glass:
        mats[CUBE], mats[BALL] = _mat(MIRROR, (1, 1, 1)), _mat(MIRROR, (1, 1, 1))
    V, I, M = [], [], []

    def add(q, m):
        base = len(V)
        v, t = _quad(*q)
        V.extend(v)
        I.extend([[base + a for a in tri] for tri in t])
        M.extend([m, m])

    add(((-1, -1, -1), (1, -1, -1), (1, 1, -1), (-1, 1, -1)), WHITE)  # floor
    add(((-1, -1, 1), (-1, 1, 1), (1, 1, 1), (1, -1, 1)), WHITE)      # ceiling
    add(((-1, 1, -1), (1, 1, -1), (1, 1, 1), (-1, 1, 1)), WHITE)      # back wall (y = +1)
    add(((-1, -1, -1), (-1, 1, -1), (-1, 1, 1), (-1, -1, 1)), RED)    # left
    add(((1, -1, -1), (1, -1, 1), (1, 1, 1), (1, 1, -1)), GREEN)      # right
    add(((-0.5, -0.5, 0.999), (-0.5, 0.5, 0.999), (0.5, 0.5, 0.999), (0.5, -0.5, 0.999)), LIGHT)  # normal -z
    # the cube [-0.75, -0.15] x [-0.1, 0.5] x [-0.999, -0.399], every face wound so that its normal points outwards
    x0, x1, y0, y1, z0, z1 = -0.75, -0.15, -0.1, 0.5, -0.999, -0.399
    c = [(x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0), (x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)]
    for f in ((0, 3, 2, 1), (4, 5, 6, 7), (0, 1, 5, 4), (3, 7, 6, 2), (0, 4, 7, 3), (1, 2, 6, 5)):  # -z +z -y +y -x +x
        add(tuple(c[i] for i in f), CUBE)
    return SceneData(
        P=np.array(V, np.float32), idx=np.array(I, np.uint32), mat_id=np.array(M, np.uint16),
        materials=np.array(mats, np.float32), mat_eta=np.array(eta, np.float32),
        spheres=np.array([[0.4, -0.2, -0.45, 0.35, BALL]], np.float32),
        cam_to_world=_camera((0, -3.6, 0), (0, 0, 0), (0, 0, 1)), fov=40.0, xres=xres, yres=yres, crop=crop,
    ).normalized()


def plastic_scene(xres=256, yres=256, crop=(0.0, 1.0, 0.0, 1.0), plastic=True, light_scale=1.0, roughness=(0.2, 0.05, 0.4)):
    """The plastic material's scene, array for array what scenes/plastic_spheres.pbrt loads to: the Cornell-style box
    [-1, 1]^3 open towards the camera with a grey PLASTIC floor (roughness 0.2), white ceiling and back wall, red left and green right walls, a
    1 x 1 ceiling emitter with Le (10, 9, 7), and two plastic spheres of radius 0.35 standing on the floor: a blue one of roughness 0.05 and an
    orange one of roughness 0.4 (remapped roughnesses, pbrt-v3's default).  `plastic=False`: the same scene with every plastic material
    replaced by matte of the same Kd (a scene of matte materials alone).  `light_scale`: the emitter's side (its radiance grows by 1 /
    light_scale^2: the same power); `roughness`: of the floor and the two spheres."""
    FLOOR, WHITE, RED, GREEN, LIGHT, BLUE, ORANGE = range(7)  # (numbered in the order the scene file's shapes first use them)
    le = tuple(np.float32(v) / np.float32(light_scale * light_scale) for v in (10, 9, 7))
    mats = [_mat(PLASTIC, (0.4, 0.4, 0.4), (0.3, 0.3, 0.3)), _mat(MATTE, (0.73, 0.73, 0.73)), _mat(MATTE, (0.65, 0.05, 0.05)), _mat(MATTE, (0.12, 0.45, 0.15)),
            _mat(MATTE, (0, 0, 0), le), _mat(PLASTIC, (0.1, 0.2, 0.6), (0.3, 0.3, 0.3)), _mat(PLASTIC, (0.6, 0.3, 0.05), (0.25, 0.25, 0.25))]  # a plastic row: (PLASTIC, Kd, Ks)
    alpha = [1.5] * 7  # (mat_eta: the float beside a row; what a row that is neither glass nor plastic carries is not read)
    for m, r in zip((FLOOR, BLUE, ORANGE), roughness):
        alpha[m] = roughness_to_alpha(r)
    if not plastic:
        for m in (FLOOR, BLUE, ORANGE):
            mats[m] = _mat(MATTE, mats[m][1:4])
    V, I, M = [], [], []

    def add(q, m):
        base = len(V)
        v, t = _quad(*q)
        V.extend(v)
        I.extend([[base + a for a in tri] for tri in t])
        M.extend([m, m])

    h = 0.5 * light_scale
    add(((-1, -1, -1), (1, -1, -1), (1, 1, -1), (-1, 1, -1)), FLOOR)  # floor
    add(((-1, -1, 1), (-1, 1, 1), (1, 1, 1), (1, -1, 1)), WHITE)      # ceiling
    add(((-1, 1, -1), (1, 1, -1), (1, 1, 1), (-1, 1, 1)), WHITE)      # back wall (y = +1)
    add(((-1, -1, -1), (-1, 1, -1), (-1, 1, 1), (-1, -1, 1)), RED)    # left
    add(((1, -1, -1), (1, -1, 1), (1, 1, 1), (1, 1, -1)), GREEN)      # right
    add(((-h, -h, 0.999), (-h, h, 0.999), (h, h, 0.999), (h, -h, 0.999)), LIGHT)  # normal -z
    return SceneData(
        P=np.array(V, np.float32), idx=np.array(I, np.uint32), mat_id=np.array(M, np.uint16),
        materials=np.array(mats, np.float32), mat_eta=np.array(alpha if plastic else [], np.float32),
        spheres=np.array([[-0.45, 0.15, -0.65, 0.35, BLUE], [0.45, -0.2, -0.65, 0.35, ORANGE]], np.float32),
        cam_to_world=_camera((0, -3.6, 0), (0, 0, 0), (0, 0, 1)), fov=40.0, xres=xres, yres=yres, crop=crop,
    ).normalized()


def substrate_scene(xres=256, yres=256, crop=(0.0, 1.0, 0.0, 1.0), substrate=True):
    """The substrate material's scene, array for array what scenes/substrate_spheres.pbrt loads to: plastic_scene's box --
    [-1, 1]^3 open towards the camera, white ceiling and back wall, red left and green right walls, the 1 x 1 ceiling emitter with Le (10, 9,
    7) -- with a grey SUBSTRATE floor (Ks 0.2, roughness 0.2) and two substrate spheres of radius 0.35 standing on it: a sharp blue one (Ks
    0.5, roughness 0.05) and a broad orange one (Ks 0.5, the default; roughness 0.4).  `substrate=False`: the same scene with every substrate
    material replaced by matte of the same Kd."""
    from .api import substrate_material
    FLOOR, WHITE, RED, GREEN, LIGHT, BLUE, ORANGE = range(7)  # (numbered in the order the scene file's shapes first use them)
    coats = {FLOOR: substrate_material((0.4, 0.4, 0.4), (0.2, 0.2, 0.2), 0.2, 0.2), BLUE: substrate_material((0.1, 0.2, 0.6), (0.5, 0.5, 0.5), 0.05, 0.05),
             ORANGE: substrate_material((0.6, 0.3, 0.05), uroughness=0.4, vroughness=0.4)}
    mats = [None, _mat(MATTE, (0.73, 0.73, 0.73)), _mat(MATTE, (0.65, 0.05, 0.05)), _mat(MATTE, (0.12, 0.45, 0.15)), _mat(MATTE, (0, 0, 0), (10, 9, 7)), None, None]
    alpha = [1.5] * 7  # (mat_eta: the float beside a row; what a row that is neither glass, plastic nor substrate carries is not read)
    for m, (row, a) in coats.items():
        mats[m] = row if substrate else _mat(MATTE, row[1:4])
        alpha[m] = a
    V, I, M = [], [], []

    def add(q, m):
        base = len(V)
        v, t = _quad(*q)
        V.extend(v)
        I.extend([[base + a for a in tri] for tri in t])
        M.extend([m, m])

    add(((-1, -1, -1), (1, -1, -1), (1, 1, -1), (-1, 1, -1)), FLOOR)  # floor
    add(((-1, -1, 1), (-1, 1, 1), (1, 1, 1), (1, -1, 1)), WHITE)      # ceiling
    add(((-1, 1, -1), (1, 1, -1), (1, 1, 1), (-1, 1, 1)), WHITE)      # back wall (y = +1)
    add(((-1, -1, -1), (-1, 1, -1), (-1, 1, 1), (-1, -1, 1)), RED)    # left
    add(((1, -1, -1), (1, -1, 1), (1, 1, 1), (1, 1, -1)), GREEN)      # right
    add(((-0.5, -0.5, 0.999), (-0.5, 0.5, 0.999), (0.5, 0.5, 0.999), (0.5, -0.5, 0.999)), LIGHT)  # normal -z
    return SceneData(
        P=np.array(V, np.float32), idx=np.array(I, np.uint32), mat_id=np.array(M, np.uint16),
        materials=np.array(mats, np.float32), mat_eta=np.array(alpha if substrate else [], np.float32),
        spheres=np.array([[-0.45, 0.15, -0.65, 0.35, BLUE], [0.45, -0.2, -0.65, 0.35, ORANGE]], np.float32),
        cam_to_world=_camera((0, -3.6, 0), (0, 0, 0), (0, 0, 1)), fov=40.0, xres=xres, yres=yres, crop=crop,
    ).normalized()


def spot_scene(xres=256, yres=256, crop=(0.0, 1.0, 0.0, 1.0)):
    """The spot light's scene, array for array what scenes/spot_cornell.pbrt loads to: the Cornell-style box [-1, 1]^3 open
    towards the camera (white floor / ceiling / back wall, red left and green right walls) WITHOUT a ceiling emitter, a blue plastic sphere
    and an orange matte sphere of radius 0.35 standing on the floor, and two spot lights under the ceiling: a warm one of half angle 35
    degrees (the falloff over the outer 10) aimed at the floor in front of the matte sphere, and a cool one of half angle 20 degrees (the
    outer 6) aimed at the plastic sphere -- so a matte vertex and a plastic vertex both sample a spot light."""
    from .api import plastic_material, spot_light
    WHITE, RED, GREEN, BLUE, ORANGE = range(5)  # (numbered in the order the scene file's shapes first use them)
    blue, alpha = plastic_material((0.1, 0.2, 0.6), (0.3, 0.3, 0.3), 0.1)
    mats = [_mat(MATTE, (0.73, 0.73, 0.73)), _mat(MATTE, (0.65, 0.05, 0.05)), _mat(MATTE, (0.12, 0.45, 0.15)), blue, _mat(MATTE, (0.6, 0.3, 0.05))]
    V, I, M = [], [], []

    def add(q, m):
        base = len(V)
        v, t = _quad(*q)
        V.extend(v)
        I.extend([[base + a for a in tri] for tri in t])
        M.extend([m, m])

    add(((-1, -1, -1), (1, -1, -1), (1, 1, -1), (-1, 1, -1)), WHITE)  # floor
    add(((-1, -1, 1), (-1, 1, 1), (1, 1, 1), (1, -1, 1)), WHITE)      # ceiling
    add(((-1, 1, -1), (1, 1, -1), (1, 1, 1), (-1, 1, 1)), WHITE)      # back wall (y = +1)
    add(((-1, -1, -1), (-1, 1, -1), (-1, 1, 1), (-1, -1, 1)), RED)    # left
    add(((1, -1, -1), (1, -1, 1), (1, 1, 1), (1, 1, -1)), GREEN)      # right
    lights, cones = zip(spot_light((0.5, -0.3, 0.95), (0.4, -0.45, -1.0), (6.0, 5.5, 4.5), 35.0, 10.0),
                        spot_light((-0.7, -0.6, 0.9), (-0.45, 0.15, -0.65), (5.0, 5.0, 6.0), 20.0, 6.0))
    return SceneData(
        P=np.array(V, np.float32), idx=np.array(I, np.uint32), mat_id=np.array(M, np.uint16),
        materials=np.array(mats, np.float32), mat_eta=np.array([1.5, 1.5, 1.5, alpha, 1.5], np.float32),
        lights=np.array(lights, np.float32), spot_cones=np.array(cones, np.float32),
        spheres=np.array([[-0.45, 0.15, -0.65, 0.35, BLUE], [0.45, -0.2, -0.65, 0.35, ORANGE]], np.float32),
        cam_to_world=_camera((0, -3.6, 0), (0, 0, 0), (0, 0, 1)), fov=40.0, xres=xres, yres=yres, crop=crop,
    ).normalized()


def sphere_light_scene(xres=256, yres=256, crop=(0.0, 1.0, 0.0, 1.0)):
    """The sphere light's scene, array for array what scenes/sphere_light_cornell.pbrt loads to: spot_scene's box -- white
    floor, ceiling and back wall, red left and green right walls, no emitter quad in the ceiling -- lit by two sphere lamps: a warm one of
    radius 0.15 under the ceiling and a small cool one of radius 0.05 beside a blue plastic sphere; a mirror sphere shows both lamps.  A
    matte vertex and a plastic vertex both sample a sphere light, and a specular path sees the lamps through their material."""
    from .api import plastic_material, sphere_light
    WHITE, RED, GREEN, WARM, COOL, BLUE, CHROME = range(7)  # (numbered in the order the scene file's shapes first use them)
    blue, alpha = plastic_material((0.1, 0.2, 0.6), (0.3, 0.3, 0.3), 0.1)
    mats = [_mat(MATTE, (0.73, 0.73, 0.73)), _mat(MATTE, (0.65, 0.05, 0.05)), _mat(MATTE, (0.12, 0.45, 0.15)), _mat(MATTE, (0, 0, 0), (20, 16, 10)),
            _mat(MATTE, (0, 0, 0), (30, 40, 60)), blue, _mat(MIRROR, (0.9, 0.9, 0.9))]
    V, I, M = [], [], []

    def add(q, m):
        base = len(V)
        v, t = _quad(*q)
        V.extend(v)
        I.extend([[base + a for a in tri] for tri in t])
        M.extend([m, m])

    add(((-1, -1, -1), (1, -1, -1), (1, 1, -1), (-1, 1, -1)), WHITE)  # floor
    add(((-1, -1, 1), (-1, 1, 1), (1, 1, 1), (1, -1, 1)), WHITE)      # ceiling
    add(((-1, 1, -1), (1, 1, -1), (1, 1, 1), (-1, 1, 1)), WHITE)      # back wall (y = +1)
    add(((-1, -1, -1), (-1, 1, -1), (-1, 1, 1), (-1, -1, 1)), RED)    # left
    add(((1, -1, -1), (1, -1, 1), (1, 1, 1), (1, 1, -1)), GREEN)      # right
    sd = SceneData(
        P=np.array(V, np.float32), idx=np.array(I, np.uint32), mat_id=np.array(M, np.uint16),
        materials=np.array(mats, np.float32), mat_eta=np.array([1.5, 1.5, 1.5, 1.5, 1.5, alpha, 1.5], np.float32),
        spheres=np.array([[0.0, 0.0, 0.8, 0.15, WARM], [-0.05, -0.45, -0.6, 0.05, COOL], [-0.45, 0.15, -0.65, 0.35, BLUE], [0.45, -0.2, -0.65, 0.35, CHROME]], np.float32),
        cam_to_world=_camera((0, -3.6, 0), (0, 0, 0), (0, 0, 1)), fov=40.0, xres=xres, yres=yres, crop=crop,
    ).normalized()
    sd.lights = np.array([sphere_light(sd, 0), sphere_light(sd, 1)], np.float32)
    return sd


def procedural_slide(width=64, height=48):
    """The slide of the projection light's demo, (height, width, 3) float32, row 0 = the top: a white frame, eight colour
    bars over the upper two thirds and a black-and-white checker below.  Every channel is exactly 0 or 1, which an 8-bit PNG and its inverse
    gamma carry without rounding: what the scene file reads back is this array bit for bit."""
    y, x = np.mgrid[0:height, 0:width]
    bar = (x * 8) // width
    bars = np.stack([(bar & 4) == 0, (bar & 2) == 0, (bar & 1) == 0], -1)
    bars[bar == 7] = True  # (no black bar: white again)
    check = ((x * 16) // width + (y * 12) // height) % 2 == 0
    rgb = np.where((y * 3 < height * 2)[..., None], bars, check[..., None])
    frame = (x < 2) | (x >= width - 2) | (y < 2) | (y >= height - 2)
    return np.where(frame[..., None], True, rgb).astype(np.float32)


def procedural_gonio(width=32, height=16):
    """A small latitude-longitude intensity map for the goniometric light's demo, (height, width, 3) float32 with row 0 at the
    light's +y pole: three lobes around the equator that fade towards the poles, tinted warm on one side and cool on the other, nowhere
    below 0.05."""
    r, c = np.mgrid[0:height, 0:width].astype(np.float64)
    theta, phi = np.pi * (r + 0.5) / height, 2.0 * np.pi * (c + 0.5) / width
    lobes = (0.5 + 0.5 * np.cos(3.0 * phi)) * np.sin(theta) ** 2
    warm = 0.5 + 0.5 * np.cos(phi)
    rgb = np.stack([0.05 + 0.95 * lobes * (0.6 + 0.4 * warm), 0.05 + 0.85 * lobes, 0.05 + 0.95 * lobes * (1.0 - 0.4 * warm)], -1)
    return rgb.astype(np.float32)


def projector_scene(xres=256, yres=256, crop=(0.0, 1.0, 0.0, 1.0)):
    """The mapped lights' scene, array for array what scenes/projector_cornell.pbrt loads to: spot_scene's box and spheres
    WITHOUT its spot lights, a projection light in front of the box's opening that throws procedural_slide onto the back wall (it looks along
    the world's +y with +z up: the light's +x is the world's -x), and a goniometric light under the ceiling whose pole is the world's +z and
    whose map is procedural_gonio -- so a matte vertex and a plastic vertex both sample a mapped light of each kind."""
    from .api import WRAP_CLAMP, WRAP_REPEAT, goniometric_light, image_texture_row, plastic_material, projection_light
    sd = spot_scene(xres, yres, crop)
    slide, gonio = procedural_slide(), procedural_gonio()
    frame = [[-1, 0, 0], [0, 0, 1], [0, 1, 0]]  # world_to_light: the rows are the light's x, y, z axes in world space
    lights, maps = zip(projection_light((0.0, -0.95, 0.1), 1, (12.0, 12.0, 12.0), 40.0, slide.shape[1] / slide.shape[0], frame),
                       goniometric_light((0.3, 0.1, 0.8), 2, (2.5, 2.5, 2.5), frame))
    sd.lights, sd.light_maps = np.array(lights, np.float32), np.array(maps, np.float32)
    sd.spot_cones = np.zeros((0, 5), np.float32)
    sd.textures = np.array([image_texture_row(0, WRAP_CLAMP), image_texture_row(1, WRAP_REPEAT)], np.float32)
    sd.images = [slide, gonio]
    return sd.normalized()


def procedural_sky(width=64, height=32):
    """A latitude-longitude sky, (height, width, 3) float32 with row 0 at the zenith (+z of the light): a gradient from a blue zenith to a
    pale horizon, a dark ground below it, and a small sun -- radiance (600, 540, 420) in the texels whose centre lies within
    max(2 degrees, 0.75 texel heights) of the direction theta 50, phi 120 degrees.  tools/make_sky_pfm.py writes the 64 x 32 one as
    scenes/sky_small.pfm."""
    theta = (np.arange(height, dtype=np.float64)[:, None] + 0.5) * np.pi / height
    phi = (np.arange(width, dtype=np.float64)[None, :] + 0.5) * 2.0 * np.pi / width
    ct = np.cos(theta) + 0.0 * phi
    up = np.clip(ct, 0.0, 1.0)[..., None] ** 0.6
    sky = (1.0 - up) * np.array([0.85, 0.88, 0.95]) + up * np.array([0.22, 0.42, 0.90])
    sky = np.where(ct[..., None] >= 0.0, sky, np.array([0.16, 0.13, 0.10]))
    ts, ps = np.radians(50.0), np.radians(120.0)
    cos_sun = np.sin(theta) * np.sin(ts) * np.cos(phi - ps) + ct * np.cos(ts)
    radius = max(np.radians(2.0), 0.75 * np.pi / height)
    sky = np.where((cos_sun >= np.cos(radius))[..., None], np.array([600.0, 540.0, 420.0]), sky)
    return np.ascontiguousarray(sky, np.float32)


def envmap_scene(xres=256, yres=256, crop=(0.0, 1.0, 0.0, 1.0), sky=None, world_to_light=None, factor=(1.0, 1.0, 1.0), constant=False):
    """The environment map's scene, with the defaults array for array what scenes/envmap_spheres.pbrt loads to: a matte
    ground z = 0 (Kd .5 .48 .45), a glass sphere (eta 1.5) and a mirror sphere (Kr .9) of radius 1 standing on it, under the sky `sky`
    ((H, W, 3), default procedural_sky(64, 32)) rotated by `world_to_light` and scaled by `factor`.  `constant=True`: the same scene under
    a constant infinite light of the map's solid-angle mean radiance x factor (tools/envmap_cost.py's comparison)."""
    GROUND, GLASS_M, MIRROR_M = range(3)
    mats = [_mat(MATTE, (0.5, 0.48, 0.45)), _mat(GLASS, (1, 1, 1), (1, 1, 1)), _mat(MIRROR, (0.9, 0.9, 0.9))]
    verts, tris = _quad((-20, -20, 0), (20, -20, 0), (20, 20, 0), (-20, 20, 0))
    sky = procedural_sky() if sky is None else np.ascontiguousarray(sky, np.float32)
    kw = {}
    if constant:
        w = np.sin((np.arange(sky.shape[0]) + 0.5) * np.pi / sky.shape[0])[:, None, None]
        mean = (sky.astype(np.float64) * w).sum(axis=(0, 1)) / (w.sum() * sky.shape[1])
        lights = [[LIGHT_INFINITE, 0, 0, 0, *(mean * np.asarray(factor, np.float64))]]
    else:
        lights = [[LIGHT_ENVMAP, 0, 0, 0, *factor]]
        kw = dict(envmap=sky, envmap_world_to_light=np.eye(3, dtype=np.float32) if world_to_light is None else world_to_light)
    return SceneData(
        P=np.array(verts, np.float32), idx=np.array(tris, np.uint32), mat_id=np.array([GROUND, GROUND], np.uint16),
        materials=np.array(mats, np.float32), mat_eta=np.array([1.5, 1.5, 1.5], np.float32), lights=np.array(lights, np.float32),
        spheres=np.array([[-1.15, 0, 1, 1, GLASS_M], [1.15, 0, 1, 1, MIRROR_M]], np.float32),
        cam_to_world=_camera((0, -7, 2.6), (0, 0, 0.9), (0, 0, 1)), fov=40.0, xres=xres, yres=yres, crop=crop, **kw,
    ).normalized()


def procedural_planks(width=64, height=64):
    """A generated pattern for the image-texture demos, (height, width, 3) float32 in [0, 1], row 0 = the top: four planks
    with a darker joint between them, a grain that runs along each, and one knot -- nothing that a constant or a checkerboard could be."""
    y, x = np.mgrid[0:height, 0:width].astype(np.float64)
    u, v = (x + 0.5) / width, (y + 0.5) / height
    plank = np.floor(v * 4.0)
    grain = 0.5 + 0.5 * np.sin(2.0 * np.pi * (v * 24.0 + 0.35 * np.sin(2.0 * np.pi * (u * 2.0 + plank * 0.37))))
    tone = 0.55 + 0.12 * np.sin(plank * 2.1 + 0.4) + 0.18 * grain
    knot = np.exp(-(((u - 0.3) / 0.06) ** 2 + ((v - 0.62) / 0.04) ** 2))
    tone = tone * (1.0 - 0.6 * knot)
    joint = np.minimum(v * 4.0 - plank, 1.0 - (v * 4.0 - plank)) < 0.04
    tone = np.where(joint, 0.18, tone)
    rgb = np.stack([tone * 0.95, tone * 0.62, tone * 0.34], -1)
    return np.clip(rgb, 0.0, 1.0).astype(np.float32)


def write_demo_textures(directory):
    """scenes/textures/planks.png, the image scenes/textured_cornell.pbrt names: procedural_planks through the library's own PNG writer (the build calls this,
    build.py ensure_demo_textures: the file is a build product); and slide.png and gonio.pfm, which scenes/projector_cornell.pbrt names
    (DESIGN.md 3.23): procedural_slide and procedural_gonio"""
    import os

    from .api import write_image
    os.makedirs(directory, exist_ok=True)
    write_image(os.path.join(directory, "planks.png"), procedural_planks())
    write_image(os.path.join(directory, "slide.png"), procedural_slide())
    write_image(os.path.join(directory, "gonio.pfm"), procedural_gonio())


def image_plane_scene(res=256, image=None, wrap="repeat", filter="bilinear", mapping=(3.0, 3.0, 0.0, 0.0)):
    """A matte plane z = 0 whose Kd is an image under a distant light and a dim sky, seen from above at an angle: the
    quad's corner (u, v) are (0,0) (1,0) (1,1) (0,1), the image (default: procedural_planks) repeats three times either way."""
    from .api import image_texture_row
    image = procedural_planks() if image is None else image
    v, t = _quad((-4, -4, 0), (4, -4, 0), (4, 4, 0), (-4, 4, 0))
    return SceneData(
        P=np.array(v, np.float32), idx=np.array(t, np.uint32), mat_id=np.zeros(2, np.uint16), materials=np.array([_mat(MATTE, (0.5, 0.5, 0.5))], np.float32),
        lights=np.array([[LIGHT_DISTANT, 0.3, -0.2, 0.9327379, 3.0, 3.0, 3.0], [LIGHT_INFINITE, 0, 0, 0, 0.2, 0.25, 0.3]], np.float32),
        mat_tex=np.array([1], np.uint32), textures=np.array([image_texture_row(0, wrap, filter, mapping)], np.float32), images=[image],
        tri_uv=np.array([[0, 0, 1, 0, 1, 1], [0, 0, 1, 1, 0, 1]], np.float32),
        cam_to_world=_camera((0.5, -6.0, 4.0), (0, 0, 0), (0, 0, 1)), fov=40.0, xres=res, yres=res).normalized()


def textured_cornell_scene(xres=256, yres=256, crop=(0.0, 1.0, 0.0, 1.0), image=None):
    """cornell_scene with a plank floor and back wall: their Kd is an image (default: procedural_planks as linear texels --
    what scenes/textured_cornell.pbrt reads back from its PNG but for the 8-bit rounding), repeated twice across each; every quad carries
    the corner (u, v) (0,0) (1,0) (1,1) (0,1)."""
    from .api import image_texture_row
    sd = cornell_scene(xres, yres, crop)
    if image is None:
        image = procedural_planks()
    sd.materials = np.concatenate([sd.materials, [_mat(MATTE, tuple(image.astype(np.float64).mean((0, 1))))]]).astype(np.float32)
    sd.mat_id = sd.mat_id.copy()
    sd.mat_id[0:2] = sd.mat_id[4:6] = len(sd.materials) - 1  # floor, back wall
    sd.mat_tex = np.array([0] * (len(sd.materials) - 1) + [1], np.uint32)
    sd.textures = np.array([image_texture_row(0, "repeat", "bilinear", (2.0, 2.0, 0.0, 0.0))], np.float32)
    sd.images = [image]
    sd.tri_uv = np.tile(np.array([[0, 0, 1, 0, 1, 1], [0, 0, 1, 1, 0, 1]], np.float32), (len(sd.idx) // 2, 1))
    return sd.normalized()


def big_mesh_scene(xres=2048, yres=2048, crop=(0.0, 1.0, 0.0, 1.0), n_tris=12_000_000):
    """The OUT-OF-CACHE workload of bench.py (`--workload big`): the C2 / C3 scene with 12M triangles -- 0.31 GB of
    quantised nodes + 0.58 GB of triangle records, well past the 256 MiB Infinity Cache -- the one regime in which HBM
    bandwidth is a real roof for this path."""
    return random_mesh_scene(n_tris, xres, yres, crop=crop)
