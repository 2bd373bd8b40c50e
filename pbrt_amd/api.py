"""Host-side mirror of the render call: what `PbrtAPI::world_end` (reference src/core/api.rs:432-473)
would do with its RenderOptions (api.rs:201-224) -- build the scene on the device and render it.

Everything that computes goes through the C ABI of include/pbrt_hip.h into the HIP kernels.
"""
import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from ._lib import EnvMap, ImageTexture, Light, LightMap, Material, Normals, PixelFilter, RenderDesc, SceneDesc, Sphere, SpotCone, Stats, Texture, check, lib

MATTE, MIRROR, GLASS = 0, 1, 2  # PBRT_HIP_MATERIAL_*; GLASS: DESIGN.md 3.16
PLASTIC = 3  # PBRT_HIP_MATERIAL_PLASTIC: DESIGN.md 3.21
SUBSTRATE = 4  # PBRT_HIP_MATERIAL_SUBSTRATE: DESIGN.md 3.24
LIGHT_POINT, LIGHT_DISTANT, LIGHT_INFINITE = 0, 1, 2
LIGHT_ENVMAP = 3  # PBRT_HIP_LIGHT_ENVMAP: the infinite light with an environment map
LIGHT_SPOT = 5  # PBRT_HIP_LIGHT_SPOT: a point light inside a cone with a smooth edge; 4 is no light type
LIGHT_MAPPED = 6  # PBRT_HIP_LIGHT_MAPPED: a point light times an image looked up in the direction from the light; 7 is no light type
LIGHT_MAP_PROJECTION, LIGHT_MAP_GONIOMETRIC = 0, 1  # PBRT_HIP_LIGHT_MAP_*: a light map's kind
LIGHT_SPHERE = 8  # PBRT_HIP_LIGHT_SPHERE: a sphere of the scene as an area light, sampled by solid angle
INTEGRATOR_PATH, INTEGRATOR_DIRECT, INTEGRATOR_PATH_MIS = 0, 1, 2  # 2: the path integrator with MIS
FILTER_TRIANGLE, FILTER_GAUSSIAN, FILTER_MITCHELL, FILTER_SINC = 1, 2, 3, 4  # PBRT_HIP_FILTER_*: the weighted pixel filters
FILTER_KINDS = {"triangle": FILTER_TRIANGLE, "gaussian": FILTER_GAUSSIAN, "mitchell": FILTER_MITCHELL, "sinc": FILTER_SINC}
FILTER_DEFAULT_PARAMS = {FILTER_TRIANGLE: (0.0, 0.0), FILTER_GAUSSIAN: (2.0, 0.0), FILTER_MITCHELL: (1.0 / 3.0, 1.0 / 3.0), FILTER_SINC: (3.0, 0.0)}  # pbrt-v3's
TEXTURE_CHECKER, TEXTURE_IMAGE = 0, 4  # the types of a `textures` row a matte Kd can name; 4: PBRT_HIP_TEXTURE_IMAGE
WRAP_REPEAT, WRAP_CLAMP, WRAP_BLACK = 0, 1, 2  # PBRT_HIP_WRAP_*
WRAPS = {"repeat": WRAP_REPEAT, "clamp": WRAP_CLAMP, "black": WRAP_BLACK}
TEXFILTER_POINT, TEXFILTER_BILINEAR = 0, 1  # PBRT_HIP_TEXFILTER_*
TEXFILTERS = {"point": TEXFILTER_POINT, "bilinear": TEXFILTER_BILINEAR}
FLAG_COUNTERS = 1
FLAG_WALK_COUNTERS = 2
SCENE_GPU_BUILD = 1  # pbrt_hip_scene_create_ex flags
SCENE_OPTIMIZED_TREE = 2
SCENE_PLAIN_TREE = 4
SCENE_HOST_BUILD = 8
BUILDERS = {"host": SCENE_HOST_BUILD, "gpu": SCENE_GPU_BUILD, "gpu-plain": SCENE_GPU_BUILD | SCENE_PLAIN_TREE, "host-optimized": SCENE_OPTIMIZED_TREE}


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _u32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


@dataclass
class SceneData:
    """Plain arrays describing a scene: RenderOptions + the geometry the reference never stores
    (api.rs:220-223).  `materials` rows: (type, kr, kg, kb, ler, leg, leb); `lights` rows:
    (type, px, py, pz, cr, cg, cb); `spheres` rows: (cx, cy, cz, r, material).  Textured materials: `mat_tex[i]` =
    0 or 1 + the row of `textures` that is material i's Kd, `textures` rows: (type 0 = checkerboard, tex1 rgb, tex2 rgb, su, sv, du,
    dv), `tri_uv` rows: (u0, v0, u1, v1, u2, v2) per triangle (needed when a triangle's material is textured).  Glass:
    a `materials` row (GLASS, Kr rgb, Kt rgb) -- a glass surface does not emit -- and `mat_eta[i]` = its index of refraction (an empty
    `mat_eta` = 1.5 for every glass row; the entries of other rows are not read).  Plastic: a `materials` row (PLASTIC, Kd rgb,
    Ks rgb) and `mat_eta[i]` = its alpha, the float that rides where glass keeps eta (plastic_material makes the pair).  Substrate: a row (SUBSTRATE, Kd rgb, Ks rgb) and its alpha likewise (substrate_material).  An environment map: a `lights` row
    (LIGHT_ENVMAP, 0, 0, 0, c rgb) -- c the factor on the texels -- and `envmap` = its (H, W, 3) texels, row 0 = the light's +z, with
    `envmap_world_to_light` = the 3 x 3 rotation; the record travels in a slot appended to the texture table (fill_desc).  Shading normals
    (DESIGN.md 3.18): `tri_n` rows: the normals of a triangle's three corners (n0 xyz, n1 xyz, n2 xyz), world space, any length, zeros = the
    triangle has none; empty = the scene has none.  Its record travels in a slot of its own behind the checkerboards and the map.  A weighted
    pixel filter: `pixel_filter` = None (the box) or (kind, param0, param1) -- kind a name or number of FILTER_KINDS, the
    parameters alpha / B, C / tau (omitted ones: pbrt-v3's defaults); its record travels in a slot of its own too, and a render's
    filter_width is then that filter's radii (0 = the kind's default).  Image textures: `images` = a list of (H, W, 3) float32
    arrays, row 0 = the image's top, and a `textures` row (TEXTURE_IMAGE, image index, wrap, filter, 0, 0, 0, su, sv, du, dv) -- WRAP_*,
    TEXFILTER_* --, which fill_desc turns into the pbrt_hip_image_texture record of the same slot (image_texture_row makes one).  Spot lights
    (DESIGN.md 3.22): a `lights` row (LIGHT_SPOT, position, I rgb) and `spot_cones` rows (axis xyz -- unit, from the light into the cone --,
    cos_total, cos_start), the k-th row the cone of the k-th LIGHT_SPOT row (spot_light makes the pair); each cone travels in a slot of its own
    behind the filter's and before the normals'.  Mapped lights: a `lights` row (LIGHT_MAPPED, position, I rgb) and `light_maps`
    rows of 14 (kind, the 1-based number of a TEXTURE_IMAGE row of `textures`, world_to_light[9] row-major, inv_tan, sx, sy), the k-th row the
    record of the k-th LIGHT_MAPPED row (projection_light / goniometric_light make the pair); each record travels in a slot of its own behind
    the cones.  Sphere lights: a `lights` row (LIGHT_SPHERE, k, 0, 0, L rgb), k the 0-based row of `spheres` it names and L the
    le of that sphere's material (sphere_light makes the row)."""
    P: np.ndarray = field(default_factory=lambda: np.zeros((0, 3), np.float32))
    idx: np.ndarray = field(default_factory=lambda: np.zeros((0, 3), np.uint32))
    mat_id: np.ndarray = field(default_factory=lambda: np.zeros((0,), np.uint16))
    materials: np.ndarray = field(default_factory=lambda: np.zeros((0, 7), np.float32))
    lights: np.ndarray = field(default_factory=lambda: np.zeros((0, 7), np.float32))
    spheres: np.ndarray = field(default_factory=lambda: np.zeros((0, 5), np.float32))
    cam_to_world: np.ndarray = field(default_factory=lambda: np.eye(4, dtype=np.float32))
    fov: float = 45.0
    xres: int = 64
    yres: int = 64
    crop: tuple = (0.0, 1.0, 0.0, 1.0)
    mat_tex: np.ndarray = field(default_factory=lambda: np.zeros((0,), np.uint32))
    textures: np.ndarray = field(default_factory=lambda: np.zeros((0, 11), np.float32))
    tri_uv: np.ndarray = field(default_factory=lambda: np.zeros((0, 6), np.float32))
    mat_eta: np.ndarray = field(default_factory=lambda: np.zeros((0,), np.float32))
    envmap: np.ndarray = field(default_factory=lambda: np.zeros((0, 0, 3), np.float32))
    envmap_world_to_light: np.ndarray = field(default_factory=lambda: np.eye(3, dtype=np.float32))
    tri_n: np.ndarray = field(default_factory=lambda: np.zeros((0, 9), np.float32))
    pixel_filter: tuple = None
    images: list = field(default_factory=list)
    spot_cones: np.ndarray = field(default_factory=lambda: np.zeros((0, 5), np.float32))
    light_maps: np.ndarray = field(default_factory=lambda: np.zeros((0, 14), np.float32))

    def normalized(self):
        self.images = [np.ascontiguousarray(im, np.float32) for im in self.images]
        assert all(im.ndim == 3 and im.shape[2] == 3 for im in self.images)
        if self.pixel_filter is not None:
            self.pixel_filter = pixel_filter_tuple(self.pixel_filter)
        self.P = np.ascontiguousarray(self.P, np.float32).reshape(-1, 3)
        self.idx = np.ascontiguousarray(self.idx, np.uint32).reshape(-1, 3)
        self.mat_id = np.ascontiguousarray(self.mat_id, np.uint16).reshape(-1)
        self.materials = np.ascontiguousarray(self.materials, np.float32).reshape(-1, 7)
        self.lights = np.ascontiguousarray(self.lights, np.float32).reshape(-1, 7)
        self.spheres = np.ascontiguousarray(self.spheres, np.float32).reshape(-1, 5)
        self.cam_to_world = np.ascontiguousarray(self.cam_to_world, np.float32).reshape(4, 4)
        self.mat_tex = np.ascontiguousarray(self.mat_tex, np.uint32).reshape(-1)
        if self.mat_tex.shape[0] != self.materials.shape[0]:
            assert self.mat_tex.shape[0] == 0
            self.mat_tex = np.zeros(self.materials.shape[0], np.uint32)
        self.mat_eta = np.ascontiguousarray(self.mat_eta, np.float32).reshape(-1)
        if 0 < self.mat_eta.shape[0] < self.materials.shape[0]:  # (materials appended since: 1.5, as for an empty array)
            self.mat_eta = np.concatenate([self.mat_eta, np.full(self.materials.shape[0] - self.mat_eta.shape[0], 1.5, np.float32)])
        assert self.mat_eta.shape[0] in (0, self.materials.shape[0])
        self.textures = np.ascontiguousarray(self.textures, np.float32).reshape(-1, 11)
        self.tri_uv = np.ascontiguousarray(self.tri_uv, np.float32).reshape(-1, 6)
        self.envmap = np.ascontiguousarray(self.envmap, np.float32)
        assert self.envmap.ndim == 3 and self.envmap.shape[2] == 3
        self.envmap_world_to_light = np.ascontiguousarray(self.envmap_world_to_light, np.float32).reshape(3, 3)
        self.tri_n = np.ascontiguousarray(self.tri_n, np.float32).reshape(-1, 9)
        self.spot_cones = np.ascontiguousarray(self.spot_cones, np.float32).reshape(-1, 5)
        self.light_maps = np.ascontiguousarray(self.light_maps, np.float32).reshape(-1, 14)
        assert self.idx.shape[0] == self.mat_id.shape[0] and self.tri_uv.shape[0] in (0, self.idx.shape[0])
        assert self.tri_n.shape[0] in (0, self.idx.shape[0])
        return self

    def crop_size(self):
        b = film_cropped_bounds(self.xres, self.yres, self.crop)
        return max(b[2] - b[0], 0), max(b[3] - b[1], 0)


def fill_desc(desc, sd, mat_t, light_t, sphere_t, tex_t=None):
    """Fill a SceneDesc-shaped ctypes struct from a SceneData; returns the keep-alive list."""
    sd.normalized()
    mats = (mat_t * max(len(sd.materials), 1))()
    for i, m in enumerate(sd.materials):
        mats[i].type = int(m[0])
        mats[i].k[:] = [float(x) for x in m[1:4]]
        mats[i].le[:] = [float(x) for x in m[4:7]]
        mats[i].kd_tex = int(sd.mat_tex[i])
        if int(m[0]) == GLASS:  # include/pbrt_hip.h: k = Kr, le = Kt, kd_tex = the IEEE-754 bits of eta
            eta = sd.mat_eta[i:i + 1] if len(sd.mat_eta) else np.array([1.5], np.float32)
            mats[i].kd_tex = int(eta.view(np.uint32)[0])
        if int(m[0]) in (PLASTIC, SUBSTRATE):  # k = Kd, le = Ks, kd_tex = the IEEE-754 bits of alpha
            mats[i].kd_tex = int(sd.mat_eta[i:i + 1].view(np.uint32)[0]) if len(sd.mat_eta) else 0  # (no alpha given: 0, which scene creation refuses)
    # the table: every `textures` row in its own slot (mat_tex numbering does not move), then the records that travel with the scene, each in a
    # slot of its own -- the map's, the pixel filter's, the spot lights' cones, the mapped lights' records, the normals' (include/pbrt_hip.h
    # pbrt_hip_envmap / _pixel_filter / _spot_cone / _light_map / _normals), in this order
    records = [image_record(sd.images[int(t[1])], int(t[2]), int(t[3]), t[7:11]) if int(t[0]) == TEXTURE_IMAGE else checker_record(t) for t in sd.textures]
    has_env = sd.envmap.size > 0
    if has_env:
        records.append(EnvMap(type=_lib.SLOT_ENVMAP, width=sd.envmap.shape[1], height=sd.envmap.shape[0], rgb=_fp(sd.envmap),
                              world_to_light=tuple(float(x) for x in sd.envmap_world_to_light.reshape(-1))))
    if sd.pixel_filter is not None:
        records.append(pixel_filter_record(sd.pixel_filter))
    first_cone = len(records)  # (0-based slot of cone 0)
    for c in sd.spot_cones:
        records.append(SpotCone(type=_lib.SLOT_SPOT, axis=tuple(float(x) for x in c[0:3]), cos_total=float(c[3]), cos_start=float(c[4])))
    first_map = len(records)  # (0-based slot of light map 0)
    for m in sd.light_maps:
        records.append(LightMap(type=_lib.SLOT_LIGHT_MAP, kind=int(m[0]), image=int(m[1]), world_to_light=tuple(float(x) for x in m[2:11]), inv_tan=float(m[11]),
                                sx=float(m[12]), sy=float(m[13])))
    if sd.tri_n.shape[0]:
        records.append(Normals(type=_lib.SLOT_NORMALS, n_tris=sd.tri_n.shape[0], tri_n=_fp(sd.tri_n)))
    texs = None
    if records:
        tex_t = tex_t or dict(desc._fields_)["textures"]._type_  # (the Texture class of the caller's own struct mirror)
        texs = (tex_t * len(records))()
        for i, rec in enumerate(records):
            _lib.put_slot(texs, i, rec)
        desc.textures = texs
    desc.n_textures = len(records)
    if sd.tri_uv.shape[0]:
        desc.tri_uv = _fp(sd.tri_uv)
    lights = (light_t * max(len(sd.lights), 1))()
    n_spot = n_mapped = 0
    for i, l in enumerate(sd.lights):
        lights[i].type = int(l[0])
        lights[i].p[:] = [float(x) for x in l[1:4]]
        lights[i].c[:] = [float(x) for x in l[4:7]]
        if int(l[0]) == LIGHT_ENVMAP:  # `pad` = the bits of the 1-based number of the map's slot (0: the scene holds no map -- refused)
            lights[i].pad = float(np.array([len(sd.textures) + 1 if has_env else 0], np.uint32).view(np.float32)[0])
        if int(l[0]) == LIGHT_SPOT:  # `pad` = the bits of the 1-based number of its cone's slot (0: `spot_cones` has no row for it -- refused)
            lights[i].pad = float(np.array([first_cone + n_spot + 1 if n_spot < len(sd.spot_cones) else 0], np.uint32).view(np.float32)[0])
            n_spot += 1
        if int(l[0]) == LIGHT_MAPPED:  # likewise, of its record's slot
            lights[i].pad = float(np.array([first_map + n_mapped + 1 if n_mapped < len(sd.light_maps) else 0], np.uint32).view(np.float32)[0])
            n_mapped += 1
        if int(l[0]) == LIGHT_SPHERE:  # `pad` = the bits of the sphere's 1-based number (the row's first word is its 0-based row); p is not used
            lights[i].pad = float(np.array([int(l[1]) + 1 if 0 <= l[1] < 2 ** 24 else 0], np.uint32).view(np.float32)[0])
            lights[i].p[:] = [0.0, 0.0, 0.0]
    spheres = (sphere_t * max(len(sd.spheres), 1))()
    for i, s in enumerate(sd.spheres):
        spheres[i].c[:] = [float(x) for x in s[0:3]]
        spheres[i].r = float(s[3])
        spheres[i].mat = int(s[4])
    desc.P = _fp(sd.P)
    desc.idx = _u32p(sd.idx)
    desc.mat_id = sd.mat_id.ctypes.data_as(C.POINTER(C.c_uint16))
    desc.mats = mats
    desc.lights = lights
    desc.spheres = spheres
    desc.n_verts = sd.P.shape[0]
    desc.n_tris = sd.idx.shape[0]
    desc.n_mats = len(sd.materials)
    desc.n_lights = len(sd.lights)
    desc.n_spheres = len(sd.spheres)
    desc.cam_to_world[:] = [float(x) for x in sd.cam_to_world.reshape(-1)]
    desc.fov = float(sd.fov)
    desc.xres = int(sd.xres)
    desc.yres = int(sd.yres)
    desc.crop[:] = [float(x) for x in sd.crop]
    return [mats, lights, spheres, texs, sd]


def roughness_to_alpha(roughness, remap=True):
    """alpha of a plastic material as the scene parser forms it: the float32 roughness through pbrt-v3's RoughnessToAlpha
    polynomial in double (remap), rounded to float32 and clamped to [1e-3, 1]"""
    import math
    r = float(np.float32(roughness))
    a = r
    if remap:
        x = math.log(max(r, 1e-3))
        a = 1.62142 + 0.819955 * x + 0.1734 * x * x + 0.0171201 * x * x * x + 0.000640711 * x * x * x * x
    a = np.float32(a)
    return np.float32(min(max(a, np.float32(1e-3)), np.float32(1.0))) if a == a else np.float32(1e-3)


def plastic_material(kd=(0.25, 0.25, 0.25), ks=(0.25, 0.25, 0.25), roughness=0.1, remap=True):
    """-> (the `materials` row (PLASTIC, Kd, Ks), alpha for `mat_eta`) of Material "plastic" with these parameters (pbrt-v3's defaults)"""
    return [PLASTIC, *kd, *ks], roughness_to_alpha(roughness, remap)


def spot_light(p, to, I=(1.0, 1.0, 1.0), coneangle=30.0, conedeltaangle=5.0):
    """-> (the `lights` row (LIGHT_SPOT, p, I), the `spot_cones` row) of LightSource "spot" at `p` aimed at `to` (pbrt-v3's defaults), as the
    scene parser forms them under an identity CTM: the axis normalised in double and rounded, the cosines from the float32
    angles in double and rounded"""
    import math
    p32, to32 = np.asarray(p, np.float32), np.asarray(to, np.float32)
    d = to32.astype(np.float64) - p32.astype(np.float64)
    axis = (d / math.sqrt(float((d * d).sum()))).astype(np.float32)
    cone, delta = float(np.float32(coneangle)), float(np.float32(conedeltaangle))
    cos_total, cos_start = np.float32(math.cos(math.radians(cone))), np.float32(math.cos(math.radians(cone - delta)))
    return [LIGHT_SPOT, *p32, *I], [*axis, cos_total, max(cos_start, cos_total)]


def _rotation9(world_to_light):
    m = np.asarray(world_to_light, np.float32).reshape(-1)
    assert m.shape == (9,)
    return [float(x) for x in m]


def projection_light(p, image, I=(1.0, 1.0, 1.0), fov=45.0, aspect=1.0, world_to_light=np.eye(3)):
    """-> (the `lights` row (LIGHT_MAPPED, p, I), the `light_maps` row) of LightSource "projection" at `p` as the scene parser
    forms them: `image` = the 1-based number of the TEXTURE_IMAGE row of `textures` it projects (the parser's: bilinear, wrap clamp), `aspect` =
    that image's width / height, inv_tan = 1 / tan(fov / 2) from the float32 angle in double and rounded, the screen window pbrt-v3's.  The
    light looks along the +z of its own frame with +y up; world_to_light is a rotation, row-major."""
    import math
    f = float(np.float32(fov))
    if not (0.0 < f < 180.0):
        f = 45.0
    a = np.float32(aspect)
    sx, sy = (a, np.float32(1.0)) if a > 1.0 else (np.float32(1.0), np.float32(1.0) / a)
    return ([LIGHT_MAPPED, *np.asarray(p, np.float32), *I],
            [LIGHT_MAP_PROJECTION, int(image), *_rotation9(world_to_light), np.float32(1.0 / math.tan(f * (math.pi / 360.0))), sx, sy])


def goniometric_light(p, image, I=(1.0, 1.0, 1.0), world_to_light=np.eye(3)):
    """-> (the `lights` row (LIGHT_MAPPED, p, I), the `light_maps` row) of LightSource "goniometric" at `p`: `image` = the
    1-based number of the TEXTURE_IMAGE row of `textures` that is its latitude-longitude map (the parser's: bilinear, wrap repeat); the pole
    is the +y of the light's own frame"""
    return [LIGHT_MAPPED, *np.asarray(p, np.float32), *I], [LIGHT_MAP_GONIOMETRIC, int(image), *_rotation9(world_to_light), 0.0, 0.0, 0.0]


def light_map_eval_device(x, image, light_map, wrap=WRAP_CLAMP, filter=TEXFILTER_BILINEAR, device=0):
    """pbrt_hip_light_map_eval_device: csrc/light_map.hpp over arrays on the device.  x (n, 10): po, nf, p, nL; image (H, W, 3) float32 with
    row 0 = its top, read with `wrap` and `filter`; light_map = a `light_maps` row (its image number is not used) -> (n, 11) float32: ok, wi,
    tmax, scale = (cos / dist^2) nL, s, t, rgb; zeros behind ok = 0"""
    x = np.ascontiguousarray(x, np.float32).reshape(-1, 10)
    out = np.zeros((x.shape[0], 11), np.float32)
    im = np.ascontiguousarray(image, np.float32)
    rec = image_record(im, int(wrap), int(filter), (1.0, 1.0, 0.0, 0.0))
    m = np.asarray(light_map, np.float32).reshape(14)
    lm = LightMap(type=_lib.SLOT_LIGHT_MAP, kind=int(m[0]), image=1, world_to_light=tuple(float(v) for v in m[2:11]), inv_tan=float(m[11]), sx=float(m[12]), sy=float(m[13]))
    check(lib().pbrt_hip_light_map_eval_device(int(device), C.byref(rec), C.byref(lm), x.shape[0], _fp(x), _fp(out)), "pbrt_hip_light_map_eval_device")
    return out


def spot_eval_device(x, device=0):
    """pbrt_hip_spot_eval_device: csrc/spot_light.hpp over arrays on the device.  x (n, 15): po, nf, p, axis, cos_total, cos_start, nL ->
    (n, 7) float32: ok, wi, tmax, the falloff, scale = ((cos / dist^2) nL) falloff; zeros behind ok = 0"""
    x = np.ascontiguousarray(x, np.float32).reshape(-1, 15)
    out = np.zeros((x.shape[0], 7), np.float32)
    check(lib().pbrt_hip_spot_eval_device(int(device), x.shape[0], _fp(x), _fp(out)), "pbrt_hip_spot_eval_device")
    return out


def sphere_light(sd, k):
    """-> the `lights` row (LIGHT_SPHERE, k, 0, 0, L) that makes sphere k of `sd` a sphere light: L is the le of the sphere's
    material, which scene creation holds the row to bit for bit"""
    mat = int(np.asarray(sd.spheres, np.float32).reshape(-1, 5)[k, 4])
    return [LIGHT_SPHERE, float(k), 0.0, 0.0, *np.asarray(sd.materials, np.float32).reshape(-1, 7)[mat, 4:7]]


def sphere_light_eval(x, device=0):
    """pbrt_hip_sphere_light_eval_device: csrc/sphere_light.hpp over arrays on the device.  x (n, 13): po, nf, c, r, u1, u2, nL -> (n, 8)
    float32: ok, wi, tmax, scale = cos (1 / pdf_omega) nL, pdf_omega (zeros behind ok = 0), and the hit side's pdf_omega from po"""
    x = np.ascontiguousarray(x, np.float32).reshape(-1, 13)
    out = np.zeros((x.shape[0], 8), np.float32)
    check(lib().pbrt_hip_sphere_light_eval_device(int(device), x.shape[0], _fp(x), _fp(out)), "pbrt_hip_sphere_light_eval_device")
    return out


def substrate_material(kd=(0.5, 0.5, 0.5), ks=(0.5, 0.5, 0.5), uroughness=0.1, vroughness=0.1, remap=True):
    """-> (the `materials` row (SUBSTRATE, Kd, Ks), alpha for `mat_eta`) of Material "substrate" with these parameters (pbrt-v3's defaults), as
    the scene parser forms them: Ks clamped to 1, alpha = sqrt(alpha_u alpha_v) in double, rounded to float32"""
    import math
    au, av = (float(roughness_to_alpha(r, remap)) for r in (uroughness, vroughness))
    return [SUBSTRATE, *kd, *(min(float(np.float32(v)), 1.0) for v in ks)], np.float32(math.sqrt(au * av))


def substrate_eval_device(x, device=0):
    """pbrt_hip_substrate_eval_device: csrc/substrate_bsdf.hpp over arrays on the device, in plastic_eval_device's layout"""
    x = np.ascontiguousarray(x, np.float32).reshape(-1, 18)
    out = np.zeros((x.shape[0], 10), np.float32)
    check(lib().pbrt_hip_substrate_eval_device(int(device), x.shape[0], _fp(x), _fp(out)), "pbrt_hip_substrate_eval_device")
    return out


def plastic_eval_device(x, device=0):
    """pbrt_hip_plastic_eval_device: csrc/plastic_bsdf.hpp over arrays on the device.  x (n, 18): nf, wo, wi, u1, u2, Kd, Ks, alpha ->
    (n, 10) float32: f(wo, wi), pdf_b(wi), the sampled wi', f(wo, wi') cos / pdf_b(wi')"""
    x = np.ascontiguousarray(x, np.float32).reshape(-1, 18)
    out = np.zeros((x.shape[0], 10), np.float32)
    check(lib().pbrt_hip_plastic_eval_device(int(device), x.shape[0], _fp(x), _fp(out)), "pbrt_hip_plastic_eval_device")
    return out


def checker_record(row):
    """the pbrt_hip_texture record of a SceneData.textures row (type, tex1 rgb, tex2 rgb, su, sv, du, dv)"""
    su, sv, du, dv = (float(x) for x in row[7:11])
    return Texture(type=int(row[0]), tex1=tuple(float(x) for x in row[1:4]), tex2=tuple(float(x) for x in row[4:7]), su=su, sv=sv, du=du, dv=dv)


def image_record(image, wrap=WRAP_REPEAT, filter=TEXFILTER_BILINEAR, mapping=(1.0, 1.0, 0.0, 0.0)):
    """the pbrt_hip_image_texture record of an (H, W, 3) float32 C-contiguous array (row 0 = the image's top), which must outlive its use"""
    assert image.dtype == np.float32 and image.flags.c_contiguous and image.ndim == 3 and image.shape[2] == 3
    su, sv, du, dv = (float(x) for x in mapping)
    return ImageTexture(type=TEXTURE_IMAGE, width=image.shape[1], height=image.shape[0], wrap=WRAPS.get(wrap, wrap), rgb=_fp(image), su=su, sv=sv,
                        du=du, dv=dv, filter=TEXFILTERS.get(filter, filter))


def image_texture_row(image_index, wrap=WRAP_REPEAT, filter=TEXFILTER_BILINEAR, mapping=(1.0, 1.0, 0.0, 0.0)):
    """a SceneData.textures row that names SceneData.images[image_index]"""
    return [TEXTURE_IMAGE, image_index, WRAPS.get(wrap, wrap), TEXFILTERS.get(filter, filter), 0, 0, 0, *mapping]


def _image_lookup_eval(call, where, images, which, uv):
    """images: a list of (image, wrap, filter, mapping); uv: (n, 2) -> (n, 3) float32: Kd of record `which` at every (u, v)"""
    arrays = [np.ascontiguousarray(im[0], np.float32) for im in images]
    recs = (ImageTexture * len(images))(*[image_record(a, *im[1:]) for a, im in zip(arrays, images)])
    uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
    out = np.zeros((uv.shape[0], 3), np.float32)
    check(call(recs, len(images), int(which), uv.shape[0], _fp(uv), _fp(out)), where)
    return out


def image_lookup_eval_host(images, which, uv):
    """pbrt_hip_image_lookup_eval_host: csrc/image_lookup.hpp over arrays on the host (no device needed)"""
    return _image_lookup_eval(lib().pbrt_hip_image_lookup_eval_host, "pbrt_hip_image_lookup_eval_host", images, which, uv)


def image_lookup_eval_device(images, which, uv, device=0):
    """pbrt_hip_image_lookup_eval_device: the same on the device, over one uploaded texel pool"""
    return _image_lookup_eval(lambda *a: lib().pbrt_hip_image_lookup_eval_device(int(device), *a), "pbrt_hip_image_lookup_eval_device", images, which, uv)


SAMPLERS = {"stratified": 0, "sobol": 1, "sobol_nd": 2, "halton": 3}  # "sobol": the padded (0,2)-sequence sampler (3.10); "sobol_nd": Sobol' proper (3.12); "halton": 3.13


def make_render_desc(desc_t, integrator=INTEGRATOR_PATH, max_depth=5, spp=(1, 1), seed=0, rank=0, world_size=1,
                     flags=0, sampler="stratified", filter_width=(0.0, 0.0), max_sample_luminance=0.0):
    r = desc_t()
    r.sampler = SAMPLERS[sampler] if isinstance(sampler, str) else int(sampler)
    filter_width = filter_width or (0.0, 0.0)
    r.filter_xwidth, r.filter_ywidth = float(filter_width[0]), float(filter_width[1])
    r.max_sample_luminance = float(max_sample_luminance)
    r.integrator = integrator
    r.max_depth = max_depth
    r.spp_x, r.spp_y = int(spp[0]), int(spp[1])
    r.seed = seed
    r.rank = rank
    r.world_size = world_size
    r.flags = flags
    return r


def device_count():
    return lib().pbrt_hip_device_count()


def build_id():
    """pbrt_hip_build_id: hash of the sources and flags the loaded library was built from"""
    return lib().pbrt_hip_build_id().decode()


def look_at(pos, look, up):
    """Transform::look_at (transform.rs:485-520) -> (world_to_camera, camera_to_world) 4x4 float32."""
    m = np.zeros(16, np.float32)
    mi = np.zeros(16, np.float32)
    a = [np.asarray(v, np.float32) for v in (pos, look, up)]
    lib().pbrt_hip_look_at(_fp(a[0]), _fp(a[1]), _fp(a[2]), _fp(m), _fp(mi))
    return m.reshape(4, 4), mi.reshape(4, 4)


def film_cropped_bounds(xres, yres, crop):
    out = (C.c_int32 * 4)()
    lib().pbrt_hip_film_cropped_bounds(xres, yres, (C.c_float * 4)(*crop), out)
    return tuple(out)


def film_sample_bounds(xres, yres, crop, radius):
    out = (C.c_int32 * 4)()
    lib().pbrt_hip_film_sample_bounds(xres, yres, (C.c_float * 4)(*crop), radius[0], radius[1], out)
    return tuple(out)


def film_tile_bounds(xres, yres, crop, radius, sample_bounds):
    out = (C.c_int32 * 4)()
    lib().pbrt_hip_film_tile_bounds(xres, yres, (C.c_float * 4)(*crop), radius[0], radius[1],
                                    (C.c_int32 * 4)(*sample_bounds), out)
    return tuple(out)


def film_to_rgb(film_xyzw, scale=1.0):
    """Film::write_image's pixel arithmetic (film.rs:340-372): (h, w, 4) XYZW -> (h, w, 3) linear RGB."""
    f = np.ascontiguousarray(film_xyzw, np.float32)
    rgb = np.zeros(f.shape[:-1] + (3,), np.float32)
    lib().pbrt_hip_film_to_rgb(_fp(f), f.size // 4, scale, _fp(rgb))
    return rgb


def write_image(name, rgb):
    rgb = np.ascontiguousarray(rgb, np.float32)
    h, w = rgb.shape[:2]
    check(lib().pbrt_hip_write_image(str(name).encode(), _fp(rgb), w, h), "pbrt_hip_write_image")


def read_image(name):
    """imageio::read_image (imageio.rs:87-184): -> (h, w, 3) float32."""
    w, h = C.c_int32(0), C.c_int32(0)
    check(lib().pbrt_hip_read_image(str(name).encode(), None, C.byref(w), C.byref(h)), "pbrt_hip_read_image")
    rgb = np.zeros((h.value, w.value, 3), np.float32)
    check(lib().pbrt_hip_read_image(str(name).encode(), _fp(rgb), C.byref(w), C.byref(h)), "pbrt_hip_read_image")
    return rgb


def bvh_build_host(P, idx):
    """The host BVH builder alone (no device): returns (nodes[n,8] uint32 view, order, depth)."""
    P = np.ascontiguousarray(P, np.float32).reshape(-1, 3)
    idx = np.ascontiguousarray(idx, np.uint32).reshape(-1, 3)
    nt = idx.shape[0]
    nodes = np.zeros((max(2 * nt, 1), 8), np.uint32)
    order = np.zeros(max(nt, 1), np.uint32)
    nn, depth = C.c_uint32(), C.c_uint32()
    check(lib().pbrt_hip_bvh_build_host(_fp(P), P.shape[0], _u32p(idx), nt, _u32p(nodes), _u32p(order),
                                        C.byref(nn), C.byref(depth)), "pbrt_hip_bvh_build_host")
    return nodes[:nn.value].copy(), order[:nt].copy(), depth.value


def quad_build_host(P, idx, split_leaves=True):
    """The production walk's quantised 4-wide tree alone (no device): (quads[n, 16] uint32, stack_need)."""
    P = np.ascontiguousarray(P, np.float32).reshape(-1, 3)
    idx = np.ascontiguousarray(idx, np.uint32).reshape(-1, 3)
    cap = 2 * idx.shape[0] + 4
    quads = np.zeros((cap, 16), np.uint32)
    nq, need = C.c_uint32(), C.c_uint32()
    check(lib().pbrt_hip_quad_build_host(_fp(P), P.shape[0], _u32p(idx), idx.shape[0], int(split_leaves), _u32p(quads), cap,
                                         C.byref(nq), C.byref(need)), "pbrt_hip_quad_build_host")
    return quads[:nq.value].copy(), need.value


TREES = {"sah": 0, "reinsert": 2, "default": 0xFFFFFFFF}


def quad_build_host_ex(P, idx, tree="default", split_leaves=True):
    """pbrt_hip_quad_build_host_ex (no device): dict(quads[n, 16] uint32, stack_need, order = leaf slot -> triangle,
    root_box[6], n_refs) of the production walk's tree collapsed from the binary tree `tree` ("sah": canonical binned SAH; "reinsert": the same
    optimised by the device builder's re-insertion pass run on the host; "default")."""
    P = np.ascontiguousarray(P, np.float32).reshape(-1, 3)
    idx = np.ascontiguousarray(idx, np.uint32).reshape(-1, 3)
    nt = idx.shape[0]
    cap = 4 * nt + 4
    quads = np.zeros((cap, 16), np.uint32)
    order = np.zeros(max(nt, 1), np.uint32)
    box = np.zeros(6, np.float32)
    nq, need, nrefs = C.c_uint32(), C.c_uint32(), C.c_uint32()
    exact = np.zeros((cap, 24), np.float32)
    check(lib().pbrt_hip_quad_build_host_ex(_fp(P), P.shape[0], _u32p(idx), nt, int(split_leaves), TREES[tree], _u32p(quads), cap,
                                            C.byref(nq), C.byref(need), _u32p(order), _fp(box), C.byref(nrefs), _fp(exact)),
          "pbrt_hip_quad_build_host_ex")
    return {"quads": quads[:nq.value].copy(), "stack_need": need.value, "order": order[:nt].copy(), "root_box": box, "n_refs": nrefs.value,
            "exact_boxes": exact[:nq.value].copy()}


def _stage_tree_args(child, boxes, order):
    child = np.ascontiguousarray(child, np.uint32).reshape(-1)
    boxes = np.ascontiguousarray(boxes, np.float32).reshape(-1)
    order = np.ascontiguousarray(order, np.uint32).reshape(-1)
    n = order.size
    if n < 1 or child.size != 2 * (n - 1) or boxes.size != 6 * (2 * n - 1):
        raise ValueError("a tree of n leaves has 2 (n - 1) child words, 6 (2 n - 1) box floats and n order words")
    return n, child, boxes, order


def gpu_build_stages(P, idx, reinsert=True, device=0):
    """pbrt_hip_gpu_build_stages_device: the device tree builder run on a triangle soup with an observer between its stages ->
    dict(morton_keys; built / optimised = dict(child[n - 1, 2], parent_internal, parent_leaf, boxes[2 n - 1, 6], order); links = dict(par, kid[n - 1, 2],
    boxes) or None where stage 2 did not run; reinsert = its counts, or None; dp = dict(F[n - 1, 4, 3], Fl[n, 3], G) or None; quads[n_quads, 16],
    stack_need)"""
    P = np.ascontiguousarray(P, np.float32).reshape(-1, 3)
    idx = np.ascontiguousarray(idx, np.uint32).reshape(-1, 3)
    n = max(idx.shape[0], 2)
    u, f = (lambda *s: np.zeros(s, np.uint32)), (lambda *s: np.zeros(s, np.float32))
    tree = lambda: {"child": u(n - 1, 2), "parent_internal": u(n - 1), "parent_leaf": u(n), "boxes": f(2 * n - 1, 6), "order": u(n)}
    keys, built, opt = u(n), tree(), tree()
    links = {"par": u(2 * n - 1), "kid": u(n - 1, 2), "boxes": f(2 * n - 1, 6)}
    dp = {"F": f(n - 1, 4, 3), "Fl": f(n, 3), "G": f(n - 1)}
    quads = u(n, 16)
    st = _lib.BuildStages(morton_keys=_u32p(keys), links_par=_u32p(links["par"]), links_kid=_u32p(links["kid"]), links_boxes=_fp(links["boxes"]),
                          dp_F=_fp(dp["F"]), dp_Fl=_fp(dp["Fl"]), dp_G=_fp(dp["G"]), quads=_u32p(quads), quad_capacity=n)
    for name, t in (("built", built), ("opt", opt)):
        for k, a in t.items():
            setattr(st, f"{name}_{k}", _fp(a) if k == "boxes" else _u32p(a))
    check(lib().pbrt_hip_gpu_build_stages_device(device, _fp(P), P.shape[0], _u32p(idx), idx.shape[0], 1 if reinsert else 0, C.byref(st)),
          "pbrt_hip_gpu_build_stages_device")
    ran = bool(st.reinsert_ran)
    return {"morton_keys": keys, "built": built, "optimised": opt, "links": links if ran else None,
            "reinsert": {"passes": st.passes, "moves": st.moves, "undone": st.undone, "visits": st.visits, "cost_before": st.cost_before,
                         "cost_after": st.cost_after} if ran else None,
            "dp": dp if st.dp_ran else None, "quads": quads[:st.n_quads].copy(), "stack_need": st.stack_need}


def reinsert_links_host(child, boxes, order):
    """pbrt_hip_reinsert_links_host (no device): stage 2 of the device builder run on the host on the binary tree child / boxes / order ->
    dict(par, kid[n - 1, 2], boxes[2 n - 1, 6], passes, visits, found, applied, max_visits, undone, fixed_before, fixed_after, fixed_exp, valid)"""
    n, child, boxes, order = _stage_tree_args(child, boxes, order)
    par, kid, bx = np.zeros(2 * n - 1, np.uint32), np.zeros((n - 1, 2), np.uint32), np.zeros((2 * n - 1, 6), np.float32)
    stats = np.zeros(8, np.uint64)
    e, valid = C.c_int32(), C.c_uint32()
    check(lib().pbrt_hip_reinsert_links_host(n, _u32p(child), _fp(boxes), _u32p(order), _u32p(par), _u32p(kid), _fp(bx),
                                             stats.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(e), C.byref(valid)), "pbrt_hip_reinsert_links_host")
    out = {"par": par, "kid": kid, "boxes": bx, "fixed_exp": e.value, "valid": bool(valid.value)}
    out.update(zip(("passes", "visits", "found", "applied", "max_visits", "undone", "fixed_before", "fixed_after"), (int(v) for v in stats)))
    return out


COLLAPSE_RULES = {"greedy": 1, "dp": 2}


def collapse_host(child, boxes, order, rule):
    """pbrt_hip_collapse_host (no device): stage 3 on the binary tree child / boxes / order, `rule` "dp" or "greedy" -> (quads[n, 16], stack_need)"""
    n, child, boxes, order = _stage_tree_args(child, boxes, order)
    quads = np.zeros((n, 16), np.uint32)
    nq, need = C.c_uint32(), C.c_uint32()
    check(lib().pbrt_hip_collapse_host(n, _u32p(child), _fp(boxes), _u32p(order), COLLAPSE_RULES[rule], _u32p(quads), n, C.byref(nq), C.byref(need)),
          "pbrt_hip_collapse_host")
    return quads[:nq.value].copy(), need.value


def film_from_acc(acc, weighted=False):
    """pbrt_hip_film_from_acc: (..., 4) int64 accumulators -> (..., 4) float32 film pixels {X, Y, Z, weight}.  weighted: the accumulators
    of a weighted pixel filter, whose fourth is the weight sum in 2^-24 units (pbrt_hip_film_from_acc_weighted)."""
    a = np.ascontiguousarray(acc, np.int64)
    film = np.zeros(a.shape[:-1] + (4,), np.float32)
    call = lib().pbrt_hip_film_from_acc_weighted if weighted else lib().pbrt_hip_film_from_acc
    call(a.ctypes.data_as(C.POINTER(C.c_int64)), a.size // 4, _fp(film))
    return film


def pixel_filter_tuple(pixel_filter):
    """(kind number, param0, param1) of a SceneData.pixel_filter: a kind's name or number, or (kind, param0[, param1]); parameters left out
    are pbrt-v3's defaults"""
    pf = (pixel_filter,) if isinstance(pixel_filter, (str, int)) else tuple(pixel_filter)
    kind = FILTER_KINDS[pf[0]] if isinstance(pf[0], str) else int(pf[0])
    dflt = FILTER_DEFAULT_PARAMS.get(kind, (0.0, 0.0))
    return (kind,) + tuple(float(pf[1 + k]) if len(pf) > 1 + k else dflt[k] for k in range(2))


def pixel_filter_record(pixel_filter):
    """the pbrt_hip_pixel_filter of a SceneData.pixel_filter (a kind's name or number, or (kind, param0, param1))"""
    kind, p0, p1 = pixel_filter_tuple(pixel_filter)
    rec = PixelFilter(type=3, kind=kind)
    rec.param[:] = [p0, p1]
    return rec


def filter_table(pixel_filter, radius=(0.0, 0.0)):
    """pbrt_hip_filter_table (host only): the (16, 16) float32 table of weights of a pixel filter -- [iy, ix] = the filter at ((ix + 0.5) rx /
    16, (iy + 0.5) ry / 16), evaluated in double and rounded once -- for radii `radius` (0 = the kind's default: 2, the sinc 4), DESIGN.md 3.19"""
    rec = pixel_filter_record(pixel_filter)
    rx, ry = (float(r) if float(r) != 0.0 else filter_default_radius(rec.kind) for r in radius)
    out = np.zeros((16, 16), np.float32)
    check(lib().pbrt_hip_filter_table(C.byref(rec), rx, ry, _fp(out)), "pbrt_hip_filter_table")
    return out


def filter_default_radius(kind):
    """pbrt-v3's default radius of a weighted filter (both axes): 2, the sinc's 4"""
    kind = FILTER_KINDS[kind] if isinstance(kind, str) else int(kind)
    return 4.0 if kind == FILTER_SINC else 2.0


def filter_footprint_eval(radius, crop_bounds, points=None, pair_points=None, pair_pixels=None, device=0):
    """pbrt_hip_filter_footprint_eval_device: csrc/filter_weight.inc over arrays on the device, for radii `radius` and the cropped window
    crop_bounds = (x0, y0, x1, y1).  points (n, 2) float32 -> bounds (n, 4) int32 {x0, y0, x1, y1} of the clipped footprints; pair_points (m,
    2) float32 with pair_pixels (m, 2) int32 -> index (m,) int32 into the filter table, -1 outside the footprint.  -> (bounds, index)"""
    pts = np.ascontiguousarray(np.zeros((0, 2)) if points is None else points, np.float32).reshape(-1, 2)
    pp = np.ascontiguousarray(np.zeros((0, 2)) if pair_points is None else pair_points, np.float32).reshape(-1, 2)
    px = np.ascontiguousarray(np.zeros((0, 2)) if pair_pixels is None else pair_pixels, np.int32).reshape(-1, 2)
    assert len(pp) == len(px)
    bounds, index = np.zeros((len(pts), 4), np.int32), np.zeros(len(pp), np.int32)
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    check(lib().pbrt_hip_filter_footprint_eval_device(int(device), float(radius[0]), float(radius[1]), (C.c_int32 * 4)(*[int(v) for v in crop_bounds]), len(pts),
                                                      _fp(pts), i32(bounds), len(pp), _fp(pp), i32(px), i32(index)), "pbrt_hip_filter_footprint_eval_device")
    return bounds, index


def envmap_tables(rgb):
    """pbrt_hip_envmap_tables (host only): the importance-sampling tables of an (H, W, 3) map -> (marginal[H + 1], conditional[H, W + 1],
    p_uv[H, W]), DESIGN.md 3.17"""
    rgb = np.ascontiguousarray(rgb, np.float32)
    h, w = rgb.shape[:2]
    marg, cond, puv = np.zeros(h + 1, np.float32), np.zeros((h, w + 1), np.float32), np.zeros((h, w), np.float32)
    check(lib().pbrt_hip_envmap_tables(_fp(rgb), w, h, _fp(marg), _fp(cond), _fp(puv)), "pbrt_hip_envmap_tables")
    return marg, cond, puv


def _envmap_eval(call, where, n_or_u, d):
    u12 = None if n_or_u is None else np.ascontiguousarray(n_or_u, np.float32).reshape(-1, 2)
    d = np.zeros((len(u12), 3), np.float32) if u12 is not None else np.ascontiguousarray(d, np.float32).reshape(-1, 3).copy()
    n = len(d)
    texel, le, pdf = np.zeros(n, np.uint32), np.zeros((n, 3), np.float32), np.zeros(n, np.float32)
    check(call(n, _fp(u12) if u12 is not None else None, _fp(d), _u32p(texel), _fp(le), _fp(pdf)), where)
    return d, texel, le, pdf


def envmap_eval_host(rgb, world_to_light=None, u12=None, d=None):
    """pbrt_hip_envmap_eval_host: csrc/envmap_core.hpp over arrays on the host.  u12 (n, 2): SAMPLE -> (d[n, 3], texel[n] = row * W + col,
    le[n, 3] = the texel's rgb, pdf[n] over solid angle); else d (n, 3): LOOKUP -> the same four, d as given."""
    rgb = np.ascontiguousarray(rgb, np.float32)
    m = np.ascontiguousarray(np.eye(3) if world_to_light is None else world_to_light, np.float32).reshape(3, 3)
    h, w = rgb.shape[:2]
    return _envmap_eval(lambda n, u, dd, t, le, pdf: lib().pbrt_hip_envmap_eval_host(_fp(rgb), w, h, _fp(m), n, u, dd, t, le, pdf),
                        "pbrt_hip_envmap_eval_host", u12, d)


# op codes of pbrt_hip_blocks_eval_device (include/pbrt_hip_debug.h PBRT_HIP_BLOCK_*): name -> (op, floats read, floats written per element)
BLOCK_OPS = {"SIN": (0, 1, 1), "COS": (1, 1, 1), "ATAN_POS": (2, 1, 1), "ACOS": (3, 1, 1), "SINCOS": (4, 1, 2), "SPHERE_UV": (5, 3, 2),
             "FRESNEL": (6, 2, 2), "COSINE_ABOUT": (7, 5, 4), "SPHERE_HIT": (8, 11, 2),
             "QUAD_STEP": (9, 24, 6), "QUAD_STEP_PK": (10, 24, 6), "TRI_HIT": (11, 16, 4),
             "MIS_W_LIGHT": (12, 2, 1), "MIS_W_BSDF": (13, 2, 1), "LIGHT": (14, 33, 8)}


def blocks_eval(op, x, device=0):
    """pbrt_hip_blocks_eval_device: the kernels' building blocks (csrc/cephes_poly.hpp, kernel_math.hpp, envmap_core.hpp) over arrays on
    the device.  op: a name of BLOCK_OPS; x: (n, floats read) float32 -> (n, floats written) float32."""
    code, w_in, w_out = BLOCK_OPS[op]
    x = np.ascontiguousarray(x, np.float32).reshape(-1, w_in)
    out = np.zeros((len(x), w_out), np.float32)
    check(lib().pbrt_hip_blocks_eval_device(int(device), code, len(x), _fp(x), _fp(out)), "pbrt_hip_blocks_eval_device")
    return out


def shading_normal_eval(x, device=0):
    """pbrt_hip_shading_normal_eval_device: csrc/shading_normal.inc over arrays on the device.  x: (n, 17) float32 rows (n0, n1, n2, ng, b1,
    b2, wo) -> (n, 4) float32 rows (nsf, fell_back), DESIGN.md 3.18"""
    x = np.ascontiguousarray(x, np.float32).reshape(-1, 17)
    out = np.zeros((len(x), 4), np.float32)
    check(lib().pbrt_hip_shading_normal_eval_device(int(device), len(x), _fp(x), _fp(out)), "pbrt_hip_shading_normal_eval_device")
    return out


def sobol_matrices():
    """pbrt_hip_sobol_matrices: (128, 32) uint32 generator matrices of sampler 2 (host only)"""
    out = np.zeros((128, 32), np.uint32)
    lib().pbrt_hip_sobol_matrices(_u32p(out))
    return out


def slab_pixel_index(xres, yres, crop, rank, world_size):
    n = lib().pbrt_hip_slab_floats(xres, yres, (C.c_float * 4)(*crop), rank, world_size)
    if n < 0:
        raise ValueError("bad sharding arguments")
    out = np.zeros(n // 4, np.int64)
    if n:
        check(lib().pbrt_hip_slab_pixel_index(xres, yres, (C.c_float * 4)(*crop), rank, world_size,
                                              out.ctypes.data_as(C.POINTER(C.c_int64))), "pbrt_hip_slab_pixel_index")
    return out


class MultiScene:
    """A scene replicated on n GPUs of this node inside ONE process (pbrt_hip_multi_*): GPU g renders the super-tiles
    t % n == g from its own host thread and stream, one RCCL gather assembles the film on GPU 0."""

    def __init__(self, sd, n_gpus=0, builder=None):
        """builder: as Scene (None = the library's default, the device builder)."""
        self._h = None
        self.sd = sd.normalized()
        desc = SceneDesc()
        keep = fill_desc(desc, self.sd, Material, Light, Sphere, Texture)
        h = C.c_void_p()
        check(lib().pbrt_hip_multi_create(C.byref(desc), int(n_gpus), BUILDERS[builder] if builder else 0, C.byref(h)),
              "pbrt_hip_multi_create")
        del keep
        self._h = h
        self.n_gpus = lib().pbrt_hip_multi_gpus(h)

    def render(self, host_film=True, **kw):
        """-> (film[h, w, 4] or None, [stats dict per GPU]).  kw as Scene.render (rank / world_size are set by the library)."""
        r = make_render_desc(RenderDesc, **kw)
        w, h = self.sd.crop_size()
        film = np.zeros((h, w, 4), np.float32) if host_film else None
        st = (Stats * self.n_gpus)()
        check(lib().pbrt_hip_multi_render(self._h, C.byref(r), _fp(film) if host_film else None, st), "pbrt_hip_multi_render")
        return film, [{k: getattr(s, k) for k, _ in Stats._fields_} for s in st]

    def film_device_ptr(self):
        p = C.c_void_p()
        check(lib().pbrt_hip_multi_film_device(self._h, C.byref(p)), "pbrt_hip_multi_film_device")
        return p.value

    def close(self):
        if self._h:
            lib().pbrt_hip_multi_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        self.close()


def render_multi(sd, n_gpus=0, **kw):
    """pbrt_hip_render_multi: create + render on n GPUs + destroy in one call -> (film, [stats per GPU])."""
    sd = sd.normalized()
    desc = SceneDesc()
    keep = fill_desc(desc, sd, Material, Light, Sphere, Texture)
    r = make_render_desc(RenderDesc, **kw)
    n = n_gpus if n_gpus > 0 else device_count()
    w, h = sd.crop_size()
    film = np.zeros((h, w, 4), np.float32)
    st = (Stats * max(n, 1))()
    check(lib().pbrt_hip_render_multi(C.byref(desc), C.byref(r), int(n_gpus), _fp(film), st), "pbrt_hip_render_multi")
    del keep
    return film, [{k: getattr(s, k) for k, _ in Stats._fields_} for s in st]


class Scene:
    """A scene resident in HBM (flattened BVH + leaf-ordered triangles + tables)."""

    def __init__(self, sd, device=-1, builder=None):
        """builder: None (the library's one default: pbrt_hip_scene_create = "gpu" unless PBRT_HIP_BUILDER=host), "host" (the host's
        binned-SAH builder, the canonical tree), "gpu" (accelerator built AND optimised by parallel
        re-insertion on the device: tens of milliseconds), "gpu-plain" (the device's tree as built,
        PBRT_HIP_SCENE_PLAIN_TREE: A-B runs) or "host-optimized" (PBRT_HIP_SCENE_OPTIMIZED_TREE: the host builder
        followed by the same re-insertion pass run on one host core, seconds per million triangles).  Same film and hit records whichever
        is used."""
        self.sd = sd.normalized()
        desc = SceneDesc()
        keep = fill_desc(desc, self.sd, Material, Light, Sphere, Texture)
        h = C.c_void_p()
        if builder is None:
            check(lib().pbrt_hip_scene_create(C.byref(desc), device, C.byref(h)), "pbrt_hip_scene_create")
        else:
            flags = BUILDERS[builder]
            check(lib().pbrt_hip_scene_create_ex(C.byref(desc), device, flags, C.byref(h)), "pbrt_hip_scene_create_ex")
        del keep
        self._h = h

    def build_info(self):
        g, ms = C.c_uint32(), C.c_double()
        check(lib().pbrt_hip_scene_build_info(self._h, C.byref(g), C.byref(ms)), "pbrt_hip_scene_build_info")
        r, cms = C.c_uint32(), C.c_double()
        check(lib().pbrt_hip_scene_canonical_info(self._h, C.byref(r), C.byref(cms)), "pbrt_hip_scene_canonical_info")
        op, om, oms = C.c_uint32(), C.c_uint32(), C.c_double()
        check(lib().pbrt_hip_scene_optimize_info(self._h, C.byref(op), C.byref(om), C.byref(oms)), "pbrt_hip_scene_optimize_info")
        cb, ca, un = C.c_double(), C.c_double(), C.c_uint32()
        check(lib().pbrt_hip_scene_optimize_cost(self._h, C.byref(cb), C.byref(ca), C.byref(un)), "pbrt_hip_scene_optimize_cost")
        return {"gpu_built": bool(g.value), "build_ms": ms.value, "canonical_tree_ready": bool(r.value), "canonical_tree_host_build_ms": cms.value,
                "reinsert_passes": op.value, "reinsert_moves": om.value, "reinsert_ms": oms.value,
                "reinsert_area_before": cb.value, "reinsert_area_after": ca.value, "reinsert_pass_undone": bool(un.value)}

    def export_quads(self):
        """(quads[n, 16] uint32, order[n_tris] uint32): the production walk's tree as it sits in HBM."""
        n = C.c_uint32()
        check(lib().pbrt_hip_scene_export_quads(self._h, None, 0, C.byref(n), None), "pbrt_hip_scene_export_quads")
        quads = np.zeros((max(n.value, 1), 16), np.uint32)
        order = np.zeros(max(self.n_prims, 1), np.uint32)
        check(lib().pbrt_hip_scene_export_quads(self._h, _u32p(quads), quads.shape[0], C.byref(n), _u32p(order)),
              "pbrt_hip_scene_export_quads")
        return quads[:n.value], order[:self.n_prims]

    def close(self):
        if getattr(self, "_h", None):
            lib().pbrt_hip_scene_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def n_prims(self):
        """primitives of the tree: the triangles, then the spheres (primitive n_tris + s)"""
        return int(self.sd.idx.shape[0]) + int(self.sd.spheres.shape[0])

    def info(self):
        nn, depth, nl, nb = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint64()
        check(lib().pbrt_hip_scene_info(self._h, C.byref(nn), C.byref(depth), C.byref(nl), C.byref(nb)),
              "pbrt_hip_scene_info")
        qn, need = C.c_uint32(), C.c_uint32()
        check(lib().pbrt_hip_scene_walk_info(self._h, C.byref(qn), C.byref(need)), "pbrt_hip_scene_walk_info")
        return {"n_nodes": nn.value, "depth": depth.value, "n_lights": nl.value, "device_bytes": nb.value,
                "quad_nodes": qn.value, "quad_stack_need": need.value}

    def export_bvh(self):
        i = self.info()
        nodes = np.zeros((max(i["n_nodes"], 1), 8), np.uint32)
        order = np.zeros(max(self.n_prims, 1), np.uint32)
        check(lib().pbrt_hip_scene_export_bvh(self._h, _u32p(nodes), _u32p(order)), "pbrt_hip_scene_export_bvh")
        return nodes[:i["n_nodes"]], order[:self.n_prims]

    def render(self, integrator=INTEGRATOR_PATH, max_depth=5, spp=(1, 1), seed=0, rank=0, world_size=1,
               counters=False, **kw):
        """-> (film[h, w, 4] float32 {X, Y, Z, weight}, stats dict).  counters: False, True (canonical
        walk, equal to the oracle's counters) or "walk" (what the production kernel itself fetches / tests).
        kw: sampler="stratified"|"sobol", filter_width=(xw, yw)."""
        r = make_render_desc(RenderDesc, integrator, max_depth, spp, seed, rank, world_size,
                             FLAG_WALK_COUNTERS if counters == "walk" else (FLAG_COUNTERS if counters else 0), **kw)
        w, h = self.sd.crop_size()
        film = np.zeros((h, w, 4), np.float32)
        st = Stats()
        check(lib().pbrt_hip_render(self._h, C.byref(r), _fp(film), C.byref(st)), "pbrt_hip_render")
        return film, {k: getattr(st, k) for k, _ in Stats._fields_}

    def envmap_eval(self, u12=None, d=None):
        """pbrt_hip_envmap_eval_device: envmap_eval_host's arithmetic on the device, over the map this scene holds"""
        return _envmap_eval(lambda n, u, dd, t, le, pdf: lib().pbrt_hip_envmap_eval_device(self._h, n, u, dd, t, le, pdf),
                            "pbrt_hip_envmap_eval_device", u12, d)

    def render_acc(self, filter_width, **kw):
        """A box filter radius other than 0.5: this rank's fixed-point film accumulators (h, w, 4) int64 {r, g, b, samples}
        (pbrt_hip_render_acc); accumulators of ranks add exactly, film_from_acc converts.  A scene with a pixel_filter: at every radius, the
        fourth accumulator the weight sum in 2^-24 units (film_from_acc(acc, weighted=True)).  kw as render."""
        r = make_render_desc(RenderDesc, filter_width=filter_width, **kw)
        w, h = self.sd.crop_size()
        acc = np.zeros((h, w, 4), np.int64)
        st = Stats()
        check(lib().pbrt_hip_render_acc(self._h, C.byref(r), acc.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(st)), "pbrt_hip_render_acc")
        return acc, {k: getattr(st, k) for k, _ in Stats._fields_}

    def render_buffer_bytes(self, **kw):
        """bytes render_device writes for this render description (slab of the rank, or the accumulators of a wide filter)"""
        kw.pop("counters", None)
        r = make_render_desc(RenderDesc, **kw)
        return lib().pbrt_hip_render_buffer_bytes(self._h, C.byref(r))

    def film_from_acc_device(self, d_acc_ptr, d_film_ptr, stream_ptr=None):
        check(lib().pbrt_hip_film_from_acc_device(self._h, C.c_void_p(d_acc_ptr), C.c_void_p(d_film_ptr), C.c_void_p(stream_ptr or 0)),
              "pbrt_hip_film_from_acc_device")

    def render_device(self, d_slab_ptr, stream_ptr=None, **kw):
        """Asynchronous render into a device slab (e.g. a torch tensor's data_ptr())."""
        counters = kw.pop("counters", False)
        r = make_render_desc(RenderDesc, flags=FLAG_WALK_COUNTERS if counters == "walk" else (FLAG_COUNTERS if counters else 0), **kw)
        check(lib().pbrt_hip_render_device(self._h, C.byref(r), C.c_void_p(d_slab_ptr), C.c_void_p(stream_ptr or 0)),
              "pbrt_hip_render_device")

    def render_prepare(self, **kw):
        """pbrt_hip_render_prepare: allocate the scratch a render with these arguments needs, launch nothing."""
        kw.pop("counters", None)
        r = make_render_desc(RenderDesc, **kw)
        check(lib().pbrt_hip_render_prepare(self._h, C.byref(r)), "pbrt_hip_render_prepare")

    def render_wait(self):
        st = Stats()
        check(lib().pbrt_hip_render_wait(self._h, C.byref(st)), "pbrt_hip_render_wait")
        return {k: getattr(st, k) for k, _ in Stats._fields_}

    def film_assemble_device(self, d_slab_ptr, rank, world_size, d_film_ptr, stream_ptr=None):
        check(lib().pbrt_hip_film_assemble_device(self._h, C.c_void_p(d_slab_ptr), rank, world_size,
                                                  C.c_void_p(d_film_ptr), C.c_void_p(stream_ptr or 0)),
              "pbrt_hip_film_assemble_device")

    def slab_floats(self, rank=0, world_size=1):
        return lib().pbrt_hip_slab_floats(self.sd.xres, self.sd.yres, (C.c_float * 4)(*self.sd.crop), rank, world_size)

    def intersect(self, o, d, tmax, counters=False):
        o = np.ascontiguousarray(o, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(d, np.float32).reshape(-1, 3)
        tmax = np.ascontiguousarray(tmax, np.float32).reshape(-1)
        n = o.shape[0]
        t = np.zeros(n, np.float32)
        prim = np.zeros(n, np.uint32)
        b1 = np.zeros(n, np.float32)
        b2 = np.zeros(n, np.float32)
        cnt = (C.c_uint64 * 2)()
        check(lib().pbrt_hip_intersect(self._h, n, _fp(o), _fp(d), _fp(tmax), _fp(t), _u32p(prim), _fp(b1), _fp(b2),
                                       cnt if counters else None), "pbrt_hip_intersect")
        return t, prim, b1, b2, (cnt[0], cnt[1])

    def occluded(self, o, d, tmax):
        o = np.ascontiguousarray(o, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(d, np.float32).reshape(-1, 3)
        tmax = np.ascontiguousarray(tmax, np.float32).reshape(-1)
        n = o.shape[0]
        hit = np.zeros(n, np.uint8)
        check(lib().pbrt_hip_occluded(self._h, n, _fp(o), _fp(d), _fp(tmax),
                                      hit.ctypes.data_as(C.POINTER(C.c_uint8))), "pbrt_hip_occluded")
        return hit
