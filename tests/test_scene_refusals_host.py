"""Scene creation's refusals, whole: every faulty description gets the status code and the full message recorded here, and of the pairs of
faults listed here -- one pair, at least, across every boundary between two stages of check_scene_desc -- the one named first is the one
reported.  (Not pinned: which of two materials whose kd_tex name slots of different wrong kinds is reported.)  The description is checked before a device is asked for, so none of this needs a GPU (a sound
description gives PBRT_HIP_ERR_NO_DEVICE without one; only the faulty ones are asserted on).  With it: the slot helpers of pbrt_amd/_lib.py,
the table api.fill_desc writes, and pbrt_amd/csrc/texture_table.hpp compiled into a stand-alone program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from pbrt_amd import GLASS, LIGHT_ENVMAP, LIGHT_POINT, MATTE, SceneData, _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, LIMIT = -1, -4
NAN, INF = float("nan"), float("inf")
NO_FLOATS = C.POINTER(C.c_float)()
UNKNOWN_FLAG, HOST_AND_GPU_BUILD = 16, api.SCENE_HOST_BUILD | api.SCENE_GPU_BUILD


# ---- the descriptions: two triangles, one matte material, one point light, and what a case adds ----

def _scene(**kw):
    kw.setdefault("materials", [[MATTE, 0.5, 0.5, 0.5, 0, 0, 0]])
    kw.setdefault("lights", [[LIGHT_POINT, 0, 0, 3, 1, 1, 1]])
    return SceneData(P=np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], np.float32), idx=np.array([[0, 1, 2], [0, 2, 3]], np.uint32),
                     mat_id=np.zeros(2, np.uint16), xres=8, yres=8, **kw).normalized()


UV = np.array([[0, 0, 1, 0, 1, 1], [0, 0, 1, 1, 0, 1]], np.float32)
ENV_LIGHT = [LIGHT_ENVMAP, 0, 0, 0, 1, 1, 1]


def _sphere(c=(0, 0, 1), r=0.5, mat=0):
    return _scene(spheres=[[*c, r, mat]])


def _checker(row=(0, 1, 1, 1, 0, 0, 0, 2, 2, 0, 0), tri_uv=UV):
    return _scene(textures=[row], mat_tex=[1], tri_uv=tri_uv)


def _image(texels=None):
    return _scene(images=[np.full((2, 2, 3), 0.5, np.float32) if texels is None else texels], textures=[api.image_texture_row(0)], mat_tex=[1], tri_uv=UV)


def _env(sky=None, lights=(ENV_LIGHT,)):
    return _scene(lights=list(lights), envmap=np.full((2, 4, 3), 0.5, np.float32) if sky is None else sky)


def _filtered():
    return _scene(pixel_filter="gaussian")


def _normals(tri_n=None):
    return _scene(tri_n=np.tile(np.array([0, 0, 1], np.float32), (2, 3)) if tri_n is None else tri_n)


def _with(a, index, value):
    a = np.array(a, np.float32)
    a[index] = value
    return a


# ---- edits of the filled ctypes description ----

def _set(**fields):
    """desc.<field> = value; a key "a__3" sets desc.a[3], "mats__0__kd_tex" sets desc.mats[0].kd_tex"""
    def edit(desc):
        for key, value in fields.items():
            *path, last = [int(p) if p.isdigit() else p for p in key.split("__")]
            obj = desc
            for p in path:
                obj = obj[p] if isinstance(p, int) else getattr(obj, p)
            if isinstance(last, int):
                obj[last] = value
            else:
                setattr(obj, last, value)
    return edit


def _slot(index, cls, **fields):
    """slot `index` of the table read as a `cls`, changed, and written back"""
    def edit(desc):
        rec = cls.from_buffer_copy(C.string_at(C.byref(desc.textures[index]), 64))
        _set(**fields)(rec)
        C.memmove(C.byref(desc.textures[index]), C.byref(rec), 64)
    return edit


def _table(*records):
    """the description's table replaced by these records"""
    def edit(desc):
        texs = (_lib.Texture * len(records))()
        for i, r in enumerate(records):
            C.memmove(C.byref(texs, 64 * i), C.byref(r), 64)
        desc.textures, desc.n_textures = texs, len(records)
        return texs, records
    return edit


def _both(*edits):
    return lambda desc: [e(desc) for e in edits]


def _filter_rec(kind=2, p0=2.0, p1=0.0):
    r = _lib.PixelFilter(type=3, kind=kind)
    r.param[:] = [p0, p1]
    return r


ONE_TEXEL = np.full((1, 1, 3), 0.5, np.float32)
TRI_N = np.tile(np.array([0, 0, 1], np.float32), (2, 3))


def _image_rec(width=1, height=1):
    """(every record of a case points at the one texel: a table whose sizes or totals are refused is refused before a texel is read)"""
    r = api.image_record(ONE_TEXEL)
    r.width, r.height = width, height
    return r


def _normals_rec(n_tris=2):
    return _lib.Normals(type=2, n_tris=n_tris, tri_n=TRI_N.ctypes.data_as(C.POINTER(C.c_float)))


def _create(sd, edit=None, flags=0):
    """pbrt_hip_scene_create_ex on `sd`'s description after `edit`: (code, message)"""
    desc = _lib.SceneDesc()
    keep = api.fill_desc(desc, sd, _lib.Material, _lib.Light, _lib.Sphere, _lib.Texture)
    if edit:
        keep.append(edit(desc))
    h = C.c_void_p()
    rc = _lib.lib().pbrt_hip_scene_create_ex(C.byref(desc), 0, flags, C.byref(h))
    msg = _lib.lib().pbrt_hip_last_error().decode()
    if rc == 0:
        _lib.lib().pbrt_hip_scene_destroy(h)
    return rc, msg


# ---- one case per refusal: name -> (scene, edit, flags), and what the library answered before its checks were rearranged ----
SLOT1 = "scene_create: texture slot 1: "
CASES = {
    # the mesh and the spheres
    "resolution": (_scene, _set(xres=0), 0),
    "mesh arrays": (_scene, _set(P=NO_FLOATS), 0),
    "no materials": (_scene, _set(n_mats=0), 0),
    "materials cap": (_scene, _set(n_mats=65537), 0),
    "triangles cap": (_scene, _set(n_tris=(1 << 24) + 1), 0),
    "primitives cap": (_scene, _set(n_spheres=(1 << 24) - 1), 0),
    "no sphere table": (_scene, _set(n_spheres=1, spheres=C.POINTER(_lib.Sphere)()), 0),
    "vertex index": (_scene, _set(idx__5=99), 0),
    "material id": (_scene, _set(mat_id__1=5), 0),
    "vertex": (_scene, _set(P__4=NAN), 0),
    "sphere radius": (lambda: _sphere(r=-1.0), None, 0),
    "sphere material": (lambda: _sphere(mat=3), None, 0),
    "sphere box": (lambda: _sphere(c=(3e38, 0, 0), r=3e38), None, 0),
    # the lights
    "no light table": (_scene, _set(lights=C.POINTER(_lib.Light)()), 0),
    "light colour": (_scene, _set(lights__0__c__1=INF), 0),
    "light type": (_scene, _set(lights__0__type=4), 0),
    "map light without a slot": (lambda: _scene(lights=[ENV_LIGHT]), None, 0),
    "two map lights": (lambda: _env(lights=(ENV_LIGHT, ENV_LIGHT)), None, 0),
    # the materials
    "material colour": (_scene, _set(mats__0__k__0=NAN), 0),
    "glass colour": (lambda: _scene(materials=[[GLASS, -1, 1, 1, 1, 1, 1]]), None, 0),
    "glass eta": (lambda: _scene(materials=[[GLASS, 1, 1, 1, 1, 1, 1]], mat_eta=[0.5]), None, 0),
    "material type": (_scene, _set(mats__0__type=3), 0),
    "kd_tex range": (_scene, _set(mats__0__kd_tex=1), 0),
    "kd_tex names the map": (_env, _set(mats__0__kd_tex=1), 0),
    "kd_tex names the normals": (_normals, _set(mats__0__kd_tex=1), 0),
    "kd_tex names the filter": (_filtered, _set(mats__0__kd_tex=1), 0),
    # the view and the flags
    "camera": (_scene, _set(cam_to_world__3=NAN), 0),
    "fov": (_scene, _set(fov=180.0), 0),
    "crop": (_scene, _set(crop__1=1.5), 0),
    "unknown flag": (_scene, None, UNKNOWN_FLAG),
    "host and device build": (_scene, None, HOST_AND_GPU_BUILD),
    # the texture table: checkerboards
    "no texture table": (_scene, _set(n_textures=1), 0),
    "texture type": (_checker, _slot(0, _lib.Texture, type=7), 0),
    "texture mapping": (lambda: _checker(row=(0, 1, 1, 1, 0, 0, 0, NAN, 2, 0, 0)), None, 0),
    "texture colour": (lambda: _checker(row=(0, 1, NAN, 1, 0, 0, 0, 2, 2, 0, 0)), None, 0),
    "tri_uv missing": (_checker, _set(tri_uv=NO_FLOATS), 0),
    "tri_uv": (lambda: _checker(tri_uv=_with(UV, (1, 2), INF)), None, 0),
    # image textures
    "image size 0": (_image, _slot(0, _lib.ImageTexture, width=0), 0),
    "image side cap": (_image, _slot(0, _lib.ImageTexture, width=16385), 0),
    "image texel cap": (_image, _slot(0, _lib.ImageTexture, width=16384, height=8192), 0),
    "image wrap": (_image, _slot(0, _lib.ImageTexture, wrap=3), 0),
    "image filter": (_image, _slot(0, _lib.ImageTexture, filter=2), 0),
    "image mapping": (_image, _slot(0, _lib.ImageTexture, su=NAN), 0),
    "image without texels": (_image, _slot(0, _lib.ImageTexture, rgb=NO_FLOATS), 0),
    "image slots cap": (_scene, _table(*[_image_rec() for _ in range(65)]), 0),
    # (2^26 texels are allowed: five records of 2^24 pass the cap, four reach it)
    "image texels cap": (_scene, _table(*[_image_rec(16384, 1024) for _ in range(5)]), 0),
    "image texel": (lambda: _image(_with(np.full((2, 2, 3), 0.5), (1, 0, 2), -1.0)), None, 0),
    # the pixel filter
    "two filters": (_scene, _table(_filter_rec(), _filter_rec(1, 0.0)), 0),
    "filter kind": (_scene, _table(_filter_rec(9)), 0),
    "filter parameter": (_scene, _table(_filter_rec(3, NAN, 0.3)), 0),
    "filter alpha": (_scene, _table(_filter_rec(2, 0.0)), 0),
    "filter tau": (_scene, _table(_filter_rec(4, -1.0)), 0),
    # shading normals
    "two normals records": (_scene, _table(_normals_rec(), _normals_rec()), 0),
    "normals count": (_scene, _table(_normals_rec(3)), 0),
    "normals missing": (_normals, _slot(0, _lib.Normals, tri_n=NO_FLOATS), 0),
    "normal": (lambda: _normals(_with(TRI_N, (1, 4), NAN)), None, 0),
    # the environment map
    "map size 0": (_env, _slot(0, _lib.EnvMap, height=0), 0),
    "map texel cap": (_env, _slot(0, _lib.EnvMap, width=4097, height=4096), 0),
    "map without texels": (_env, _slot(0, _lib.EnvMap, rgb=NO_FLOATS), 0),
    "map texel": (lambda: _env(_with(np.full((2, 4, 3), 0.5), (1, 2, 0), -1.0)), None, 0),
    "map rotation not finite": (_env, _slot(0, _lib.EnvMap, world_to_light__4=INF), 0),
    "map rotation": (_env, _slot(0, _lib.EnvMap, world_to_light__0=2.0), 0),
    # ---- two faults: the first one named is the one reported ----
    "resolution, then flag": (_scene, _set(xres=0), UNKNOWN_FLAG),
    "light colour, then texture type": (_checker, _both(_set(lights__0__c__1=INF), _slot(0, _lib.Texture, type=7)), 0),
    "camera, then crop": (_scene, _set(cam_to_world__3=NAN, crop__1=1.5), 0),
    "kd_tex names the filter, then the filter's kind": (_filtered, _both(_set(mats__0__kd_tex=1), _slot(0, _lib.PixelFilter, kind=9)), 0),
    "two filters, then normals count": (_scene, _table(_filter_rec(), _filter_rec(), _normals_rec(3)), 0),
    "image texel, then tri_uv missing": (lambda: _image(_with(np.full((2, 2, 3), 0.5), (1, 0, 2), -1.0)), _set(tri_uv=NO_FLOATS), 0),
    "tri_uv missing, then flag": (_checker, _set(tri_uv=NO_FLOATS), UNKNOWN_FLAG),
    "flag, then sphere box": (lambda: _sphere(c=(3e38, 0, 0), r=3e38), None, UNKNOWN_FLAG),
    "light type, then map light without a slot": (lambda: _scene(lights=[[LIGHT_POINT, 0, 0, 3, 1, 1, 1], ENV_LIGHT]), _set(lights__0__type=4), 0),
    "map light without a slot, then material type": (lambda: _scene(lights=[ENV_LIGHT]), _set(mats__0__type=3), 0),
    # (pairs across every boundary between two stages of check_scene_desc)
    "vertex index, then light colour": (_scene, _set(idx__5=99, lights__0__c__1=INF), 0),
    "vertex index, then camera": (_scene, _set(idx__5=99, cam_to_world__3=NAN), 0),
    "light colour, then material colour": (_scene, _set(lights__0__c__1=INF, mats__0__k__0=NAN), 0),
    "glass eta, then crop": (lambda: _scene(materials=[[GLASS, 1, 1, 1, 1, 1, 1]], mat_eta=[0.5]), _set(crop__1=1.5), 0),
    "camera, then sphere material": (lambda: _sphere(mat=3), _set(cam_to_world__3=NAN), 0),
    "light colour, then no texture table": (_scene, _set(lights__0__c__1=INF, n_textures=1), 0),
    "sphere material, then no texture table": (lambda: _sphere(mat=3), _set(n_textures=1), 0),
    "no texture table, then light type": (_scene, _set(n_textures=1, lights__0__type=4), 0),
    "texture type, then material type": (_checker, _both(_slot(0, _lib.Texture, type=7), _set(mats__0__type=3)), 0),
    "flag, then light type": (_scene, _set(lights__0__type=4), UNKNOWN_FLAG),
    "flag, then material type": (_scene, _set(mats__0__type=3), UNKNOWN_FLAG),
    "sphere box, then light type": (lambda: _sphere(c=(3e38, 0, 0), r=3e38), _set(lights__0__type=4), 0),
    "two map lights, then material type": (lambda: _env(lights=(ENV_LIGHT, ENV_LIGHT)), _set(mats__0__type=3), 0),
}
EXPECTED = {
    'resolution': (INVALID, 'scene_create: resolution must be positive'),
    'mesh arrays': (INVALID, 'scene_create: missing mesh arrays'),
    'no materials': (INVALID, 'scene_create: no materials'),
    'materials cap': (LIMIT, 'scene_create: more than 65536 materials'),
    'triangles cap': (LIMIT, 'scene_create: more than 2^24 triangles (leaf references hold a 24-bit slot)'),
    'primitives cap': (LIMIT, 'scene_create: more than 2^24 primitives (triangles + spheres; leaf references hold a 24-bit slot)'),
    'no sphere table': (INVALID, 'scene_create: n_spheres > 0 but no sphere table'),
    'vertex index': (INVALID, 'scene_create: vertex index out of range'),
    'material id': (INVALID, 'scene_create: material id out of range'),
    'vertex': (INVALID, 'scene_create: vertex 1 is not finite'),
    'sphere radius': (INVALID, 'scene_create: sphere centre / radius must be finite and the radius positive'),
    'sphere material': (INVALID, 'scene_create: sphere material id out of range'),
    'sphere box': (INVALID, "scene_create: a sphere's bounding box is not finite"),
    'no light table': (INVALID, 'scene_create: n_lights > 0 but no light table'),
    'light colour': (INVALID, 'scene_create: light 0: position / direction / colour is not finite'),
    'light type': (INVALID, 'scene_create: unknown light type'),
    'map light without a slot': (INVALID, 'scene_create: light 0: an environment-map light (type 3) must name a type-1 slot of the texture table in `pad`'),
    'two map lights': (LIMIT, 'scene_create: more than one environment-map light (type 3)'),
    'material colour': (INVALID, 'scene_create: material 0: colour / emission is not finite'),
    'glass colour': (INVALID, 'scene_create: material 0: glass Kr / Kt must be finite and >= 0'),
    'glass eta': (INVALID, 'scene_create: material 0: glass eta (the float in kd_tex) must be finite and lie in [1, 16]'),
    'material type': (INVALID, 'scene_create: unknown material type'),
    'kd_tex range': (INVALID, 'scene_create: material texture number out of range'),
    'kd_tex names the map': (INVALID, 'scene_create: material 0: kd_tex names an environment map, which is not a texture for Kd'),
    'kd_tex names the normals': (INVALID, "scene_create: material 0: kd_tex names the shading normals' record, which is not a texture for Kd"),
    'kd_tex names the filter': (INVALID, "scene_create: material 0: kd_tex names the pixel filter's record, which is not a texture for Kd"),
    'camera': (INVALID, 'scene_create: camera matrix is not finite'),
    'fov': (INVALID, 'scene_create: fov must lie in (0, 180) degrees'),
    'crop': (INVALID, 'scene_create: crop window values must lie in [0, 1]'),
    'unknown flag': (INVALID, 'scene_create: unknown flag'),
    'host and device build': (INVALID, 'scene_create: PBRT_HIP_SCENE_HOST_BUILD / _OPTIMIZED_TREE are host builds, not combined with PBRT_HIP_SCENE_GPU_BUILD / _PLAIN_TREE'),
    'no texture table': (INVALID, 'scene_create: n_textures > 0 but no texture table'),
    'texture type': (INVALID, 'scene_create: unknown texture type'),
    'texture mapping': (INVALID, 'scene_create: texture mapping is not finite'),
    'texture colour': (INVALID, 'scene_create: texture colour is not finite'),
    'tri_uv missing': (INVALID, "scene_create: a triangle's material is textured but tri_uv is NULL"),
    'tri_uv': (INVALID, 'scene_create: tri_uv is not finite'),
    'image size 0': (INVALID, SLOT1 + 'image texture: width and height must be >= 1'),
    'image side cap': (LIMIT, SLOT1 + 'image texture: width or height above 16384'),
    'image texel cap': (LIMIT, SLOT1 + 'image texture: more than 2^26 texels'),
    'image wrap': (INVALID, SLOT1 + 'image texture: unknown wrap mode (0 repeat, 1 clamp, 2 black)'),
    'image filter': (INVALID, SLOT1 + 'image texture: unknown filter (0 point, 1 bilinear)'),
    'image mapping': (INVALID, SLOT1 + 'image texture: the mapping is not finite'),
    'image without texels': (INVALID, SLOT1 + 'image texture: no texels (rgb is NULL)'),
    'image slots cap': (LIMIT, 'scene_create: texture slot 65: more than 64 image textures'),
    'image texels cap': (LIMIT, 'scene_create: texture slot 5: the image textures hold more than 2^26 texels together'),
    'image texel': (INVALID, SLOT1 + 'image texture: texel 2 is not finite or is negative'),
    'two filters': (LIMIT, 'scene_create: texture slot 2: more than one pixel filter record (type 3)'),
    'filter kind': (INVALID, SLOT1 + 'pixel filter: unknown kind 9 (1 triangle, 2 gaussian, 3 mitchell, 4 sinc)'),
    'filter parameter': (INVALID, SLOT1 + 'pixel filter "mitchell": a parameter is not finite'),
    'filter alpha': (INVALID, SLOT1 + 'pixel filter "gaussian": alpha must be positive'),
    'filter tau': (INVALID, SLOT1 + 'pixel filter "sinc": tau must be positive'),
    'two normals records': (LIMIT, 'scene_create: texture slot 2: shading normals: more than one normals record (type 2)'),
    'normals count': (INVALID, SLOT1 + 'shading normals: n_tris is 3, the description has 2 triangles'),
    'normals missing': (INVALID, SLOT1 + 'shading normals: tri_n is NULL'),
    'normal': (INVALID, SLOT1 + 'shading normals: component 4 of triangle 1 is not finite'),
    'map size 0': (INVALID, SLOT1 + 'environment map: width and height must be >= 1'),
    'map texel cap': (LIMIT, SLOT1 + 'environment map: more than 2^24 texels'),
    'map without texels': (INVALID, SLOT1 + 'environment map: no texels (rgb is NULL)'),
    'map texel': (INVALID, SLOT1 + 'environment map: texel 6 is not finite or is negative'),
    'map rotation not finite': (INVALID, SLOT1 + 'environment map: world_to_light is not finite'),
    'map rotation': (INVALID, SLOT1 + 'environment map: world_to_light is not orthonormal to 1e-4 (a rotation is expected)'),
    'resolution, then flag': (INVALID, 'scene_create: resolution must be positive'),
    'light colour, then texture type': (INVALID, 'scene_create: light 0: position / direction / colour is not finite'),
    'camera, then crop': (INVALID, 'scene_create: camera matrix is not finite'),
    "kd_tex names the filter, then the filter's kind": (INVALID, "scene_create: material 0: kd_tex names the pixel filter's record, which is not a texture for Kd"),
    'two filters, then normals count': (LIMIT, 'scene_create: texture slot 2: more than one pixel filter record (type 3)'),
    'image texel, then tri_uv missing': (INVALID, SLOT1 + 'image texture: texel 2 is not finite or is negative'),
    'tri_uv missing, then flag': (INVALID, "scene_create: a triangle's material is textured but tri_uv is NULL"),
    'flag, then sphere box': (INVALID, 'scene_create: unknown flag'),
    'light type, then map light without a slot': (INVALID, 'scene_create: unknown light type'),
    'map light without a slot, then material type': (INVALID, 'scene_create: light 0: an environment-map light (type 3) must name a type-1 slot of the texture table in `pad`'),
    'vertex index, then light colour': (INVALID, 'scene_create: vertex index out of range'),
    'vertex index, then camera': (INVALID, 'scene_create: vertex index out of range'),
    'light colour, then material colour': (INVALID, 'scene_create: light 0: position / direction / colour is not finite'),
    'glass eta, then crop': (INVALID, 'scene_create: material 0: glass eta (the float in kd_tex) must be finite and lie in [1, 16]'),
    'camera, then sphere material': (INVALID, 'scene_create: camera matrix is not finite'),
    'light colour, then no texture table': (INVALID, 'scene_create: light 0: position / direction / colour is not finite'),
    'sphere material, then no texture table': (INVALID, 'scene_create: sphere material id out of range'),
    'no texture table, then light type': (INVALID, 'scene_create: n_textures > 0 but no texture table'),
    'texture type, then material type': (INVALID, 'scene_create: unknown texture type'),
    'flag, then light type': (INVALID, 'scene_create: unknown flag'),
    'flag, then material type': (INVALID, 'scene_create: unknown flag'),
    'sphere box, then light type': (INVALID, "scene_create: a sphere's bounding box is not finite"),
    'two map lights, then material type': (LIMIT, 'scene_create: more than one environment-map light (type 3)'),
}
assert set(EXPECTED) == set(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_refusal_is_the_recorded_one(name):
    make, edit, flags = CASES[name]
    assert _create(make(), edit, flags) == EXPECTED[name]


def test_sound_descriptions_are_not_refused_by_the_checks():
    """the scenes the cases start from pass every check: what is left is the device (none here, or a scene there)"""
    for make in (_scene, _sphere, _checker, _image, _env, _filtered, _normals):
        assert _create(make())[0] in (0, -2), make.__name__


# ---- the slot helpers of pbrt_amd/_lib.py, and the table fill_desc writes ----

def _distinct_records():
    floats = np.arange(12, dtype=np.float32)
    fp = floats.ctypes.data_as(C.POINTER(C.c_float))
    return floats, [
        _lib.Texture(type=_lib.SLOT_CHECKER, tex1=(0.25, 0.5, 0.75), tex2=(1.5, 2.5, 3.5), su=4.0, sv=5.0, du=-0.5, dv=0.125, pad=(11, 12, 13, 14, 15)),
        _lib.EnvMap(type=_lib.SLOT_ENVMAP, width=7, height=3, reserved=9, rgb=fp, world_to_light=tuple(0.5 * k for k in range(9)), pad=21),
        _lib.Normals(type=_lib.SLOT_NORMALS, n_tris=5, reserved=(31, 32), tri_n=fp, pad=tuple(range(40, 50))),
        _lib.PixelFilter(type=_lib.SLOT_FILTER, kind=3, param=(0.6, 0.15), pad=tuple(range(60, 72))),
        _lib.ImageTexture(type=_lib.SLOT_IMAGE, width=6, height=2, wrap=1, rgb=fp, su=2.0, sv=3.0, du=0.25, dv=0.75, filter=1, pad=(81, 82, 83, 84, 85)),
    ]


def _fields(rec):
    out = {}
    for name, _ in rec._fields_:
        v = getattr(rec, name)
        out[name] = C.cast(v, C.c_void_p).value if isinstance(v, C._Pointer) else (list(v) if isinstance(v, C.Array) else v)
    return out


def test_slot_helpers_round_trip_every_record_class():
    floats, records = _distinct_records()
    table = (_lib.Texture * len(records))()
    for i, rec in enumerate(records):
        _lib.put_slot(table, len(records) - 1 - i, rec)  # (not its own type's number)
    for i, rec in enumerate(records):
        back = _lib.read_slot(table, len(records) - 1 - i, type(rec))
        assert type(back) is type(rec) and _fields(back) == _fields(rec), type(rec).__name__
        assert back.type == table[len(records) - 1 - i].type == i
    assert _fields(records[1])["rgb"] == floats.ctypes.data  # (the comparison above saw pointers, not None)


def test_fill_desc_writes_rows_then_map_then_filter_then_normals():
    sd = _scene(lights=[ENV_LIGHT], envmap=np.full((2, 4, 3), 0.5, np.float32), pixel_filter="mitchell", tri_n=TRI_N, tri_uv=UV, mat_tex=[3],
                images=[ONE_TEXEL], textures=[[0, 1, 1, 1, 0, 0, 0, 2, 2, 0, 0], [0, 0, 1, 0, 1, 0, 1, 1, 1, 0, 0], api.image_texture_row(0, "clamp", "point")])
    desc = _lib.SceneDesc()
    keep = api.fill_desc(desc, sd, _lib.Material, _lib.Light, _lib.Sphere, _lib.Texture)
    assert keep and desc.n_textures == 6
    assert [desc.textures[i].type for i in range(6)] == [0, 0, 4, 1, 3, 2]
    assert np.array([desc.lights[0].pad], np.float32).view(np.uint32)[0] == 4
    im, env = _lib.read_slot(desc.textures, 2, _lib.ImageTexture), _lib.read_slot(desc.textures, 3, _lib.EnvMap)
    assert (im.width, im.height, im.wrap, im.filter) == (1, 1, api.WRAP_CLAMP, api.TEXFILTER_POINT) and (env.width, env.height) == (4, 2)
    assert _lib.read_slot(desc.textures, 4, _lib.PixelFilter).kind == api.FILTER_MITCHELL and _lib.read_slot(desc.textures, 5, _lib.Normals).n_tris == 2
    assert _create(sd)[0] in (0, -2)


# ---- pbrt_amd/csrc/texture_table.hpp in a stand-alone program (plain g++, nothing of HIP) ----
PROGRAM = r"""
#include <stdio.h>
#include "texture_table.hpp"
using namespace pbrt_hip;
static const char *kNames[] = {"checker", "envmap", "normals", "filter", "image", "unknown", "none", "out-of-range"};
int main() {
  static float texels[6] = {0.5f, 1.5f, 2.5f, 3.5f, 4.5f, 5.5f};
  pbrt_hip_texture ck{};
  ck.tex1[1] = 0.25f; ck.tex2[2] = 0.75f; ck.su = 2.f; ck.dv = -1.f;
  pbrt_hip_envmap env{};
  env.width = 2; env.height = 1; env.rgb = texels; env.world_to_light[4] = 1.f;
  pbrt_hip_normals nrm{};
  nrm.n_tris = 7; nrm.tri_n = texels + 1;
  pbrt_hip_pixel_filter flt{};
  flt.kind = PBRT_HIP_FILTER_SINC; flt.param[0] = 3.f;
  pbrt_hip_image_texture img{};
  img.width = 1; img.height = 2; img.wrap = PBRT_HIP_WRAP_BLACK; img.filter = PBRT_HIP_TEXFILTER_BILINEAR; img.rgb = texels; img.sv = 4.f;
  pbrt_hip_pixel_filter second = flt;
  second.kind = PBRT_HIP_FILTER_TRIANGLE;
  pbrt_hip_texture odd{};
  odd.type = 9u;
  // (a kind is not its slot's number here)
  const pbrt_hip_texture slots[7] = {write_slot(img), write_slot(flt), write_slot(ck), write_slot(nrm), write_slot(env), write_slot(second), odd};
  pbrt_hip_material mats[2] = {};
  mats[1].kd_tex = 3u;
  const uint16_t mat_id[2] = {0, 1};
  pbrt_hip_sphere ball{};
  pbrt_hip_scene_desc d{};
  d.textures = slots; d.n_textures = 7; d.mats = mats; d.n_mats = 2; d.mat_id = mat_id; d.n_tris = 2; d.spheres = &ball; d.n_spheres = 1;
  const TextureTable t = decode_texture_table(d);
  printf("kinds");
  for (SlotKind k : t.kinds) printf(" %s", kNames[(int)k]);
  printf("\nnamed %s %s %s\n", kNames[(int)t.named(0)], kNames[(int)t.named(5)], kNames[(int)t.named(8)]);
  printf("filter %d kind %u param %g\n", (int)t.filter.has_value(), t.filter->kind, t.filter->param[0]);
  printf("normals %d n_tris %u first %g\n", (int)t.normals.has_value(), t.normals->n_tris, t.normals->tri_n[0]);
  printf("images %zu slot %u size %ux%u wrap %u filter %u sv %g\n", t.images.size(), t.images[0].slot, t.images[0].rec.width, t.images[0].rec.height, t.images[0].rec.wrap,
         t.images[0].rec.filter, t.images[0].rec.sv);
  printf("envmap %d %d size %ux%u m4 %g\n", (int)t.envmap(5).has_value(), (int)t.envmap(3).has_value(), t.envmap(5)->width, t.envmap(5)->height, t.envmap(5)->world_to_light[4]);
  printf("textured %d %d\n", (int)t.textured_tris, (int)t.textured_sph);
  const pbrt_hip_texture c2 = read_slot<pbrt_hip_texture>(slots, 2);
  const pbrt_hip_envmap e2 = read_slot<pbrt_hip_envmap>(slots, 4);
  const pbrt_hip_normals n2 = read_slot<pbrt_hip_normals>(slots, 3);
  const pbrt_hip_pixel_filter f2 = read_slot<pbrt_hip_pixel_filter>(slots, 5);
  const pbrt_hip_image_texture i2 = read_slot<pbrt_hip_image_texture>(slots, 0);
  printf("read checker %u %g %g %g %g\n", c2.type, c2.tex1[1], c2.tex2[2], c2.su, c2.dv);
  printf("read envmap %u %u %u %g %g\n", e2.type, e2.width, e2.height, e2.rgb[5], e2.world_to_light[4]);
  printf("read normals %u %u %g\n", n2.type, n2.n_tris, n2.tri_n[4]);
  printf("read filter %u %u %g\n", f2.type, f2.kind, f2.param[0]);
  printf("read image %u %u %u %u %u %g %g\n", i2.type, i2.width, i2.height, i2.wrap, i2.filter, i2.sv, i2.rgb[2]);
  return 0;
}
"""
PROGRAM_PRINTS = """kinds image filter checker normals envmap filter unknown
named none envmap out-of-range
filter 1 kind 4 param 3
normals 1 n_tris 7 first 1.5
images 1 slot 0 size 1x2 wrap 2 filter 1 sv 4
envmap 1 0 size 2x1 m4 1
textured 1 0
read checker 0 0.25 0.75 2 -1
read envmap 1 2 1 5.5 1
read normals 2 7 5.5
read filter 3 1 3
read image 4 1 2 2 1 4 2.5
"""


def test_texture_table_header_stands_alone(tmp_path):
    """one slot of each kind (and a second filter, and a slot of no kind) written with write_slot, decoded in one pass, read back with read_slot"""
    src, exe = tmp_path / "table.cpp", tmp_path / "table"
    src.write_text(PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "pbrt_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout == PROGRAM_PRINTS
