"""The three small descriptions whose device tables are held word for word (tests/test_scene_tables_host.py against
tests/golden/scene_tables.npz, which tests/golden/make_golden_scene_tables.py records), and the call of pbrt_hip_scene_tables_host that
returns a description's tables as uint32 arrays.  Host code alone: no GPU is asked for."""
import ctypes as C

import numpy as np

from pbrt_amd import GLASS, LIGHT_DISTANT, LIGHT_ENVMAP, LIGHT_INFINITE, LIGHT_POINT, MATTE, MIRROR, SceneData, _lib, api

SCALARS = ("le_inf", "has_inf", "env", "has_spot", "has_mapped", "env_w", "env_h", "env_m", "env_c")


def scene_a():
    """the PLS family: every light kind but the environment map, emissive triangles (one of no area), a mesh triangle and a sphere, a material
    of every type, and a table of checker, 2 x 2 image, cone, projection map, goniometric map"""
    P = np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0],            # a floor quad: triangles 0, 1 (matte with kd_tex, mirror)
                  [-0.5, 1.5, -0.25], [0.25, 1.5, 0.5], [0.5, 1.75, -0.5],   # emissive triangle 2
                  [2, 0, 1], [2, 1, 1.5], [2.5, 0.25, 3],                    # emissive triangle 3
                  [3, 3, 3], [4, 4, 4], [5, 5, 5],                           # emissive triangle 4: collinear corners, no area
                  [-2, 0, 0], [-2, 1, 0], [-2, 0, 1]], np.float32)           # triangles 5 .. 7: glass, plastic, substrate
    idx = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [7, 8, 9], [10, 11, 12], [13, 14, 15], [13, 15, 14], [14, 13, 15]], np.uint32)
    mat_id = np.array([1, 2, 0, 0, 0, 3, 4, 5], np.uint16)
    plastic, plastic_alpha = api.plastic_material(kd=(0.3, 0.2, 0.1), ks=(0.25, 0.5, 0.75), roughness=0.2)
    substrate, substrate_alpha = api.substrate_material(kd=(0.4, 0.5, 0.6), ks=(0.125, 0.25, 1.0), uroughness=0.3, vroughness=0.05)
    materials = [[MATTE, 0.75, 0.5, 0.25, 3.0, 2.0, 1.5],       # emissive matte
                 [MATTE, 0.5, 0.5, 0.5, 0, 0, 0],                # matte with kd_tex (the checker)
                 [MIRROR, 0.9, 0.8, 0.7, 0, 0, 0],
                 [GLASS, 0.95, 0.9, 0.85, 0.6, 0.7, 0.8],
                 plastic, substrate]
    mat_eta = np.array([0, 0, 0, 1.33, plastic_alpha, substrate_alpha], np.float32)
    rot = np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0]], np.float32)
    spot, cone = api.spot_light((0.5, 2.5, 1.5), (0.25, 0.0, 0.5), I=(4, 5, 6), coneangle=35.0, conedeltaangle=10.0)
    proj, proj_map = api.projection_light((1, 2, 3), 2, I=(7, 8, 9), fov=50.0, aspect=1.5, world_to_light=rot)
    gonio, gonio_map = api.goniometric_light((-1, 2, 0.5), 2, I=(0.5, 0.25, 0.125), world_to_light=rot.T)
    lights = [[LIGHT_POINT, 0.1, 0.2, 3, 1, 2, 3], [LIGHT_DISTANT, 0, 0.6, 0.8, 0.5, 0.6, 0.7], [LIGHT_INFINITE, 0, 0, 0, 0.01, 0.02, 0.03], spot, proj, gonio]
    image = np.arange(12, dtype=np.float32).reshape(2, 2, 3) / 16
    return SceneData(P=P, idx=idx, mat_id=mat_id, materials=materials, mat_eta=mat_eta, lights=lights, spheres=[[0, 0, 1, 0.5, 2]], xres=8, yres=8,
                     mat_tex=[0, 1, 0, 0, 0, 0], textures=[[0, 1, 0.5, 0.25, 0, 0.125, 0.75, 2, 3, 0.5, 0.25], api.image_texture_row(0, mapping=(2.0, 1.0, 0.5, 0.0))],
                     tri_uv=np.tile(np.array([0, 0, 1, 0, 1, 1], np.float32), (8, 1)), images=[image], spot_cones=[cone], light_maps=[proj_map, gonio_map]).normalized()


def scene_b():
    """spheres only -- no triangle: the caller's vertices are dropped --, an environment-map light over a 2 x 2 map, matte and mirror"""
    sky = np.array([[[1, 2, 3], [0.5, 0.25, 0.125]], [[0, 0.5, 1], [4, 2, 1]]], np.float32)
    return SceneData(P=np.array([[9, 9, 9], [8, 8, 8]], np.float32), materials=[[MATTE, 0.5, 0.25, 0.75, 0, 0, 0], [MIRROR, 0.9, 0.9, 0.9, 0, 0, 0]],
                     lights=[[LIGHT_ENVMAP, 0, 0, 0, 2, 1, 0.5]], spheres=[[0, 0, 1, 0.5, 0], [1.5, -0.25, 0.75, 0.25, 1]], xres=8, yres=8, envmap=sky,
                     envmap_world_to_light=np.array([[0, 1, 0], [0, 0, 1], [1, 0, 0]], np.float32)).normalized()


def scene_c():
    """two matte triangles and a point light: no extra rows, no texture rows, no texels"""
    return SceneData(P=np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], np.float32), idx=np.array([[0, 1, 2], [0, 2, 3]], np.uint32),
                     mat_id=np.zeros(2, np.uint16), materials=[[MATTE, 0.5, 0.5, 0.5, 0, 0, 0]], lights=[[LIGHT_POINT, 0, 0, 3, 1, 1, 1]], xres=8, yres=8).normalized()


CASES = {"A": scene_a, "B": scene_b, "C": scene_c}


def tables(sd):
    """-> {name: uint32 array} of everything pbrt_hip_scene_tables_host reports for `sd`: the arrays as their words, each scalar as the words of
    its float32 / uint32 value(s)"""
    desc = _lib.SceneDesc()
    keep = api.fill_desc(desc, sd, _lib.Material, _lib.Light, _lib.Sphere)
    out = _lib.SceneTables()
    _lib.check(_lib.lib().pbrt_hip_scene_tables_host(C.byref(desc), C.byref(out)), "pbrt_hip_scene_tables_host")  # the counts
    arrays = {a: np.zeros(getattr(out, "n_" + a), np.uint32) for a in _lib.SceneTables.ARRAYS}
    for a, v in arrays.items():
        setattr(out, a, v.ctypes.data_as(C.POINTER(C.c_uint32)))
    _lib.check(_lib.lib().pbrt_hip_scene_tables_host(C.byref(desc), C.byref(out)), "pbrt_hip_scene_tables_host")
    del keep
    for s in SCALARS:
        v = getattr(out, s)
        arrays[s] = np.array(list(v), np.float32).view(np.uint32) if hasattr(v, "__len__") else np.array([v], np.uint32)
    return arrays
