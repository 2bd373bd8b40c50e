"""`.pbrt` scene ingestion through the C ABI (pbrt_hip_load_file / pbrt_hip_load_string): the
reference's tokenizer + parameter lists + API state machine (src/core/parser.rs, src/core/api.rs),
completed in C++ (csrc/scene_parser.cpp) for the directives this path covers."""
import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from ._lib import (SLOT_ENVMAP, SLOT_FILTER, SLOT_IMAGE, SLOT_LIGHT_MAP, SLOT_NORMALS, SLOT_SPOT, EnvMap, ImageTexture, LightMap, Normals, PixelFilter, RenderDesc, SceneDesc,
                   SpotCone, check, lib, read_slot)
from .api import GLASS, LIGHT_MAPPED, LIGHT_SPHERE, LIGHT_SPOT, PLASTIC, SUBSTRATE, SceneData


@dataclass
class LoadedScene:
    scene: SceneData
    integrator: int
    max_depth: int
    spp: tuple
    filename: str
    warnings: list = field(default_factory=list)
    ctm: np.ndarray = None      # CTM when parsing stopped
    names: dict = None          # camera / sampler / integrator / filter / accelerator / film names as given
    film_scale: float = 1.0     # Film "float scale" (film.rs:368-371): pass to film_to_rgb
    sampler: int = 0            # PBRT_HIP_SAMPLER_*
    filter_width: tuple = (0.5, 0.5)
    max_sample_luminance: float = 0.0  # Film "float maxsampleluminance" (film.rs:75,279); 0 = none

    def render_kwargs(self):
        return dict(integrator=self.integrator, max_depth=self.max_depth, spp=self.spp, sampler=self.sampler,
                    filter_width=self.filter_width, max_sample_luminance=self.max_sample_luminance)


def _collect(h):
    l = lib()
    try:
        d, r = SceneDesc(), RenderDesc()
        fn = C.create_string_buffer(4096)
        check(l.pbrt_hip_loaded_get(h, C.byref(d), C.byref(r), fn, len(fn)), "pbrt_hip_loaded_get")

        def arr(ptr, n, dt):
            return np.ctypeslib.as_array(ptr, shape=(n,)).astype(dt).copy() if n else np.zeros(0, dt)

        # The texture table, classified once by the slots' first words.  The map's record becomes SceneData's `envmap`, the
        # normals' (3.18) `tri_n`, the pixel filter's (3.19) `pixel_filter`; every other slot stays a `textures` row -- numbered as it is while
        # the records' slots come last, as the parser leaves them unless a texture is declared after the light (such a scene's texture numbers
        # are remapped here).  An image's texels (3.20) join `images`, and its row -- in the slot's own place -- names them.
        slots = {}
        for i in range(d.n_textures):
            slots.setdefault(d.textures[i].type, []).append(i)

        def first(kind, cls):
            return read_slot(d.textures, slots[kind][0], cls) if kind in slots else None

        tex_slots = sorted(i for kind, at in slots.items() if kind not in (SLOT_ENVMAP, SLOT_NORMALS, SLOT_FILTER, SLOT_SPOT, SLOT_LIGHT_MAP) for i in at)
        renum = {0: 0, **{i + 1: k + 1 for k, i in enumerate(tex_slots)}}
        e, nr, pf = first(SLOT_ENVMAP, EnvMap), first(SLOT_NORMALS, Normals), first(SLOT_FILTER, PixelFilter)
        envmap = arr(e.rgb, 3 * e.width * e.height, np.float32).reshape(e.height, e.width, 3) if e else np.zeros((0, 0, 3), np.float32)
        env_m = np.array(list(e.world_to_light), np.float32).reshape(3, 3) if e else np.eye(3, dtype=np.float32)
        tri_n = arr(nr.tri_n, 9 * nr.n_tris, np.float32).reshape(-1, 9) if nr else np.zeros((0, 9), np.float32)
        pixel_filter = (int(pf.kind), float(pf.param[0]), float(pf.param[1])) if pf else None
        images = []

        def tex_row(i):
            if i not in slots.get(SLOT_IMAGE, ()):
                t = d.textures[i]
                return [t.type, *t.tex1, *t.tex2, t.su, t.sv, t.du, t.dv]
            im = read_slot(d.textures, i, ImageTexture)
            images.append(arr(im.rgb, 3 * im.width * im.height, np.float32).reshape(im.height, im.width, 3))
            return [SLOT_IMAGE, len(images) - 1, im.wrap, im.filter, 0, 0, 0, im.su, im.sv, im.du, im.dv]

        tex_rows = [tex_row(i) for i in tex_slots]
        # a spot light's `pad` holds the bits of its cone's slot number: the cones in the order of their lights
        cones = []
        for i in range(d.n_lights):
            if d.lights[i].type == LIGHT_SPOT:
                c = read_slot(d.textures, int(np.array([d.lights[i].pad], np.float32).view(np.uint32)[0]) - 1, SpotCone)
                cones.append([*c.axis, c.cos_total, c.cos_start])
        # a mapped light's likewise, of its record's slot (3.23): the records in the order of their lights, their images renumbered as rows
        maps = []
        for i in range(d.n_lights):
            if d.lights[i].type == LIGHT_MAPPED:
                m = read_slot(d.textures, int(np.array([d.lights[i].pad], np.float32).view(np.uint32)[0]) - 1, LightMap)
                maps.append([m.kind, renum[m.image], *m.world_to_light, m.inv_tan, m.sx, m.sy])
        sd = SceneData(
            light_maps=np.array(maps, np.float32).reshape(-1, 14),
            spot_cones=np.array(cones, np.float32).reshape(-1, 5),
            images=images, pixel_filter=pixel_filter, tri_n=tri_n, envmap=envmap, envmap_world_to_light=env_m,
            P=arr(d.P, 3 * d.n_verts, np.float32).reshape(-1, 3), idx=arr(d.idx, 3 * d.n_tris, np.uint32).reshape(-1, 3),
            mat_id=arr(d.mat_id, d.n_tris, np.uint16),
            materials=np.array([[d.mats[i].type, *d.mats[i].k, *d.mats[i].le] for i in range(d.n_mats)], np.float32).reshape(-1, 7),
            # (a sphere light's `pad` holds the bits of its sphere's 1-based number, DESIGN.md 3.25: the row's first word is the 0-based row)
            lights=np.array([[d.lights[i].type, *([int(np.array([d.lights[i].pad], np.float32).view(np.uint32)[0]) - 1, 0, 0] if d.lights[i].type == LIGHT_SPHERE
                                                  else d.lights[i].p), *d.lights[i].c] for i in range(d.n_lights)], np.float32).reshape(-1, 7),
            spheres=np.array([[*d.spheres[i].c, d.spheres[i].r, d.spheres[i].mat] for i in range(d.n_spheres)], np.float32).reshape(-1, 5),
            cam_to_world=np.array(list(d.cam_to_world), np.float32).reshape(4, 4), fov=d.fov, xres=d.xres, yres=d.yres,
            crop=tuple(d.crop),
            # (a glass row's kd_tex holds eta, a plastic or a substrate row's alpha: DESIGN.md 3.16, 3.21, 3.24)
            mat_tex=np.array([0 if d.mats[i].type in (GLASS, PLASTIC, SUBSTRATE) else renum[d.mats[i].kd_tex] for i in range(d.n_mats)], np.uint32),
            mat_eta=(np.array([d.mats[i].kd_tex if d.mats[i].type in (GLASS, PLASTIC, SUBSTRATE) else 0x3FC00000 for i in range(d.n_mats)], np.uint32).view(np.float32)
                     if any(d.mats[i].type in (GLASS, PLASTIC, SUBSTRATE) for i in range(d.n_mats)) else np.zeros(0, np.float32)),
            textures=np.array(tex_rows, np.float32).reshape(-1, 11),
            tri_uv=(arr(d.tri_uv, 6 * d.n_tris, np.float32).reshape(-1, 6) if d.tri_uv else np.zeros((0, 6), np.float32))).normalized()
        wbuf = C.create_string_buffer(1 << 16)
        nw = l.pbrt_hip_loaded_warnings(h, wbuf, len(wbuf))
        ctm = np.zeros(16, np.float32)
        names = C.create_string_buffer(1024)
        check(l.pbrt_hip_loaded_state(h, ctm.ctypes.data_as(C.POINTER(C.c_float)), names, len(names)), "pbrt_hip_loaded_state")
        keys = ("camera", "sampler", "integrator", "filter", "accelerator", "film")
        return LoadedScene(sd, r.integrator, r.max_depth, (r.spp_x, r.spp_y), fn.value.decode(),
                           [w for w in wbuf.value.decode().split("\n") if w][:nw], ctm.reshape(4, 4),
                           dict(zip(keys, names.value.decode().split(" "))),
                           film_scale=float(l.pbrt_hip_loaded_film_scale(h)), sampler=int(r.sampler),
                           filter_width=(float(r.filter_xwidth), float(r.filter_ywidth)),
                           max_sample_luminance=float(r.max_sample_luminance))
    finally:
        l.pbrt_hip_loaded_free(h)


def load_file(path):
    h = C.c_void_p()
    check(lib().pbrt_hip_load_file(str(path).encode(), C.byref(h)), "pbrt_hip_load_file")
    return _collect(h)


def load_string(text, base_dir=None):
    b = text.encode() if isinstance(text, str) else text
    h = C.c_void_p()
    check(lib().pbrt_hip_load_string(b, len(b), base_dir.encode() if base_dir else None, C.byref(h)), "pbrt_hip_load_string")
    return _collect(h)


def tokenize(text):
    """parser.rs Tokenizer: -> (tokens, ok).  ok is False when the stream ends in an error."""
    b = text.encode() if isinstance(text, str) else text
    buf = C.create_string_buffer(len(b) * 2 + 16)
    n = lib().pbrt_hip_tokenize(b, len(b), buf, len(buf))
    toks = [t for t in buf.value.decode().split("\n") if t]
    return toks, n >= 0
