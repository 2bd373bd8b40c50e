"""The small device tables of a scene -- lights, mats, mat_extra, spheres, with the builders' arrays and the texture rows beside them -- as
scene creation's gather stage assembles them on the host (pbrt_hip_scene_tables_host: no GPU is asked for).  Three witnesses: the words
that the commit before pbrt_amd/csrc/scene_tables.hpp computed for three small descriptions (tests/golden/scene_tables.npz), the rows of
every kind of light and material restated here from DESIGN.md section 4, and the header compiled alone under plain g++."""
import os
import subprocess

import numpy as np
import pytest

import scene_tables_cases as cases
from spot_host_build import STUB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, U32 = np.float32, np.uint32


@pytest.fixture(scope="module")
def scenes():
    return {name: make() for name, make in cases.CASES.items()}


@pytest.fixture(scope="module")
def tables(scenes):
    return {name: cases.tables(sd) for name, sd in scenes.items()}


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_tables_are_the_parents_word_for_word(tables, name):
    golden = np.load(os.path.join(ROOT, "tests", "golden", "scene_tables.npz"))
    keys = sorted(k.split("/", 1)[1] for k in golden.files if k.startswith(name + "/"))
    assert keys == sorted(tables[name]) and len(keys) == 18
    for key in keys:
        want, got = golden[f"{name}/{key}"], tables[name][key]
        assert want.dtype == U32 and got.dtype == U32
        assert got.shape == want.shape and np.array_equal(got, want), key  # (as words: a NaN row must be the same NaN)


def test_what_the_cases_cover(tables):
    a, b, c = (tables[n] for n in "ABC")
    assert a["lights"].size == 4 * 5 * 9 and list(a["lights"][::20]) == [0, 1, 2, 5, 6, 7, 3, 3, 3]  # six explicit lights, then three emissive triangles
    nrm = a["lights"].reshape(-1, 5, 4)[8, 4].view(F32)
    assert np.isnan(nrm[:3]).all() and nrm[3] == 0  # the triangle of no area
    assert list(a["mats"][::8]) == [0, 0, 1, 2, 3, 4] and a["mat_extra"].size == 4 * 6 and a["textures"].size == 4 * 3 * 5 and a["image_texels"].size == 4 * 4
    assert [int(a[k][0]) for k in ("has_inf", "env", "has_spot", "has_mapped")] == [1, 0, 1, 1]
    assert b["P"].size == 3 * 4 and b["idx"].size == 6 and list(b["lights"][::20]) == [4] and [int(b[k][0]) for k in ("env", "env_w", "env_h")] == [1, 2, 2]
    assert c["lights"].size == 20 and all(c[k].size == 0 for k in ("mat_extra", "textures", "image_texels", "spheres"))


# ---- the rows restated, in float32 operation by operation ----

def _bits(u):
    return np.array([u], U32).view(F32)[0]


def _row(*v):
    return np.array(v, F32)


ZERO = _row(0, 0, 0, 0)


def _plain(dev_type, l):
    return [_row(_bits(dev_type), *l[1:4]), ZERO, ZERO, _row(*l[4:7], 0), ZERO]


def _spot(l, cone):
    return [_row(_bits(5), *l[1:4]), _row(*cone[0:4]), _row(cone[4], 0, 0, 0), _row(*l[4:7], 0), ZERO]


def _mapped(l, m):
    kind, image, M = int(m[0]), int(m[1]), m[2:11]
    return [_row(_bits(6 + kind), *l[1:4]), _row(*M[0:3], m[11]), _row(*M[3:6], m[12]), _row(*l[4:7], _bits(image - 1)), _row(*M[6:9], m[13])]


def _triangle(p0, p1, p2, le):
    a, b = p1 - p0, p2 - p0
    cr = np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], F32)
    ln = np.sqrt(F32((cr[0] * cr[0] + cr[1] * cr[1]) + cr[2] * cr[2]))
    with np.errstate(invalid="ignore"):
        n = cr / ln
    return [_row(_bits(3), *p0), _row(*p1, F32(0.5) * ln), _row(*p2, 0), _row(*le, 0), _row(*n, 0)]


def _expected_lights(sd):
    rows, n_spot, n_mapped = [], 0, 0
    for l in sd.lights:
        t = int(l[0])
        if t == 5:
            rows += _spot(l, sd.spot_cones[n_spot])
            n_spot += 1
        elif t == 6:
            rows += _mapped(l, sd.light_maps[n_mapped])
            n_mapped += 1
        else:
            rows += _plain(4 if t == 3 else t, l)
    for tri, m in zip(sd.idx, sd.mat_id):
        mat = sd.materials[m]
        if int(mat[0]) in (0, 1) and (mat[4:7] > 0).any():  # (glass, plastic and substrate keep a parameter where the others keep le)
            rows += _triangle(*(sd.P[v] for v in tri), mat[4:7])
    return np.array(rows, F32)


def test_light_rows_of_every_kind_restated(scenes, tables):
    """five rows per light: point, distant, infinite, spot, projection, goniometric and three emissive triangles in A, the environment map in B"""
    seen = set()
    for name in "ABC":
        want, got = _expected_lights(scenes[name]), tables[name]["lights"].reshape(-1, 4)
        assert got.shape == want.shape
        nan = np.isnan(want)  # (0 / 0 of the triangle without area: that it is NaN is restated, which NaN the golden says)
        assert np.array_equal(np.isnan(got.view(F32)), nan)
        assert np.array_equal(got[~nan], want.view(U32)[~nan])
        seen |= set(int(t) for t in got[::5, 0])
    assert seen == set(range(8))


def test_material_rows_of_every_type_restated(scenes, tables):
    """two rows per material, and a row of mat_extra per material once the scene has glass, plastic or substrate"""
    seen = set()
    for name in "ABC":
        sd = scenes[name]
        mats, extra = [], []
        for m, tex, eta in zip(sd.materials, sd.mat_tex, sd.mat_eta if len(sd.mat_eta) else np.zeros(len(sd.materials), F32)):
            t = int(m[0])
            seen.add(t)
            mats.append(_row(_bits(t), *m[1:4]))
            mats.append(ZERO if t >= 2 else _row(*m[4:7], _bits(int(tex) if t == 0 else 0)))
            extra.append(_row(*m[4:7], eta) if t >= 2 else _row(0, 0, 0, 1))
        if not any(int(m[0]) >= 2 for m in sd.materials):
            extra = []
        assert np.array_equal(tables[name]["mats"], np.array(mats, F32).view(U32).reshape(-1))
        assert np.array_equal(tables[name]["mat_extra"], np.array(extra, F32).view(U32).reshape(-1))
        spheres = [r for s in sd.spheres for r in (_row(*s[0:4]), _row(_bits(int(s[4])), 0, 0, 0))]
        assert np.array_equal(tables[name]["spheres"], np.array(spheres, F32).view(U32).reshape(-1))
    assert seen == set(range(5))


# ---- pbrt_amd/csrc/scene_tables.hpp alone: plain g++, the few-line <hip/hip_runtime.h> of the host builds ----

PROGRAM = r"""#include <cstdio>
#include "scene_tables.hpp"
using namespace pbrt_hip;
struct Scene { const float4 *lights; };
int main() {
  static_assert(kLightRows == 5 && kMatRows == 2 && kSphereRows == 2, "row counts");
  static_assert(dev_light_type(PBRT_HIP_LIGHT_ENVMAP) == kDevLightEnv && dev_light_type(PBRT_HIP_LIGHT_MAPPED, 1u) == kDevLightGonio, "device words");
  static_assert(mat_is_matte(0u) && mat_is_glass(2u) && mat_is_coated(3u) && mat_is_coated(4u) && mat_is_substrate(4u) && !mat_is_coated(1u) && mat_has_extra(2u) && !mat_has_extra(1u), "predicates");
  std::vector<float4> t;
  const float p[3] = {1, 2, 3}, c[3] = {4, 5, 6}, p0[3] = {0, 0, 0}, p1[3] = {2, 0, 0}, p2[3] = {0, 2, 0};
  pbrt_hip_spot_cone cone{};
  cone.axis[2] = -1.f; cone.cos_total = 0.5f; cone.cos_start = 0.75f;
  pbrt_hip_light_map map{};
  map.kind = PBRT_HIP_LIGHT_MAP_GONIOMETRIC; map.image = 3u;
  for (int k = 0; k < 9; k++) map.world_to_light[k] = (float)k;
  push_light_plain(&t, dev_light_type(PBRT_HIP_LIGHT_ENVMAP), p, c);
  push_light_spot(&t, p, c, cone);
  push_light_mapped(&t, p, c, map);
  push_light_triangle(&t, p0, p1, p2, c);
  const Scene S = {t.data()};
  printf("rows %zu\n", t.size());
  for (uint32_t li = 0; li < 4; li++) printf("light %u type %u row3 %g %g\n", li, light_type(S, li), light_row(S, li, 3u).x, light_row(S, li, 3u).w);
  printf("same row %d\n", (int)(&light_row(S, 2u, 1u) == t.data() + 11));
  printf("cone %g %g slot %u\n", light_row(S, 1u, 1u).w, light_row(S, 1u, 2u).x, table_bits(light_row(S, 2u, 3u).w));
  printf("triangle area %g n %g %g %g\n", light_row(S, 3u, 1u).w, light_row(S, 3u, 4u).x, light_row(S, 3u, 4u).y, light_row(S, 3u, 4u).z);
  pbrt_hip_material glass{};
  glass.type = PBRT_HIP_MATERIAL_GLASS; glass.le[1] = 0.5f; glass.kd_tex = table_bits(1.5f);
  float4 rows[2];
  std::vector<float4> extra;
  write_material(rows, &extra, 1u, 3u, glass);
  printf("glass %u le %g extra %zu %g %g %g\n", table_bits(rows[0].x), rows[1].y, extra.size(), extra[1].y, extra[1].w, extra[2].w);
  return 0;
}
"""
PROGRAM_PRINTS = """rows 20
light 0 type 4 row3 4 0
light 1 type 5 row3 4 0
light 2 type 7 row3 4 2.8026e-45
light 3 type 3 row3 4 0
same row 1
cone 0.5 0.75 slot 2
triangle area 2 n 0 0 1
glass 2 le 0 extra 3 0.5 1.5 1
"""


def test_scene_tables_header_stands_alone(tmp_path):
    """the header's static_asserts hold, its writers and readers agree, and nothing of HIP beyond the float4 type is needed"""
    os.makedirs(tmp_path / "stub" / "hip")
    (tmp_path / "stub" / "hip" / "hip_runtime.h").write_text(STUB)
    src, exe = tmp_path / "tables.cpp", tmp_path / "tables"
    src.write_text(PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-I", str(tmp_path / "stub"), "-I", os.path.join(ROOT, "pbrt_amd", "csrc"), str(src), "-o",
                    str(exe)], check=True)
    assert subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout == PROGRAM_PRINTS
