// texture_table.hpp -- THE reader and writer of pbrt_hip_scene_desc.textures.  A slot of that table is 64 bytes whose first word says
// which of seven records it is (include/pbrt_hip.h); the table's element type is 4-aligned while two records hold a pointer, so a slot is
// read and written with memcpy -- here, and nowhere else under csrc.  read_slot / write_slot move one record; TextureTable is a
// description's table decoded in one pass, which the stages of scene creation (capi_scene.cpp) ask instead of walking the table again.
// Plain C++17, nothing of HIP.
#pragma once
#include <stdint.h>

#include <cstring>
#include <optional>
#include <vector>

#include "../../include/pbrt_hip.h"

namespace pbrt_hip {

// what a slot is: its first word (0 and 1 have no name in the public header); anything else is kUnknown, which scene creation refuses.
// The kinds up to kImage ARE their first word; a spot light's cone (first word 6; 5 is no kind) stands behind the three
// that are no record at all, whose numbers callers of this header hold: slot_type_word() is the kind's first word.
enum class SlotKind : uint32_t {
  kChecker = 0u,
  kEnvmap = 1u,
  kNormals = PBRT_HIP_TEXTURE_NORMALS,
  kFilter = PBRT_HIP_TEXTURE_FILTER,
  kImage = PBRT_HIP_TEXTURE_IMAGE,
  kUnknown,
  kNone,        // (of a 1-based number: 0, "no slot")
  kOutOfRange,  // (of a 1-based number: beyond the table)
  kSpot,
  kLightMap,  // (first word 8; 7 is no kind)
};
constexpr uint32_t slot_type_word(SlotKind kind) {
  return kind == SlotKind::kSpot ? PBRT_HIP_TEXTURE_SPOT : (kind == SlotKind::kLightMap ? PBRT_HIP_TEXTURE_LIGHT_MAP : (uint32_t)kind);
}

// the record type of a kind, stated once
template <class Rec> struct SlotOf;
template <> struct SlotOf<pbrt_hip_texture> { static constexpr SlotKind kind = SlotKind::kChecker; };
template <> struct SlotOf<pbrt_hip_envmap> { static constexpr SlotKind kind = SlotKind::kEnvmap; };
template <> struct SlotOf<pbrt_hip_normals> { static constexpr SlotKind kind = SlotKind::kNormals; };
template <> struct SlotOf<pbrt_hip_pixel_filter> { static constexpr SlotKind kind = SlotKind::kFilter; };
template <> struct SlotOf<pbrt_hip_image_texture> { static constexpr SlotKind kind = SlotKind::kImage; };
template <> struct SlotOf<pbrt_hip_spot_cone> { static constexpr SlotKind kind = SlotKind::kSpot; };
template <> struct SlotOf<pbrt_hip_light_map> { static constexpr SlotKind kind = SlotKind::kLightMap; };

inline SlotKind slot_kind(const pbrt_hip_texture *textures, uint32_t index) {
  const uint32_t type = textures[index].type;
  if (type == PBRT_HIP_TEXTURE_SPOT) return SlotKind::kSpot;
  if (type == PBRT_HIP_TEXTURE_LIGHT_MAP) return SlotKind::kLightMap;
  return type <= (uint32_t)SlotKind::kImage ? (SlotKind)type : SlotKind::kUnknown;
}

// slot `index` (0-based) read as a Rec, whatever its first word says
template <class Rec>
Rec read_slot(const pbrt_hip_texture *textures, uint32_t index) {
  static_assert(sizeof(Rec) == sizeof(pbrt_hip_texture) && sizeof(Rec) == 64 && sizeof(SlotOf<Rec>) > 0, "a record is one 64-byte slot of the texture table");
  Rec rec;
  std::memcpy(&rec, textures + index, sizeof rec);
  return rec;
}

// the slot that holds `rec`; its first word is the record type's
template <class Rec>
pbrt_hip_texture write_slot(const Rec &rec) {
  static_assert(sizeof(Rec) == sizeof(pbrt_hip_texture) && sizeof(Rec) == 64, "a record is one 64-byte slot of the texture table");
  pbrt_hip_texture slot;
  std::memcpy(&slot, &rec, sizeof slot);
  slot.type = slot_type_word(SlotOf<Rec>::kind);
  return slot;
}

// A description's table, decoded once: decode_texture_table(), of a description whose `textures` holds n_textures slots and whose mat_id
// and spheres' `mat` have been checked against n_mats.
struct TextureTable {
  const pbrt_hip_texture *slots = nullptr;
  std::vector<SlotKind> kinds;  // of slot i
  // the first record of its kind (scene creation refuses a second)
  std::optional<pbrt_hip_pixel_filter> filter;
  std::optional<pbrt_hip_normals> normals;
  struct Image {
    uint32_t slot;
    pbrt_hip_image_texture rec;
  };
  std::vector<Image> images;  // in slot order
  struct Cone {
    uint32_t slot;
    pbrt_hip_spot_cone rec;
  };
  std::vector<Cone> cones;  // the spot lights' cones, in slot order
  struct LightMap {
    uint32_t slot;
    pbrt_hip_light_map rec;
  };
  std::vector<LightMap> light_maps;  // the mapped lights' records, in slot order
  // a triangle's / a sphere's material has a texture for Kd: the corner (u, v) must be there / the sphere's own (u, v) are used
  bool textured_tris = false, textured_sph = false;

  // what the 1-based number of a kd_tex, of an environment-map light, of a spot light, of a mapped light or of a light map's `image` names
  SlotKind named(uint32_t number) const { return number == 0u ? SlotKind::kNone : (number > kinds.size() ? SlotKind::kOutOfRange : kinds[number - 1u]); }
  // the environment map that 1-based `number` names, or nothing
  std::optional<pbrt_hip_envmap> envmap(uint32_t number) const {
    if (named(number) != SlotKind::kEnvmap) return std::nullopt;
    return read_slot<pbrt_hip_envmap>(slots, number - 1u);
  }
  // the cone that 1-based `number` names, or nothing
  const pbrt_hip_spot_cone *cone(uint32_t number) const {
    if (named(number) != SlotKind::kSpot) return nullptr;
    for (const Cone &c : cones)
      if (c.slot == number - 1u) return &c.rec;
    return nullptr;
  }
  // the light map that 1-based `number` names, or nothing
  const pbrt_hip_light_map *light_map(uint32_t number) const {
    if (named(number) != SlotKind::kLightMap) return nullptr;
    for (const LightMap &m : light_maps)
      if (m.slot == number - 1u) return &m.rec;
    return nullptr;
  }
};

// a material whose Kd is a texture
inline bool kd_textured(const pbrt_hip_material &m) { return m.kd_tex != 0u && m.type == 0u; }

inline TextureTable decode_texture_table(const pbrt_hip_scene_desc &d) {
  TextureTable t;
  t.slots = d.textures;
  t.kinds.resize(d.n_textures);
  for (uint32_t i = 0; i < d.n_textures; i++) {
    t.kinds[i] = slot_kind(d.textures, i);
    if (t.kinds[i] == SlotKind::kFilter && !t.filter) t.filter = read_slot<pbrt_hip_pixel_filter>(d.textures, i);
    if (t.kinds[i] == SlotKind::kNormals && !t.normals) t.normals = read_slot<pbrt_hip_normals>(d.textures, i);
    if (t.kinds[i] == SlotKind::kImage) t.images.push_back({i, read_slot<pbrt_hip_image_texture>(d.textures, i)});
    if (t.kinds[i] == SlotKind::kSpot) t.cones.push_back({i, read_slot<pbrt_hip_spot_cone>(d.textures, i)});
    if (t.kinds[i] == SlotKind::kLightMap) t.light_maps.push_back({i, read_slot<pbrt_hip_light_map>(d.textures, i)});
  }
  for (uint32_t k = 0; k < d.n_tris && !t.textured_tris; k++) t.textured_tris = kd_textured(d.mats[d.mat_id[k]]);
  for (uint32_t s = 0; s < d.n_spheres && !t.textured_sph; s++) t.textured_sph = kd_textured(d.mats[d.spheres[s].mat]);
  return t;
}

}  // namespace pbrt_hip
