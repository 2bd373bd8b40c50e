// image_texture.hpp -- image textures for Kd on the host: the record's checks, and the texel pool with the slot's three
// rows that the kernels read (image_lookup.hpp is the one statement of the lookup's arithmetic).
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/pbrt_hip.h"

namespace pbrt_hip {

// PBRT_HIP_OK, or the refusal of one record (every message holds "image"; `what` prefixes it): everything but the texels ...
int image_check(const pbrt_hip_image_texture &t, const std::string &what);
// ... and the texels, finite and >= 0 -- read only once the sizes and image_check_totals have passed for every record of the table
int image_check_texels(const pbrt_hip_image_texture &t, const std::string &what);
// the caps over all the image slots of a table: their number and the sum of their texels (PBRT_HIP_ERR_LIMIT)
int image_check_totals(uint32_t n_slots, uint64_t n_texels, const std::string &what);

// appends the record's texels to `pool` as {r, g, b, 0} in the record's own row order and writes the slot's three rows (image_lookup.hpp encode)
void image_pack(const pbrt_hip_image_texture &t, std::vector<float4> *pool, float4 rows[3]);

// a mapped light's record (every message holds "light map"): its kind, its rotation and its window -- everything but what
// its `image` names, which is the table's to say
int light_map_check(const pbrt_hip_light_map &m, const std::string &what);

}  // namespace pbrt_hip
