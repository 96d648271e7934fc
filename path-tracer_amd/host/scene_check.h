// Checks of a scene description's light and material tables, shared by pt_scene_create (csrc/pt_gpu.hip prep_create) and
// the edits of a live scene on the host (pth_scene_set_lights / _set_materials) and on the device (pt_scene_set_lights /
// _set_materials): one implementation, one set of messages.  Both throw pth::Error with PT_ERR_INVALID.
#pragma once
#include <cstdint>

#include "ptgpu.h"

namespace pth {
// Every texture index of every material -1 or a texture with the channels its slot demands (3: albedo, emissive, normal;
// 1: opacity, metalness, roughness) whose texels lie inside the blob.
void check_materials(const pt_material* materials, uint32_t n_materials, const pt_texture* textures, uint32_t n_textures,
                     uint64_t n_texel_bytes);
// Every light of a kind PT_LIGHT_*.
void check_lights(const pt_light* lights, uint32_t n_lights);
}  // namespace pth
