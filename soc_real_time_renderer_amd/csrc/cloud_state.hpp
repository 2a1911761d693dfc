// cloud_state.hpp — the renderer-owned state of CloudRendering (part of clouds_plan.hpp; on its own so that renderer.hpp
// does not pull the clouds kernels' argument structs and constants into every host file).
#pragma once

#include <stdint.h>

namespace soc {

// `state` of cloud_rendering_launch (the render graph's CloudRendering; null: the stateless entry, which builds every
// table and clears its counter block on every call): the renderer-owned record of what the workspace holds between frames.
struct CloudState {
    // static tables (SOC_CLOUDS_STATIC_TABLES, default 1): built when first needed and when their key changes
    bool od_valid = false, noise_valid = false;
    uint32_t c2_bits = 0;                 // od table: the bit pattern of dot(pSun, pSun)
    const void* noise_data = nullptr;     // noise tables: the noise image's (data, format, pitch)
    int32_t noise_format = 0, noise_pitch = 0;
    void* workspace = nullptr;            // the workspace the tables and counter blocks were built in
    // two counter blocks, alternating by frame: frame N uses block N & 1 and its clouds_classify clears the other
    bool blocks_primed = false;           // both blocks were cleared and every frame since ran the alternating form
    uint32_t frame = 0;
    void invalidate_tables() { od_valid = noise_valid = false; }
    void reset() { *this = CloudState(); }
};

}  // namespace soc
