// Host build (g++) of csrc/bc7_decode.h, the BC7 decoder the kernels and dxtlt_decode_bc7_blocks use, so that the CPU test suite
// can compare it with the numpy statement of the decoder (tests/bc7_decode_ref.py) and with Pillow's recorded answers.
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../dxt-lossless-transform_amd/csrc/bc7_decode.h"

// 64 bytes per block: sixteen r, g, b, a pixels, pixel 4 r + c at (c, r)
extern "C" void shim_bc7_decode_blocks(const uint8_t* in, uint8_t* out, size_t num_blocks)
{
    for (size_t i = 0; i < num_blocks; ++i) {
        dxtlt::bc7::B128 b;
        std::memcpy(b.d, in + 16 * i, 16);
        uint32_t px[16];
        dxtlt::bc7::decode_bc7_block(b, px);
        for (int k = 0; k < 16; ++k)
            for (int c = 0; c < 4; ++c)
                out[64 * i + 4 * k + c] = (uint8_t)(px[k] >> (8 * c));
    }
}
