// Host build (g++) of csrc/bc6h_decode.h, the BC6H decoder the kernels and dxtlt_decode_bc6h_blocks use, so that the CPU test suite
// can compare it with the numpy statement of the decoder (tests/bc6h_decode_ref.py) and with Pillow's recorded answers.
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../dxt-lossless-transform_amd/csrc/bc6h_decode.h"

// 128 bytes per block: sixteen pixels of four little-endian halves r, g, b, a; pixel 4 r + c at (c, r)
extern "C" void shim_bc6h_decode_blocks(const uint8_t* in, uint8_t* out, size_t num_blocks)
{
    for (size_t i = 0; i < num_blocks; ++i) {
        dxtlt::bc7::B128 b;
        std::memcpy(b.d, in + 16 * i, 16);
        uint32_t px[32];
        dxtlt::bc6h::decode_bc6h_block(b, px);
        for (int k = 0; k < 32; ++k)
            for (int c = 0; c < 4; ++c)
                out[128 * i + 4 * k + c] = (uint8_t)(px[k] >> (8 * c));
    }
}

// the decoder's field table, for the comparison with the layout strings of tests/bc6h_ref.py: the runs of class k as
// (channel, endpoint, block bit, value bit, length) quintuples into out[5 * cap]; returns their number
template <int K>
static int runs_of(int* out, int cap)
{
    const int n = dxtlt::bc6h::n_field_runs<K>();
    for (int i = 0; i < n && i < cap; ++i) {
        const dxtlt::bc6h::FieldRun r = dxtlt::bc6h::DecodeTab<K>::runs[i];
        const int q[5] = {r.ch, r.e, r.src, r.dst, r.len};
        std::memcpy(out + 5 * i, q, sizeof q);
    }
    return n;
}

extern "C" int shim_bc6h_field_runs(int k, int* out, int cap)
{
    switch (k) {
#define DXTLT_C(K) case K: return runs_of<K>(out, cap);
    DXTLT_BC6H_CASES(DXTLT_C)
#undef DXTLT_C
    default: return -1;
    }
}

// (bits, delta r, delta g, delta b, transformed, two regions) of class k
extern "C" int shim_bc6h_class_desc(int k, int* out)
{
    switch (k) {
#define DXTLT_C(K)                                                                                                       \
    case K: {                                                                                                            \
        using T = dxtlt::bc6h::DecodeTab<K>;                                                                             \
        const int q[6] = {T::bits, T::delta[0], T::delta[1], T::delta[2], T::transformed ? 1 : 0, T::two_regions ? 1 : 0}; \
        std::memcpy(out, q, sizeof q);                                                                                   \
        return 0;                                                                                                        \
    }
    DXTLT_BC6H_CASES(DXTLT_C)
#undef DXTLT_C
    default: return -1;
    }
}
