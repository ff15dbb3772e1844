// normalize_api.cpp -- C ABI of the BC1 / BC2 / BC3 block-normalisation entry points (include/dxtlt_bc1_normalize.h,
// include/dxtlt_bc23_normalize.h): the reference's experimental modules, /root/reference/src/core/dxt-lossless-transform-bc{1,2,3}/
// src/experimental/normalize_blocks/{normalize.rs, transform.rs}, on the device.  Host-pointer calls stage through the calling
// thread's device buffers (H2D, kernel, D2H, synchronous).  What every call answers to defective arguments, and in which order,
// is pinned by tests/test_normalize_defects.py.
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../include/dxtlt_bc1_normalize.h"
#include "../../include/dxtlt_bc23_normalize.h"
#include "../../include/dxtlt_gfx950.h"
#include "bcn_launch.h"
#include "host_common.h"

using dxtlt::Settings;
using dxtlt_host::fail;
using dxtlt_host::kInvalidArgument;
using dxtlt_host::kInvalidLength;
using dxtlt_host::kOk;

namespace {

using dxtlt_host::NormFormat;
using dxtlt_host::kNormBc1;
using dxtlt_host::kNormBc2;
using dxtlt_host::kNormBc3;

int32_t check_modes(const NormFormat& F, uint8_t alpha_mode, uint8_t color_mode)
{
    if (color_mode > dxtlt::norm_limits(F.fmt).colour)
        return fail(kInvalidArgument, "color_mode must be 0 (None), 1 (Color0Only) or 2 (ReplicateColor)");
    if (alpha_mode > dxtlt::norm_limits(F.fmt).alpha)
        return fail(kInvalidArgument, "alpha_mode must be 0..3");
    return kOk;
}

hipError_t launch_blocks(const NormFormat& F, const void* in, void* out, size_t len, uint8_t alpha_mode, uint8_t color_mode,
                         hipStream_t st)
{
    return F.fmt == 1 ? dxtlt::launch_normalize_bc1_blocks(in, out, len / 8, color_mode, st)
                      : dxtlt::launch_normalize_bc23_blocks(F.fmt, in, out, len / 16, alpha_mode, color_mode, st);
}

// d_any: BC1 only
hipError_t launch_all_modes(const NormFormat& F, const void* in, void* const* outs, size_t len, uint32_t* d_any, hipStream_t st)
{
    return F.fmt == 1 ? dxtlt::launch_normalize_bc1_all_modes(in, outs, len / 8, d_any, st)
                      : dxtlt::launch_normalize_bc23_all_modes(F.fmt, in, outs, len / 16, st);
}

hipError_t launch_split2(const NormFormat& F, void* colours, void* indices, size_t num_blocks, uint8_t color_mode, hipStream_t st)
{
    return F.fmt == 1 ? dxtlt::launch_normalize_bc1_split(colours, indices, num_blocks, color_mode, st)
                      : dxtlt::launch_normalize_bc2_split(colours, indices, num_blocks, color_mode, st);
}

// Host-pointer calls: these uploads, this launch, these downloads, one synchronise, all on the staging stream
struct Transfers {
    struct Copy {
        void* device;
        void* host;
        size_t bytes;
        const char* what;
    } item[13];
    int count = 0;
    Transfers& add(void* device, const void* host, size_t bytes, const char* what = nullptr)
    {
        item[count++] = Copy{device, const_cast<void*>(host), bytes, what};
        return *this;
    }
};

template <class LaunchFn>
int32_t staged(hipStream_t st, const Transfers& up, LaunchFn launch, const Transfers& down)
{
    for (int i = 0; i < up.count; ++i)
        HIP_TRY(hipMemcpyAsync(up.item[i].device, up.item[i].host, up.item[i].bytes, hipMemcpyHostToDevice, st), "H2D copy");
    HIP_TRY(launch(), "kernel launch");
    for (int i = 0; i < down.count; ++i)
        HIP_TRY(hipMemcpyAsync(down.item[i].host, down.item[i].device, down.item[i].bytes, hipMemcpyDeviceToHost, st),
                down.item[i].what ? down.item[i].what : "D2H copy");
    HIP_TRY(hipStreamSynchronize(st), "stream synchronize");
    return kOk;
}

constexpr size_t pad256(size_t n) { return (n + 255) & ~(size_t)255; }

// a device word for the "any block normalised" flag, next to the staging buffers of this thread; get(): zeroed on `stream`
struct FlagWord {
    uint32_t* d = nullptr;
    int device = -1;
    ~FlagWord()
    {
        if (d) (void)hipFree(d);
    }
    int32_t get(uint32_t** out, hipStream_t stream)
    {
        int dev = 0;
        HIP_TRY(hipGetDevice(&dev), "hipGetDevice");
        if (dev != device) {
            if (d) (void)hipFree(d);
            d = nullptr;
            HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d), 256), "hipMalloc(flag)");
            device = dev;
        }
        HIP_TRY(hipMemsetAsync(d, 0, sizeof(uint32_t), stream), "memset flag");
        *out = d;
        return kOk;
    }
};
thread_local FlagWord g_flag;

// ---- AoS blocks ---------------------------------------------------------------------------------------------------
int32_t blocks_device(const NormFormat& F, const void* d_in, void* d_out, size_t len, uint8_t alpha_mode, uint8_t color_mode,
                      void* stream)
{
    if (len % F.block_bytes != 0)
        return fail(kInvalidLength, F.bad_len);
    if (int32_t rc = check_modes(F, alpha_mode, color_mode); rc != kOk)
        return rc;
    if (len > 0 && (d_in == nullptr || d_out == nullptr))
        return fail(kInvalidArgument, "NULL device buffer with len > 0");
    HIP_TRY(launch_blocks(F, d_in, d_out, len, alpha_mode, color_mode, static_cast<hipStream_t>(stream)), "kernel launch");
    return kOk;
}

int32_t blocks_host(const NormFormat& F, const uint8_t* in, uint8_t* out, size_t len, uint8_t alpha_mode, uint8_t color_mode)
{
    if (len % F.block_bytes != 0)
        return fail(kInvalidLength, F.bad_len);
    if (int32_t rc = check_modes(F, alpha_mode, color_mode); rc != kOk)
        return rc;
    if (len == 0)
        return kOk;
    if (in == nullptr || out == nullptr)
        return fail(kInvalidArgument, "NULL buffer with len > 0");
    if (alpha_mode == 0 && color_mode == 0) {   // normalize.rs (bc1 :53-64, bc2 :50-61, bc3 :52-62): plain copy, nothing when in place
        if (in != out)
            std::memcpy(out, in, len);
        return kOk;
    }
    void *d_a = nullptr, *d_b = nullptr;
    hipStream_t st = nullptr;
    if (int32_t rc = dxtlt_host::acquire_staging(len, &d_a, &d_b, &st); rc != kOk)
        return rc;
    return staged(st, Transfers().add(d_a, in, len), [&] { return launch_blocks(F, d_a, d_a, len, alpha_mode, color_mode, st); },
                  Transfers().add(d_a, out, len));
}

// ---- all modes ----------------------------------------------------------------------------------------------------
// d_any / out_any: BC1 only
int32_t all_modes_device(const NormFormat& F, const void* d_in, void* const* d_outs, size_t len, uint32_t* d_any, void* stream)
{
    if (len % F.block_bytes != 0)
        return fail(kInvalidLength, F.bad_len);
    if (d_outs == nullptr)
        return fail(kInvalidArgument, "NULL output pointer array");
    if (len > 0) {
        if (d_in == nullptr)
            return fail(kInvalidArgument, "NULL device buffer with len > 0");
        for (int i = 0; i < F.all_modes_outputs; ++i)
            if (d_outs[i] == nullptr)
                return fail(kInvalidArgument, F.fmt == 1 ? "NULL device buffer with len > 0" : "NULL device output buffer with len > 0");
    }
    HIP_TRY(launch_all_modes(F, d_in, d_outs, len, d_any, static_cast<hipStream_t>(stream)), "kernel launch");
    return kOk;
}

int32_t all_modes_host(const NormFormat& F, const uint8_t* in, uint8_t* const* outs, size_t len, bool* out_any)
{
    if (len % F.block_bytes != 0)
        return fail(kInvalidLength, F.bad_len);
    if (outs == nullptr)
        return fail(kInvalidArgument, "NULL output pointer array");
    if (out_any)
        *out_any = false;
    if (len == 0)
        return kOk;
    if (in == nullptr)
        return fail(kInvalidArgument, "NULL buffer with len > 0");
    for (int i = 0; i < F.all_modes_outputs; ++i)
        if (outs[i] == nullptr)
            return fail(kInvalidArgument, F.fmt == 1 ? "NULL buffer with len > 0" : "NULL output buffer with len > 0");
    // staging: the input at the start of the first buffer, the outputs packed after it and in the second buffer.  BC1's `None`
    // output is no plain copy either: fully transparent blocks are rewritten in every output (normalize.rs:447-454)
    const size_t padded = pad256(len);
    const int half = (F.all_modes_outputs + 2) / 2;
    void *d_a = nullptr, *d_b = nullptr;
    hipStream_t st = nullptr;
    if (int32_t rc = dxtlt_host::acquire_staging((size_t)half * padded, &d_a, &d_b, &st); rc != kOk)
        return rc;
    uint32_t* d_flag = nullptr;
    uint32_t any = 0;
    if (F.fmt == 1)
        if (int32_t rc = g_flag.get(&d_flag, st); rc != kOk)
            return rc;
    void* d_outs[12] = {};
    Transfers down;
    for (int i = 0; i < F.all_modes_outputs; ++i) {
        const int slot = i + 1;   // slot 0 of buffer a holds the input
        d_outs[i] = slot < half ? static_cast<uint8_t*>(d_a) + (size_t)slot * padded
                                : static_cast<uint8_t*>(d_b) + (size_t)(slot - half) * padded;
        down.add(d_outs[i], outs[i], len);
    }
    if (d_flag)
        down.add(d_flag, &any, sizeof(uint32_t), "D2H flag");
    if (int32_t rc = staged(st, Transfers().add(d_a, in, len), [&] { return launch_all_modes(F, d_a, d_outs, len, d_flag, st); }, down);
        rc != kOk)
        return rc;
    if (out_any)
        *out_any = any != 0;
    return kOk;
}

// ---- colours (4 bytes per block) and indices (4 bytes per block) in two arrays, in place: BC1 and BC2 -----------------
int32_t split2_device(const NormFormat& F, void* d_colors, void* d_indices, size_t num_blocks, uint8_t color_mode, void* stream)
{
    if (int32_t rc = check_modes(F, 0, color_mode); rc != kOk)
        return rc;
    if (num_blocks > 0 && (d_colors == nullptr || d_indices == nullptr))
        return fail(kInvalidArgument, "NULL device buffer with num_blocks > 0");
    HIP_TRY(launch_split2(F, d_colors, d_indices, num_blocks, color_mode, static_cast<hipStream_t>(stream)), "kernel launch");
    return kOk;
}

int32_t split2_host(const NormFormat& F, uint8_t* colors_ptr, uint8_t* indices_ptr, size_t num_blocks, uint8_t color_mode)
{
    if (int32_t rc = check_modes(F, 0, color_mode); rc != kOk)
        return rc;
    if (num_blocks == 0 || color_mode == DXTLT_NORMALIZE_NONE)   // bc1 normalize.rs:293-295
        return kOk;
    if (colors_ptr == nullptr || indices_ptr == nullptr)
        return fail(kInvalidArgument, "NULL buffer with num_blocks > 0");
    const size_t half = num_blocks * 4;
    void *d_col = nullptr, *d_idx = nullptr;
    hipStream_t st = nullptr;
    if (int32_t rc = dxtlt_host::acquire_staging(half, &d_col, &d_idx, &st); rc != kOk)
        return rc;
    return staged(st, Transfers().add(d_col, colors_ptr, half).add(d_idx, indices_ptr, half),
                  [&] { return launch_split2(F, d_col, d_idx, num_blocks, color_mode, st); },
                  Transfers().add(d_col, colors_ptr, half).add(d_idx, indices_ptr, half));
}

// ---- fused normalise + transform: transform_bcN_with_settings(normalize_blocks(input, modes), settings) in one pass over the data.
// The modes go into the forward tile kernels (bcn_device.h), the host call takes the common host paths (host_staging.cpp).
// The checks keep each format's own order and codes.  BC1, host: colour mode, then dxtlt_host::transform's length (kInvalidLength),
// decorrelation mode, NULL; BC1, device: length (kInvalidLength) first.  BC2 / BC3 answer every defect -- a mode out of range, a
// length that is no whole number of blocks, a NULL pointer with len > 0 -- with kInvalidArgument, before any device work.
int32_t check_fused(const NormFormat& F, bool device, const void* in, const void* out, size_t len, const Settings& s)
{
    const bool bc1 = F.fmt == 1;
    if (bc1 && device && len % F.block_bytes != 0)
        return fail(kInvalidLength, F.bad_len);
    if (int32_t rc = check_modes(F, (uint8_t)s.normalize_alpha, (uint8_t)s.normalize); rc != kOk)
        return rc;
    if (bc1 && !device)
        return kOk;
    if (s.variant > 3)
        return fail(kInvalidArgument, "decorrelation_mode must be 0..3");
    if (len % F.block_bytes != 0)
        return fail(kInvalidArgument, F.bad_len);
    if (len > 0 && (in == nullptr || out == nullptr))
        return fail(kInvalidArgument, bc1 ? "NULL device buffer with len > 0" : "NULL buffer with len > 0");
    return kOk;
}

int32_t fused_host(const NormFormat& F, const uint8_t* in, uint8_t* out, size_t len, const Settings& s)
{
    if (int32_t rc = check_fused(F, false, in, out, len, s); rc != kOk)
        return rc;
    return dxtlt_host::transform(F.fmt, false, in, out, len, s);
}

int32_t fused_device(const NormFormat& F, const void* d_in, void* d_out, size_t len, const Settings& s, void* stream)
{
    if (int32_t rc = check_fused(F, true, d_in, d_out, len, s); rc != kOk)
        return rc;
    return dxtlt_host::enqueue(F.fmt, false, d_in, d_out, len / F.block_bytes, s, static_cast<hipStream_t>(stream));
}

}  // namespace

int32_t dxtlt_host::normalize_thread_flag(uint32_t** d_flag, hipStream_t stream) { return g_flag.get(d_flag, stream); }

void dxtlt_host::release_normalize_thread_flag()
{
    if (g_flag.d) (void)hipFree(g_flag.d);
    g_flag.d = nullptr;
    g_flag.device = -1;
}

extern "C" {

// ---- BC1 (include/dxtlt_bc1_normalize.h) ----------------------------------------------------------------------------
int32_t dxtlt_bc1_normalize_blocks(const uint8_t* i, uint8_t* o, size_t len, uint8_t color_mode)
{
    return blocks_host(kNormBc1, i, o, len, 0, color_mode);
}
int32_t dxtlt_bc1_normalize_blocks_device(const void* i, void* o, size_t len, uint8_t color_mode, void* st)
{
    return blocks_device(kNormBc1, i, o, len, 0, color_mode, st);
}
int32_t dxtlt_bc1_normalize_split_blocks_in_place(uint8_t* colors_ptr, uint8_t* indices_ptr, size_t num_blocks, uint8_t color_mode)
{
    return split2_host(kNormBc1, colors_ptr, indices_ptr, num_blocks, color_mode);
}
int32_t dxtlt_bc1_normalize_split_blocks_in_place_device(void* d_colors, void* d_indices, size_t num_blocks, uint8_t color_mode,
                                                         void* st)
{
    return split2_device(kNormBc1, d_colors, d_indices, num_blocks, color_mode, st);
}
int32_t dxtlt_bc1_normalize_blocks_all_modes(const uint8_t* i, uint8_t* const o[3], size_t len, bool* out_any_normalized)
{
    return all_modes_host(kNormBc1, i, o, len, out_any_normalized);
}
int32_t dxtlt_bc1_normalize_blocks_all_modes_device(const void* i, void* const o[3], size_t len, uint32_t* d_any_normalized,
                                                    void* st)
{
    return all_modes_device(kNormBc1, i, o, len, d_any_normalized, st);
}
int32_t dxtlt_transform_bc1_with_normalize_blocks(const uint8_t* i, uint8_t* o, uint8_t* work_ptr, size_t len, uint8_t color_mode,
                                                  uint8_t decorrelation_mode, bool split_colour_endpoints)
{
    (void)work_ptr;  // the reference's CPU scratch buffer; the fused kernel needs none
    return fused_host(kNormBc1, i, o, len, Settings{decorrelation_mode, false, split_colour_endpoints, color_mode});
}
int32_t dxtlt_transform_bc1_with_normalize_blocks_device(const void* i, void* o, size_t len, uint8_t color_mode,
                                                         uint8_t decorrelation_mode, bool split_colour_endpoints, void* st)
{
    return fused_device(kNormBc1, i, o, len, Settings{decorrelation_mode, false, split_colour_endpoints, color_mode}, st);
}

// ---- BC2 / BC3 (include/dxtlt_bc23_normalize.h) ---------------------------------------------------------------------
int32_t dxtlt_bc2_normalize_blocks(const uint8_t* i, uint8_t* o, size_t len, uint8_t color_mode)
{
    return blocks_host(kNormBc2, i, o, len, 0, color_mode);
}
int32_t dxtlt_bc3_normalize_blocks(const uint8_t* i, uint8_t* o, size_t len, uint8_t alpha_mode, uint8_t color_mode)
{
    return blocks_host(kNormBc3, i, o, len, alpha_mode, color_mode);
}
int32_t dxtlt_bc2_normalize_blocks_device(const void* i, void* o, size_t len, uint8_t color_mode, void* st)
{
    return blocks_device(kNormBc2, i, o, len, 0, color_mode, st);
}
int32_t dxtlt_bc3_normalize_blocks_device(const void* i, void* o, size_t len, uint8_t alpha_mode, uint8_t color_mode, void* st)
{
    return blocks_device(kNormBc3, i, o, len, alpha_mode, color_mode, st);
}
int32_t dxtlt_bc2_normalize_blocks_all_modes(const uint8_t* i, uint8_t* const o[3], size_t len)
{
    return all_modes_host(kNormBc2, i, o, len, nullptr);
}
int32_t dxtlt_bc3_normalize_blocks_all_modes(const uint8_t* i, uint8_t* const o[12], size_t len)
{
    return all_modes_host(kNormBc3, i, o, len, nullptr);
}
int32_t dxtlt_bc2_normalize_blocks_all_modes_device(const void* i, void* const o[3], size_t len, void* st)
{
    return all_modes_device(kNormBc2, i, o, len, nullptr, st);
}
int32_t dxtlt_bc3_normalize_blocks_all_modes_device(const void* i, void* const o[12], size_t len, void* st)
{
    return all_modes_device(kNormBc3, i, o, len, nullptr, st);
}

int32_t dxtlt_transform_bc2_with_normalize_blocks(const uint8_t* i, uint8_t* o, size_t len, uint8_t color_mode,
                                                  uint8_t decorrelation_mode, bool split_colour_endpoints)
{
    return fused_host(kNormBc2, i, o, len, Settings{decorrelation_mode, false, split_colour_endpoints, color_mode});
}
int32_t dxtlt_transform_bc2_with_normalize_blocks_device(const void* i, void* o, size_t len, uint8_t color_mode,
                                                         uint8_t decorrelation_mode, bool split_colour_endpoints, void* st)
{
    return fused_device(kNormBc2, i, o, len, Settings{decorrelation_mode, false, split_colour_endpoints, color_mode}, st);
}
int32_t dxtlt_transform_bc3_with_normalize_blocks(const uint8_t* i, uint8_t* o, size_t len, uint8_t alpha_mode, uint8_t color_mode,
                                                  uint8_t decorrelation_mode, bool split_alpha_endpoints,
                                                  bool split_colour_endpoints)
{
    return fused_host(kNormBc3, i, o, len, Settings{decorrelation_mode, split_alpha_endpoints, split_colour_endpoints, color_mode, alpha_mode});
}
int32_t dxtlt_transform_bc3_with_normalize_blocks_device(const void* i, void* o, size_t len, uint8_t alpha_mode, uint8_t color_mode,
                                                         uint8_t decorrelation_mode, bool split_alpha_endpoints,
                                                         bool split_colour_endpoints, void* st)
{
    return fused_device(kNormBc3, i, o, len, Settings{decorrelation_mode, split_alpha_endpoints, split_colour_endpoints, color_mode, alpha_mode},
                        st);
}

int32_t dxtlt_bc2_normalize_split_blocks_in_place_device(void* d_colors, void* d_indices, size_t num_blocks, uint8_t color_mode,
                                                         void* st)
{
    return split2_device(kNormBc2, d_colors, d_indices, num_blocks, color_mode, st);
}
int32_t dxtlt_bc2_normalize_split_blocks_in_place(const uint8_t* alpha_ptr, uint8_t* colors_ptr, uint8_t* indices_ptr,
                                                  size_t num_blocks, uint8_t color_mode)
{
    (void)alpha_ptr;   // the colour decision ignores alpha (bc2 normalize.rs:131-150)
    return split2_host(kNormBc2, colors_ptr, indices_ptr, num_blocks, color_mode);
}

int32_t dxtlt_bc3_normalize_split_blocks_in_place_device(void* d_aep, void* d_aidx, void* d_cep, void* d_cidx, size_t num_blocks,
                                                         uint8_t alpha_mode, uint8_t color_mode, void* st)
{
    if (int32_t rc = check_modes(kNormBc3, alpha_mode, color_mode); rc != kOk)
        return rc;
    if (num_blocks > 0 && (d_aep == nullptr || d_aidx == nullptr || d_cep == nullptr || d_cidx == nullptr))
        return fail(kInvalidArgument, "NULL device buffer with num_blocks > 0");
    HIP_TRY(dxtlt::launch_normalize_bc3_split(d_aep, d_aidx, d_cep, d_cidx, num_blocks, alpha_mode, color_mode,
                                              static_cast<hipStream_t>(st)),
            "kernel launch");
    return kOk;
}

int32_t dxtlt_bc3_normalize_split_blocks_in_place(uint8_t* aep, uint8_t* aidx, uint8_t* cep, uint8_t* cidx, size_t num_blocks,
                                                  uint8_t alpha_mode, uint8_t color_mode)
{
    if (int32_t rc = check_modes(kNormBc3, alpha_mode, color_mode); rc != kOk)
        return rc;
    if (num_blocks == 0 || (alpha_mode == 0 && color_mode == 0))
        return kOk;
    if (aep == nullptr || aidx == nullptr || cep == nullptr || cidx == nullptr)
        return fail(kInvalidArgument, "NULL buffer with num_blocks > 0");
    // sections packed into the two staging buffers: [alpha endpoints | alpha indices] and [colour endpoints | indices]
    const size_t n = num_blocks, off_aidx = pad256(2 * n), off_cidx = pad256(4 * n);
    void *d_a = nullptr, *d_c = nullptr;
    hipStream_t st = nullptr;
    const size_t need_a = off_aidx + 6 * n, need_c = off_cidx + 4 * n;
    if (int32_t rc = dxtlt_host::acquire_staging(need_a > need_c ? need_a : need_c, &d_a, &d_c, &st); rc != kOk)
        return rc;
    uint8_t* da = static_cast<uint8_t*>(d_a);
    uint8_t* dc = static_cast<uint8_t*>(d_c);
    const Transfers sections = Transfers().add(da, aep, 2 * n).add(da + off_aidx, aidx, 6 * n).add(dc, cep, 4 * n).add(dc + off_cidx, cidx, 4 * n);
    return staged(st, sections,
                  [&] { return dxtlt::launch_normalize_bc3_split(da, da + off_aidx, dc, dc + off_cidx, n, alpha_mode, color_mode, st); },
                  sections);
}

}  // extern "C"
