// pixel_batch_plan_main.cpp -- the two planners of the batched pixel calls (csrc/pixel_batch_plan.h: pure host functions) as a
// stand-alone program for the host sanitizers: tests/test_pixels_batch_plan_sanitized.py builds it with
// -fsanitize=address,undefined together with the host side of csrc/batch_kernels.hip (build_batch_index) and runs it.  It plans the
// no-device cases of tests/test_pixels_batch_plan.py -- every class, the wide index, empty items, every refusal, the overlap rule in
// both orders, the launch limit, the auto plan under a small cap with an oversize item -- and writes the auto call's tables for a
// made-up arena address.  No device is touched and no address is dereferenced.  Prints "ok" and returns 0, or says what failed.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../dxt-lossless-transform_amd/csrc/pixel_batch_plan.h"

namespace pb = dxtlt_host::pixel_batch;

#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            return 1;                                                          \
        }                                                                      \
    } while (0)

static void* at(uint64_t a) { return reinterpret_cast<void*>(static_cast<uintptr_t>(a)); }

static DxtltPixelBatchItem item(uint64_t in, uint64_t out, uint64_t len, int B, int inverse, int decorrelate, int layout)
{
    DxtltPixelBatchItem it{};
    it.d_input = at(in), it.d_output = at(out), it.len = len;
    it.pixel_bytes = (uint8_t)B, it.inverse = (uint8_t)inverse, it.decorrelate = (uint8_t)decorrelate, it.layout = (uint8_t)layout;
    return it;
}

static DxtltPixelBatchAutoItem auto_item(uint64_t in, uint64_t out, uint64_t len, int B)
{
    DxtltPixelBatchAutoItem it{};
    it.d_input = at(in), it.d_output = at(out), it.len = len, it.pixel_bytes = (uint8_t)B;
    return it;
}

int main()
{
    using namespace dxtlt_host;
    const uint64_t A = 0x1000000000ull, B = 0x2000000000ull;
    const uint64_t counts[] = {1, 15, 16, 17, 4095, 4096, 4097, 8193, 87381};
    pb::Plan plan;

    // every class, two items each, every residue as it comes
    std::vector<DxtltPixelBatchItem> items;
    for (int k = 0; k < 48; ++k) {
        const int c = k / 2, bytes = c < 12 ? 4 : 3;
        items.push_back(item(A + ((uint64_t)k << 22) + 7 * k, B + ((uint64_t)k << 22) + 11 * k, counts[k % 9] * bytes, bytes, (c / 6) % 2, (c / 3) % 2, c % 3));
    }
    CHECK(pb::plan_call(items.data(), items.size(), plan).code == kOk);
    CHECK(plan.launches.size() == 24);
    size_t bytes = 0;
    for (size_t k = 0; k < plan.launches.size(); ++k) {
        const pb::ClassLaunch& l = plan.launches[k];
        CHECK(l.key == (int)k && l.entries.size() == 2 && !l.wide && l.at == bytes);
        CHECK(l.entries[0].first_wg == 0 && l.entries[1].first_wg == l.entries[0].end_wg && l.entries[1].end_wg == l.wgs);
        bytes += l.entry_bytes + dxtlt::batch_index_bytes(l.wgs);
    }
    CHECK(plan.tables.size() == bytes);

    // 300 items of one to three tiles: the wide index; empty items between them own nothing
    items.clear();
    for (int k = 0; k < 300; ++k) {
        items.push_back(item(A + ((uint64_t)k << 20), B + ((uint64_t)k << 20), 4 * (100 + 4096ull * (k % 3)), 4, 0, 1, 2));
        if (k % 50 == 0)
            items.push_back(item(0, 0, 0, 3, 1, 0, 0));
    }
    CHECK(pb::plan_call(items.data(), items.size(), plan).code == kOk);
    CHECK(plan.launches.size() == 1 && plan.launches[0].wide && plan.launches[0].entries.size() == 300 && plan.launches[0].wgs == 600);
    CHECK(pb::plan_call(items.data(), 0, plan).code == kOk && plan.launches.empty() && plan.tables.empty());
    CHECK(pb::plan_call(nullptr, 3, plan).code == kInvalidArgument);

    // every refusal, alone, behind and in front of a good item
    const DxtltPixelBatchItem ok = item(A + (1ull << 32), B + (1ull << 32), 4096 * 4, 4, 0, 1, 2);
    struct Bad {
        DxtltPixelBatchItem it;
        int32_t status;
    };
    const Bad bad[] = {{item(A, B, 8, 2, 0, 1, 2), kInvalidArgument},  {item(0, 0, 0, 0, 0, 1, 2), kInvalidArgument},
                       {item(A, B, 8, 4, 0, 1, 3), kInvalidArgument},  {item(0, B, 8, 4, 0, 1, 2), kInvalidArgument},
                       {item(A, 0, 8, 4, 1, 1, 2), kInvalidArgument},  {item(A, B, 10, 4, 0, 1, 2), kInvalidLength},
                       {item(A, B, 10, 3, 0, 1, 2), kInvalidLength},   {item(A, B, 64ull << 30, 4, 0, 1, 2), kInvalidArgument},
                       {item(A, A + 4, 8, 4, 0, 1, 2), kInvalidArgument}};
    for (const Bad& b : bad) {
        const DxtltPixelBatchItem alone[1] = {b.it}, behind[2] = {ok, b.it}, front[2] = {b.it, ok};
        CHECK(pb::plan_call(alone, 1, plan).code == b.status);
        CHECK(pb::plan_call(behind, 2, plan).code == b.status);
        CHECK(pb::plan_call(front, 2, plan).code == b.status);
    }
    // an output overlaps nothing, in both orders; inputs may overlap
    const uint64_t n = 4096;
    const DxtltPixelBatchItem first = item(A, B, n, 4, 0, 1, 2);
    const DxtltPixelBatchItem clash[] = {item(A + 0x100000, B + n - 1, n, 4, 0, 1, 2), item(A + 0x100000, A + n - 1, n, 4, 1, 0, 0),
                                         item(B + n - 4, A + 0x100000, n, 4, 1, 0, 0)};
    for (const DxtltPixelBatchItem& c : clash) {
        const DxtltPixelBatchItem ab[2] = {first, c}, ba[2] = {c, first};
        CHECK(pb::plan_call(ab, 2, plan).code == kInvalidArgument && pb::plan_call(ba, 2, plan).code == kInvalidArgument);
    }
    const DxtltPixelBatchItem shared[2] = {first, item(A + 8, B + n, n, 4, 0, 1, 2)};
    CHECK(pb::plan_call(shared, 2, plan).code == kOk && plan.launches.size() == 1);
    // the launch limit: five items of 63 GiB in one class
    items.clear();
    for (uint64_t k = 0; k < 5; ++k)
        items.push_back(item((k + 1) << 40, ((k + 1) << 40) + (1ull << 39), 63ull << 30, 4, 0, 1, 2));
    CHECK(pb::plan_call(items.data(), 5, plan).code == kInvalidArgument);
    CHECK(pb::plan_call(items.data(), 4, plan).code == kOk && plan.launches[0].wgs == 4 * ((63ull << 30) / 16384));

    // the auto plan: default cap, a small cap with two oversize items, the tables for a made-up arena
    const uint64_t lens[] = {0, 4, 3 * 17, 4 * 4097, 3 * (32768 + 7), 4 * 87381, 0, 3 * 87381, 4 * 8191};
    std::vector<DxtltPixelBatchAutoItem> autos;
    for (uint64_t k = 0; k < 9; ++k)
        autos.push_back(auto_item(A + (k << 24) + k, B + (k << 24) + 3 * k, lens[k], lens[k] % 4 == 0 && k != 7 ? 4 : 3));
    pb::AutoPlan ap;
    CHECK(pb::plan_auto_call(autos.data(), autos.size(), 256ull << 20, ap).code == kOk);
    CHECK(ap.chunks.size() == 1 && ap.counters == 54 && ap.chunks[0].candidate_launches() == 2);
    const uint64_t cap = 5 * 4 * 8191 + 5 * 3 * (32768 + 7) + 64;
    CHECK(pb::plan_auto_call(autos.data(), autos.size(), cap, ap).code == kOk);
    CHECK(ap.chunks.size() == 5);
    for (size_t i = 0; i < autos.size(); ++i) {
        CHECK(ap.items[i].slice_off % 16 == 0 && ap.items[i].slice_bytes == 5 * lens[i] && ap.items[i].first_counter == 6 * i);
        CHECK(ap.items[i].slice_bytes <= cap || ap.chunks[ap.items[i].chunk].count == 1);
    }
    std::vector<uint8_t> table(ap.table_bytes + 16);
    uint8_t* host = table.data() + (16 - reinterpret_cast<uintptr_t>(table.data()) % 16) % 16;
    pb::fill_auto_tables(ap, autos.data(), static_cast<uint8_t*>(at(0x3000000000ull)), host);
    for (const pb::AutoChunk& c : ap.chunks) {
        const dxtlt::EstimateTableEntry* s = reinterpret_cast<const dxtlt::EstimateTableEntry*>(host + c.sections_at);
        CHECK(c.estimator_entries == 0 || s[c.estimator_entries - 1].end_wg == c.estimator_wgs);
        for (int b = 0; b < 2; ++b) {
            const pb::PixelBatchEntry* e = reinterpret_cast<const pb::PixelBatchEntry*>(host + c.at[b]);
            CHECK(c.entries[b] == 0 || (e[0].first_wg == 0 && e[c.entries[b] - 1].end_wg == c.wgs[b]));
        }
    }
    std::vector<DxtltPixelBatchAutoItem> big;
    for (uint64_t k = 0; k < 5; ++k)
        big.push_back(auto_item((k + 1) << 40, ((k + 1) << 40) + (1ull << 39), 63ull << 30, 4));
    CHECK(pb::plan_auto_call(big.data(), 5, 256ull << 20, ap).code == kInvalidArgument);
    CHECK(pb::plan_auto_call(big.data(), 4, 256ull << 20, ap).code == kOk && ap.chunks.size() == 4);
    const DxtltPixelBatchAutoItem over[2] = {auto_item(A, B, n, 4), auto_item(A + 0x100000, A + n - 1, n, 4)};
    CHECK(pb::plan_auto_call(over, 2, 256ull << 20, ap).code == kInvalidArgument);
    CHECK(pb::plan_auto_call(nullptr, 2, 256ull << 20, ap).code == kInvalidArgument);

    std::puts("ok");
    return 0;
}
